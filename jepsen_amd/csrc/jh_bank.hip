// jh_bank.hip -- the bank workload checker on MI355X.
//
// jepsen.tests.bank/checker, jepsen/src/jepsen/tests/bank.clj:46-121: every
// :ok :read carries a map {account balance}; per read the first matching error
// of check-op's cond (unexpected-key, nil-balance, wrong-total,
// negative-value), and per error type the count, first, last, worst (and for
// wrong-total the lowest and highest total). A read's map is a CSR range of
// (account code, balance) pairs in aux (include/jh.h).
//
// Pipeline (stage 1's loops and host side are row_select.h):
//   1. k_bank_flag     type / f in 16-byte row-pair loads: the :ok :read rows as
//                      ballot words (one bit per row) and their number per
//                      4096-row tile; an exclusive scan of the tile counts
//      k_bank_compact  value / value2 of the flagged rows: (row, first pair,
//                      count) of every read IN HISTORY ORDER (positions from
//                      the ballot words, no atomic), ranges bounds-checked;
//                      an exclusive scan of the counts -> off
//   2. k_bank_init     per read: the record of an empty read (it owns no
//                      entry, so no entry lane visits it), and for every
//                      1024-entry span boundary a read covers, the span's
//                      first read
//   3. k_bank_entries  the reads' pairs as one virtual concatenation; one wave
//                      per span, 64 pairs per step in 16-byte loads. A step
//                      inside one read adds into per-lane accumulators. In
//                      any other step the reads starting inside it are counted
//                      into 64 LDS words from the next offsets (so empty reads
//                      cost a load, not a search), a ballot or a prefix sum
//                      gives every lane its read, and a segmented scan over
//                      the wave finishes every read that ends in the step.
//                      Positive and negative balances are summed apart, 64
//                      bits plus a carry count each (32 bits across the lanes
//                      while the step's balances are small).
//      k_bank_carry    reads cut by a span edge: the wave that holds a read's
//                      first piece adds up the following waves' pieces, in
//                      order and exactly
//      k_bank_resum    (rare) a read whose positive or negative sum leaves
//                      int64: one lane re-sums it in pair order with overflow
//                      checks -- the reference's (reduce + ...) throws on a
//                      PREFIX, which depends on the order
//   4. k_bank_sum      over the records: per type count, first, last, worst
//      k_bank_fin      (badness, ties to the earlier read), lowest / highest
//                      total; block partials, one finishing block
// No global atomic per read or per wave anywhere; the only atomics are the
// error flags of a malformed range.
#include "row_select.h"

namespace {
constexpr int B_STEPS = 16;
constexpr int64_t B_SPAN = 64 * B_STEPS;     // entries per wave
constexpr int C_RESUM = -1;                  // record class: to be re-summed in order
constexpr long long B_MAX_COUNT = 0x7fffffffLL;

struct BMeta {
    unsigned bad_range, too_long, flagged, pad;
};

// the sums of one run of pairs: positive balances and magnitudes of the
// negative ones as 64 bits + carries (hi: positive carries in the low half,
// negative in the high half), cnt: unexpected keys << 32 | nil balances
struct BSum {
    unsigned long long pos, neg, hi, cnt;
};

__device__ __forceinline__ void bsum_add(BSum &a, const BSum &b) {
    a.pos += b.pos;
    a.neg += b.neg;
    a.hi += b.hi + (a.pos < b.pos ? 1ULL : 0ULL) + (a.neg < b.neg ? 1ULL << 32 : 0ULL);
    a.cnt += b.cnt;
}

struct BPart {                // a piece of a read cut by a span edge
    long long r;              // -1: none
    BSum s;
};

// check-op's cond for a read whose sum is `total`
__device__ __forceinline__ void b_classify(long long total, unsigned long long n_un, unsigned long long n_nil,
                                           unsigned long long negmag, long long want, int negb, int &cls,
                                           unsigned long long &bad) {
    if (n_un) { cls = 1; bad = n_un; }
    else if (n_nil) { cls = 2; bad = n_nil; }
    else if (total != want) {
        cls = 3;
        bad = total > want ? (unsigned long long)total - (unsigned long long)want
                           : (unsigned long long)want - (unsigned long long)total;
    } else if (!negb && negmag) { cls = 4; bad = negmag; }
    else { cls = 0; bad = 0; }
}

// Every prefix of the read's sum lies in [-neg, pos]: when both fit int64 no
// prefix overflows and the total is pos - neg; otherwise the order decides.
__device__ __forceinline__ void b_finish(const BSum &s, long long r, long long want, int negb,
                                         long long *__restrict__ tot, unsigned long long *__restrict__ bad,
                                         int *__restrict__ cls, BMeta *m) {
    const bool fits = s.hi == 0 && s.pos <= 0x7fffffffffffffffULL && s.neg <= 0x8000000000000000ULL;
    if (!fits) {
        cls[r] = C_RESUM;
        m->flagged = 1;
        return;
    }
    int c;
    unsigned long long b;
    const long long total = (long long)(s.pos - s.neg);
    b_classify(total, s.cnt >> 32, s.cnt & 0xffffffffULL, s.neg, want, negb, c, b);
    tot[r] = total; bad[r] = b; cls[r] = c;
}

// ---------------------------------------------------------------------------
// 1. the :ok :read rows (row_select.h, pair layout, one kind)
__global__ void __launch_bounds__(256) k_bank_flag(const int64_t *__restrict__ type, const int64_t *__restrict__ f,
                                                   int64_t n, int vec, unsigned long long *__restrict__ words,
                                                   long long *__restrict__ tile_cnt) {
    rs_flag_pairs<1>(type, f, n, vec, words, tile_cnt,
                     [](int, const long long &t, const long long &ff) { return t == T_OK && ff == JH_F_READ; });
}

// (row, first pair, count) of every read, in history order
__global__ void __launch_bounds__(256) k_bank_compact(const int64_t *__restrict__ value, const int64_t *__restrict__ value2,
                                                      int64_t n, int vec, const unsigned long long *__restrict__ words,
                                                      const long long *__restrict__ tile_base, int64_t half,
                                                      int64_t *__restrict__ row, int64_t *__restrict__ start,
                                                      int64_t *__restrict__ cnt, BMeta *m) {
    rs_compact_pairs(n, words, tile_base, [&](int64_t p, bool r0, bool r1, long long o) {
        const longlong2 v2 = ld_pair(value, p, n, vec), c2 = ld_pair(value2, p, n, vec);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (!(h ? r1 : r0)) continue;
            long long v = h ? v2.y : v2.x, c = h ? c2.y : c2.x;
            if (v == JH_NIL) { v = 0; c = 0; }            // a nil :value is the empty map
            else if (v < 0 || c < 0 || v > half || c > half - v) { atomicOr(&m->bad_range, 1u); v = 0; c = 0; }
            else if (c > B_MAX_COUNT) { atomicOr(&m->too_long, 1u); v = 0; c = 0; }
            row[o] = 2 * p + h; start[o] = v; cnt[o] = c;
            o++;
        }
    });
}

// ---------------------------------------------------------------------------
// 2. empty reads get their record here; every span learns its first read
__global__ void __launch_bounds__(256) k_bank_init(const int64_t *__restrict__ off, int64_t R, long long want,
                                                   long long *__restrict__ first, long long *__restrict__ tot,
                                                   unsigned long long *__restrict__ bad, int *__restrict__ cls) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o0 = off[r], o1 = off[r + 1];
        if (o0 == o1) {
            int c;
            unsigned long long b;
            b_classify(0, 0, 0, 0, want, 1, c, b);
            tot[r] = 0; bad[r] = b; cls[r] = c;
        } else {
            for (int64_t s = (o0 + B_SPAN - 1) / B_SPAN; s * B_SPAN < o1; s++) first[s] = r;
        }
    }
}

// ---------------------------------------------------------------------------
// 3. the entry pass: one wave per span of B_SPAN entries.
__device__ __forceinline__ BSum b_wave_sum(BSum a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        BSum x;
        x.pos = __shfl_xor(a.pos, o); x.neg = __shfl_xor(a.neg, o);
        x.hi = __shfl_xor(a.hi, o); x.cnt = __shfl_xor(a.cnt, o);
        bsum_add(a, x);
    }
    return a;
}

__device__ __forceinline__ BSum b_entry(const int64_t *__restrict__ aux, int vec, int64_t q, long long n_accounts) {
    const longlong2 pr = vec ? ((const longlong2 *)aux)[q] : make_longlong2(aux[2 * q], aux[2 * q + 1]);
    const bool un = pr.x < 0 || pr.x >= n_accounts, nil = pr.y == JH_NIL;
    BSum s = {0, 0, 0, ((unsigned long long)un << 32) | (unsigned long long)nil};
    if (!nil) {
        if (pr.y > 0) s.pos = (unsigned long long)pr.y;
        else s.neg = 0ULL - (unsigned long long)pr.y;
    }
    return s;
}

// rc is the read of the step's first entry. The wave keeps off[rc + 1 + lane]
// and start[rc + 1 + lane] in registers while rc stays: a step that lies
// strictly inside read rc only adds into per-lane accumulators (no cross-lane
// work, no dependent load before the pairs); any other step counts the reads
// that start inside it into 64 LDS words (so empty reads cost a load, not a
// search), takes every lane's offsets from those registers, and runs a
// segmented scan over the wave.
__global__ void __launch_bounds__(256) k_bank_entries(const int64_t *__restrict__ aux, int vec,
                                                      const int64_t *__restrict__ off, const int64_t *__restrict__ start,
                                                      int64_t R, int64_t E, const long long *__restrict__ first,
                                                      long long n_accounts, long long want, int negb,
                                                      long long *__restrict__ tot, unsigned long long *__restrict__ bad,
                                                      int *__restrict__ cls, BPart *__restrict__ parts, BMeta *m) {
    __shared__ unsigned head_all[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned *head = head_all[wave];
    const int64_t w = blockIdx.x * 4LL + wave;
    const int64_t span0 = w * B_SPAN;
    if (span0 >= E) return;                                // wave-uniform; no block barrier below
    const int64_t span1 = std::min<int64_t>(E, span0 + B_SPAN);
    long long rc = first[w];                               // the read holding entry span0
    const long long off_first = off[rc];
    long long d_rc = start[rc] - off_first;                // start[rc] - off[rc]
    const long long r_head = off_first < span0 ? rc : -1;     // a read that began in an earlier span
    bool head_done = false, carrying = false, have = false;
    long long o = 0, sv = 0;                               // off / start of read rc + 1 + lane (off[R] = E)
    BSum acc = {0, 0, 0, 0};                               // per lane: the read carried over a step edge
    for (int64_t e0 = span0; e0 < span1; e0 += 64) {
        const int64_t e = e0 + lane;
        const bool live = e < span1;
        if (!have) {
            const long long j = rc + 1 + lane;
            o = j <= R ? off[j] : LLONG_MAX;
            sv = j < R ? start[j] : 0;
            have = true;
        }
        if (__shfl(o, 0) > e0 + 64 && e0 + 64 <= span1) {    // the step lies strictly inside read rc
            bsum_add(acc, b_entry(aux, vec, d_rc + e, n_accounts));
            carrying = true;
            continue;
        }
        // the read of every lane: rc + the reads that start in (e0, e]
        head[lane] = 0;
        __threadfence_block();
        bool multi = false;
        for (long long j = rc + 1 + lane;;) {
            const long long p = o > e0 ? o - e0 : 0;
            const bool in = j < R && p < 64;
            if (in) atomicAdd(&head[p], 1u);
            if (!__shfl((int)in, 63)) break;               // the last offset seen lies past the step
            multi = true;                                  // more than 64 reads start here: empty ones
            j += 64;
            o = j <= R ? off[j] : LLONG_MAX;
        }
        __threadfence_block();
        unsigned inc = head[lane];
        if (!__any(inc > 1)) {                             // no two reads start on one entry: a ballot will do
            inc = __popcll(__ballot(inc == 1) & ((2ULL << lane) - 1));
        } else {
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned x = __shfl_up(inc, d);
                if (lane >= d) inc += x;
            }
        }
        const long long r = rc + inc;
        long long d_r;                                     // start[r] - off[r]
        if (!multi) {                                      // inc <= 63: the offsets are in the wave's registers
            const int k = (int)inc - 1;
            const long long dd = __shfl(sv - o, k < 0 ? 0 : k);
            d_r = k < 0 ? d_rc : dd;
        } else {
            d_r = start[r] - off[r];
        }
        BSum s = {0, 0, 0, 0};
        if (live) s = b_entry(aux, vec, d_r + e, n_accounts);
        if (carrying) {                                    // lane 0 continues the read of the step before
            const BSum c = b_wave_sum(acc);
            if (lane == 0) bsum_add(s, c);
        }
        // segmented inclusive scan: inc does not decrease with the lane. Cross-lane moves go
        // through the LDS unit, which the CU's four SIMDs share, so they are kept few: balances
        // below 2^25 (and no carry so far) are summed in 32 bits, the counts only when there are any
        if (!__any(((s.pos | s.neg) >> 25) != 0 || s.hi != 0)) {
            unsigned sp = (unsigned)s.pos, sn = (unsigned)s.neg;
            const bool anyc = __any(s.cnt != 0);
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned px = __shfl_up(sp, d), nx = __shfl_up(sn, d), ix = __shfl_up(inc, d);
                const bool same = lane >= d && ix == inc;
                if (same) { sp += px; sn += nx; }
                if (anyc) {
                    const unsigned long long cx = __shfl_up(s.cnt, d);
                    if (same) s.cnt += cx;
                }
            }
            s.pos = sp; s.neg = sn;
        } else {
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                BSum x;
                x.pos = __shfl_up(s.pos, d); x.neg = __shfl_up(s.neg, d);
                x.hi = __shfl_up(s.hi, d); x.cnt = __shfl_up(s.cnt, d);
                const unsigned ix = __shfl_up(inc, d);
                if (lane >= d && ix == inc) bsum_add(s, x);
            }
        }
        const unsigned inc_next = __shfl_down(inc, 1);
        const unsigned inc63 = __shfl(inc, 63);
        const long long r63 = rc + inc63;                  // r63 < R and off has R + 1 entries
        const long long o63r = __shfl(o, multi ? 0 : (int)inc63);
        const long long o63 = multi ? off[r63 + 1] : o63r;
        const bool end = live && (e + 1 == E || (lane < 63 ? inc_next != inc : o63 == e + 1));
        if (end) {
            if (r == r_head) {
                BPart *pp = parts + 2 * w;
                pp->r = r; pp->s = s;
            } else {
                b_finish(s, r, want, negb, tot, bad, cls, m);
            }
        }
        const unsigned long long endm = __ballot(end);
        head_done = head_done || __any(end && r == r_head);
        carrying = e0 + 63 < span1 && !(endm >> 63);
        const BSum zero = {0, 0, 0, 0};
        acc = carrying && lane == 63 ? s : zero;
        d_rc = __shfl(d_r, 63);                            // lane 63 is live whenever another step follows
        if (multi || r63 != rc) have = false;
        rc = r63;
    }
    const BSum carry = b_wave_sum(acc);
    if (lane == 0) {
        BPart *hp = parts + 2 * w, *tp = hp + 1;
        const bool whole = carrying && rc == r_head;       // one read covers the whole span
        if (!head_done) {
            if (whole) { hp->r = rc; hp->s = carry; }
            else hp->r = -1;
        }
        if (carrying && !whole) { tp->r = rc; tp->s = carry; }
        else tp->r = -1;
    }
}

// a read's first piece is the tail piece of its wave; the pieces that follow
// are the head pieces of the next waves, one per wave without a gap
__global__ void __launch_bounds__(256) k_bank_carry(const BPart *__restrict__ parts, int64_t W, long long want, int negb,
                                                    long long *__restrict__ tot, unsigned long long *__restrict__ bad,
                                                    int *__restrict__ cls, BMeta *m) {
    for (int64_t w = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; w < W; w += (int64_t)gridDim.x * blockDim.x) {
        const long long r = parts[2 * w + 1].r;
        if (r < 0) continue;
        BSum s = parts[2 * w + 1].s;
        for (int64_t j = w + 1; j < W && parts[2 * j].r == r; j++) bsum_add(s, parts[2 * j].s);
        b_finish(s, r, want, negb, tot, bad, cls, m);
    }
}

// one lane per flagged read, sequentially in pair order
__global__ void __launch_bounds__(256) k_bank_resum(const int64_t *__restrict__ aux, const int64_t *__restrict__ start,
                                                    const int64_t *__restrict__ cnt, int64_t R, long long n_accounts,
                                                    long long want, int negb, long long *__restrict__ tot,
                                                    unsigned long long *__restrict__ bad, int *__restrict__ cls) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
        if (cls[r] != C_RESUM) continue;
        const int64_t q0 = start[r], c = cnt[r];
        long long sum = 0;
        unsigned long long n_un = 0, n_nil = 0, negmag = 0;
        bool ovf = false, negsat = false;
        for (int64_t i = 0; i < c; i++) {
            const long long code = aux[2 * (q0 + i)], b = aux[2 * (q0 + i) + 1];
            n_un += code < 0 || code >= n_accounts;
            if (b == JH_NIL) { n_nil++; continue; }
            if (!ovf && __builtin_add_overflow(sum, b, &sum)) ovf = true;
            if (b < 0) {
                const unsigned long long mag = 0ULL - (unsigned long long)b;
                negmag += mag;
                if (negmag < mag) negsat = true;
            }
        }
        if (negsat) negmag = ~0ULL;
        int k;
        unsigned long long b;
        if (ovf) {
            b_classify(0, n_un, n_nil, 0, 0, 1, k, b);      // only the key and nil tests can be decided
            tot[r] = JH_NIL; bad[r] = b; cls[r] = k | 8;
        } else {
            b_classify(sum, n_un, n_nil, negmag, want, negb, k, b);
            tot[r] = sum; bad[r] = b; cls[r] = k;
        }
    }
}

// ---------------------------------------------------------------------------
// 4. summary. Positions are read numbers (they grow with the row).
constexpr long long NONE_R = LLONG_MAX;
struct BAcc {
    long long cnt[4], first[4], last[4], wr[4];
    unsigned long long wbad[4];
    long long lo_t, lo_r, hi_t, hi_r, unknown;

    __device__ void clear() {
        for (int t = 0; t < 4; t++) { cnt[t] = 0; first[t] = NONE_R; last[t] = -1; wr[t] = NONE_R; wbad[t] = 0; }
        lo_t = LLONG_MAX; lo_r = NONE_R; hi_t = LLONG_MIN; hi_r = NONE_R; unknown = 0;
    }
    __device__ void worst(int t, unsigned long long b, long long r) {
        if (r != NONE_R && (wr[t] == NONE_R || b > wbad[t] || (b == wbad[t] && r < wr[t]))) { wbad[t] = b; wr[t] = r; }
    }
    __device__ void lowest(long long v, long long r) {
        if (r != NONE_R && (lo_r == NONE_R || v < lo_t || (v == lo_t && r < lo_r))) { lo_t = v; lo_r = r; }
    }
    __device__ void highest(long long v, long long r) {
        if (r != NONE_R && (hi_r == NONE_R || v > hi_t || (v == hi_t && r < hi_r))) { hi_t = v; hi_r = r; }
    }
    __device__ void merge(const BAcc &o) {
        for (int t = 0; t < 4; t++) {
            cnt[t] += o.cnt[t];
            first[t] = first[t] < o.first[t] ? first[t] : o.first[t];
            last[t] = last[t] > o.last[t] ? last[t] : o.last[t];
            worst(t, o.wbad[t], o.wr[t]);
        }
        lowest(o.lo_t, o.lo_r);
        highest(o.hi_t, o.hi_r);
        unknown += o.unknown;
    }
};
constexpr int ACC_WORDS = sizeof(BAcc) / 8;

__device__ __forceinline__ void acc_block_reduce(BAcc &a, BAcc *sh /* [4] shared */) {
    for (int o = 32; o > 0; o >>= 1) {
        BAcc x;
        long long *src = (long long *)&a, *dst = (long long *)&x;
#pragma unroll
        for (int i = 0; i < ACC_WORDS; i++) dst[i] = __shfl_xor(src[i], o);
        a.merge(x);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) { a = sh[0]; a.merge(sh[1]); a.merge(sh[2]); a.merge(sh[3]); }
}

__global__ void __launch_bounds__(256) k_bank_sum(const long long *__restrict__ tot, const unsigned long long *__restrict__ bad,
                                                  const int *__restrict__ cls, int64_t R, BAcc *__restrict__ parts) {
    __shared__ BAcc sh[4];
    BAcc a;
    a.clear();
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
        const int c = cls[r];
        if (c == 0) continue;
        if (c == 8) { a.unknown++; continue; }
        const int t = (c & 7) - 1;
        a.cnt[t]++;
        if (a.first[t] == NONE_R) a.first[t] = r;
        a.last[t] = r;
        a.worst(t, bad[r], r);
        if (t == 2) { const long long v = tot[r]; a.lowest(v, r); a.highest(v, r); }
    }
    acc_block_reduce(a, sh);
    if (threadIdx.x == 0) parts[blockIdx.x] = a;
}

struct BOut {
    long long unknown, first_error_row;
    long long cnt[4], first_row[4], last_row[4], worst_row[4], worst_bad[4], lowest_row, highest_row;
};

__global__ void __launch_bounds__(256) k_bank_fin(const BAcc *__restrict__ parts, int np, const int64_t *__restrict__ row,
                                                  BOut *out) {
    __shared__ BAcc sh[4];
    BAcc a;
    a.clear();
    for (int i = threadIdx.x; i < np; i += 256) a.merge(parts[i]);
    acc_block_reduce(a, sh);
    if (threadIdx.x == 0) {
        long long fe = NONE_R;
        for (int t = 0; t < 4; t++) {
            const bool any = a.cnt[t] > 0;
            out->cnt[t] = a.cnt[t];
            out->first_row[t] = any ? row[a.first[t]] : -1;
            out->last_row[t] = any ? row[a.last[t]] : -1;
            out->worst_row[t] = any ? row[a.wr[t]] : -1;
            out->worst_bad[t] = any ? (long long)a.wbad[t] : 0;
            if (any && a.first[t] < fe) fe = a.first[t];
        }
        out->lowest_row = a.cnt[2] ? row[a.lo_r] : -1;
        out->highest_row = a.cnt[2] ? row[a.hi_r] : -1;
        out->first_error_row = fe == NONE_R ? -1 : row[fe];
        out->unknown = a.unknown;
    }
}

__global__ void __launch_bounds__(256) k_bank_triples(const int64_t *__restrict__ row, const long long *__restrict__ tot,
                                                      const int *__restrict__ cls, int64_t k, int64_t *__restrict__ out) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < k; r += (int64_t)gridDim.x * blockDim.x) {
        out[3 * r] = row[r]; out[3 * r + 1] = tot[r]; out[3 * r + 2] = cls[r];
    }
}

}  // namespace

void bank_check(jh_ctx *ctx, const jh_history *dh, const jh_bank_opts *opts, jh_bank_result *res,
                int64_t *reads_out, int64_t reads_cap, int64_t *n_reads, hipStream_t st) {
    memset(res, 0, sizeof *res);
    res->valid = JH_VALID;
    res->first_error_row = -1;
    for (auto &e : res->errors) e.first_row = e.last_row = e.worst_row = e.lowest_row = e.highest_row = -1;
    if (n_reads) *n_reads = 0;
    const int64_t n = dh->n;
    if (dh->n_aux < 0 || (dh->n_aux & 1)) throw_jh(JH_EINVAL, "bank: n_aux must be even and >= 0 (pairs)");
    if (n == 0) return;
    if (n > 0x7fffffff00LL) throw_jh(JH_EUNSUPPORTED, "bank: more than 2^39 rows");
    DeviceTimer timer{ctx, st};
    timer.start();
    const long long want = opts->total_amount;
    const int negb = opts->negative_balances != 0;
    const int64_t half = dh->n_aux / 2;

    // 1. the reads, in history order
    BMeta *m = ctx->ws<BMeta>(WS_B_META, 1);
    HIP_TRY(hipMemsetAsync(m, 0, sizeof *m, st));
    const int vec = (((uintptr_t)dh->type | (uintptr_t)dh->f | (uintptr_t)dh->value | (uintptr_t)dh->value2) & 15) == 0;
    const RowSel<1> sel = select_rows<1>(
        ctx, {WS_B_WORDS, WS_B_TCNT, WS_B_TBASE, WS_B_TMP}, n, 2 * RS_TILE, RS_WORDS,
        [&](int g, unsigned long long *words, long long *tile_cnt) {
            k_bank_flag<<<g, 256, 0, st>>>(dh->type, dh->f, n, vec, words, tile_cnt);
        }, st);
    const long long R = sel.count[0];
    res->read_count = R;
    if (n_reads) *n_reads = R;
    if (R == 0) { res->device_ms = timer.stop(); return; }
    if (R >= 0x7fffffffLL) throw_jh(JH_EUNSUPPORTED, "bank: more than 2^31 - 2 reads");
    if (half > 0 && !dh->aux) throw_jh(JH_EINVAL, "bank: n_aux > 0 without aux");

    int64_t *row = ctx->ws<int64_t>(WS_B_ROW, R);
    int64_t *start = ctx->ws<int64_t>(WS_B_START, R);
    int64_t *cnt = ctx->ws<int64_t>(WS_B_CNT, R + 1);
    int64_t *off = ctx->ws<int64_t>(WS_B_OFF, R + 1);
    long long *tot = ctx->ws<long long>(WS_B_TOT, R);
    unsigned long long *bad = ctx->ws<unsigned long long>(WS_B_BAD, R);
    int *cls = ctx->ws<int>(WS_B_CLS, R);
    HIP_TRY(hipMemsetAsync(cnt + R, 0, sizeof(int64_t), st));
    k_bank_compact<<<sel.grid, 256, 0, st>>>(dh->value, dh->value2, n, vec, sel.words[0], sel.base[0], half, row, start,
                                             cnt, m);
    excl_sum(ctx, WS_B_TMP, as_input(cnt), off, (int)(R + 1), st);
    struct { BMeta m; long long E; } hb;
    HIP_TRY(hipMemcpyAsync(&hb.m, m, sizeof hb.m, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&hb.E, off + R, sizeof hb.E, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hb.m.bad_range) throw_jh(JH_EINVAL, "bank: a read's pair range leaves [0, n_aux / 2) or has a negative count");
    if (hb.m.too_long) throw_jh(JH_EUNSUPPORTED, "bank: a read of more than 2^31 - 1 pairs");
    const int64_t E = hb.E;
    res->entries = E;

    // 2 / 3. records
    const int64_t W = (E + B_SPAN - 1) / B_SPAN;
    long long *first = ctx->ws<long long>(WS_B_FIRST, W);
    k_bank_init<<<grid_for(R, 256, 2048), 256, 0, st>>>(off, R, want, first, tot, bad, cls);
    if (E > 0) {
        BPart *parts = ctx->ws<BPart>(WS_B_PARTS, 2 * W);
        const int avec = ((uintptr_t)dh->aux & 15) == 0;
        if ((W + 3) / 4 > 0x7fffffffLL) throw_jh(JH_EUNSUPPORTED, "bank: too many pairs");
        k_bank_entries<<<(unsigned)((W + 3) / 4), 256, 0, st>>>(dh->aux, avec, off, start, R, E, first, opts->n_accounts,
                                                                want, negb, tot, bad, cls, parts, m);
        k_bank_carry<<<grid_for(W, 256, 2048), 256, 0, st>>>(parts, W, want, negb, tot, bad, cls, m);
        HIP_TRY(hipMemcpyAsync(&hb.m, m, sizeof hb.m, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (hb.m.flagged)
            k_bank_resum<<<grid_for(R, 256, 2048), 256, 0, st>>>(dh->aux, start, cnt, R, opts->n_accounts, want, negb,
                                                                 tot, bad, cls);
    }

    // 4. summary
    const int gs = grid_for(R, 256, 1024);
    BAcc *accs = ctx->ws<BAcc>(WS_B_ACC, gs);
    BOut *out = ctx->ws<BOut>(WS_B_OUT, 1);
    k_bank_sum<<<gs, 256, 0, st>>>(tot, bad, cls, R, accs);
    k_bank_fin<<<1, 256, 0, st>>>(accs, gs, row, out);
    BOut ho;
    HIP_TRY(hipMemcpyAsync(&ho, out, sizeof ho, hipMemcpyDeviceToHost, st));
    const int64_t k = reads_out ? std::min<int64_t>(R, reads_cap) : 0;
    if (k > 0) {
        int64_t *tri = ctx->ws<int64_t>(WS_B_TRI, 3 * k);
        k_bank_triples<<<grid_for(k, 256, 2048), 256, 0, st>>>(row, tot, cls, k, tri);
        HIP_TRY(hipMemcpyAsync(reads_out, tri, sizeof(int64_t) * 3 * k, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (int t = 0; t < 4; t++) {
        jh_bank_err &e = res->errors[t];
        e.count = ho.cnt[t]; e.first_row = ho.first_row[t]; e.last_row = ho.last_row[t];
        e.worst_row = ho.worst_row[t]; e.worst_badness = ho.worst_bad[t];
        res->error_count += ho.cnt[t];
    }
    res->errors[2].lowest_row = ho.lowest_row;
    res->errors[2].highest_row = ho.highest_row;
    res->first_error_row = ho.first_error_row;
    if (ho.unknown > 0) { res->valid = JH_UNKNOWN; res->cause = JH_CAUSE_OVERFLOW; }
    else res->valid = res->error_count ? JH_INVALID : JH_VALID;
    res->device_ms = timer.stop();
}
