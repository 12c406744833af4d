// jh_longfork.hip -- the long-fork workload checker on MI355X.
//
// jepsen.tests.long-fork/checker, jepsen/src/jepsen/tests/long_fork.clj:158-324:
// the :ok read txns are grouped by key set (groups of n keys, group-for); two
// reads of a group fork when each has a non-nil value where the other has nil.
// A read of n keys is an n-bit "seen" mask, a fork is two masks neither of
// which contains the other, and "no group forks" is decided from integer
// counters without pairwise work (stage 4); pairs are listed only for the
// reads of groups already known to be broken (stage 5).
//
// Pipeline:
//   1. k_lf_flag       type / f in 16-byte row-pair loads: the :ok read rows
//                      and the :invoke write rows as ballot words and their
//                      numbers per 4096-row tile (jh_bank's scheme: row_select.h);
//                      exclusive scans of the tile counts
//      k_lf_compact    value / value2 of the flagged rows, in history order
//                      from the ballot words (no atomic): reads as (row, first
//                      pair, count), ranges bounds-checked; writes as (key,
//                      row) with the min / max written key
//      k_lf_reads      per read (1 to 16 lanes each): shape (count == n, keys
//                      the aligned group, no key twice), group floor(k / n),
//                      seen-mask (bit k mod n), early / late; counts, min /
//                      max group
//   2. multiple writes the smallest row that is not the first write of its key
//      dense           k_lf_first (atomicMin into a first-row table indexed by
//                      key - min) and k_lf_repeat (min over rows that differ
//                      from their key's entry)
//      sparse          stable radix sort of key - min, k_lf_repeat_sorted (min
//                      of row[i] over key[i] == key[i - 1])
//   3. group slots     dense: group - min group. sparse: sort the groups, flag
//                      the starts, exclusive sum, scatter the rank back
//   4. k_lf_count      pass A over the pairs: cnt[slot * n + bit] += 1 for
//                      every non-nil pair (lanes of a wave on one word are
//                      combined first) and a compare-and-set on the value
//                      table; two distinct values mark the word
//      k_lf_test       pass B, one lane per read: it fails when the min of cnt
//                      over its set bits <= the max over its clear bits; a
//                      failing read sets its group's bit
//   5. listing         (only with a flagged group) every read of a flagged
//                      group, stably sorted by slot; k_lf_pairs, one wave per
//                      suspect over the later suspects of its group: counts,
//                      exclusive sum, then the pairs in order up to fork_cap
#include "row_select.h"

namespace {
constexpr unsigned long long SIGN = 1ULL << 63;
constexpr unsigned long long NONE = ~0ULL;
constexpr unsigned CONFLICT = 1u << 31;      // cnt word: two distinct non-nil values seen
constexpr unsigned long long DENSE_MAX = 1ULL << 28;   // table entries a forced dense path may ask for
constexpr long long L_MAX_COUNT = 0x7ffffffeLL;

struct LMeta {
    unsigned bad_range, unsup, conflict, any_fail;
    // order-preserving unsigned images (x ^ SIGN) of signed minima / maxima
    unsigned long long gmin, gmax, kmin, kmax;
    unsigned long long ill1_row, ill2_row;      // smallest rows, NONE: none
    unsigned long long mw_row;                  // smallest repeated write row
    unsigned long long reads_early, reads_late, entries, fork_groups;
    int n_sel, pad;
};

__device__ __forceinline__ unsigned long long ord(long long x) { return (unsigned long long)x ^ SIGN; }

__global__ void k_lf_meta_init(LMeta *m) {
    memset(m, 0, sizeof *m);
    m->gmin = m->kmin = NONE;
    m->ill1_row = m->ill2_row = m->mw_row = NONE;
}

// Clojure's floored mod / quot for 1 <= n <= 64
__device__ __forceinline__ void floor_divmod(long long k, long long n, long long &q, int &r) {
    q = k / n;
    long long rem = k - q * n;
    if (rem < 0) { rem += n; q--; }
    r = (int)rem;
}

// ---------------------------------------------------------------------------
// 1. the :ok read rows (kind 0) and the :invoke write rows (kind 1): row_select.h, pair layout
__global__ void __launch_bounds__(256) k_lf_flag(const int64_t *__restrict__ type, const int64_t *__restrict__ f,
                                                 int64_t n, int vec, unsigned long long *__restrict__ words,
                                                 long long *__restrict__ tile_cnt) {
    rs_flag_pairs<2>(type, f, n, vec, words, tile_cnt, [](int k, const long long &t, const long long &ff) {
        return k ? t == T_INVOKE && ff == JH_F_WRITE : t == T_OK && ff == JH_F_READ;
    });
}

// The flagged rows of one kind, in history order.
// WR = 0: reads -> (row, first pair, count), a[o] = row, b[o] = start, c[o] = count.
// WR = 1: writes -> a[o] = key, b[o] = row; min / max key into the meta.
template <int WR>
__global__ void __launch_bounds__(256) k_lf_compact(const int64_t *__restrict__ value, const int64_t *__restrict__ value2,
                                                    int64_t n, int vec, const unsigned long long *__restrict__ words,
                                                    const long long *__restrict__ tile_base, int64_t half,
                                                    int64_t *__restrict__ a, int64_t *__restrict__ b,
                                                    int64_t *__restrict__ c, LMeta *m) {
    __shared__ unsigned long long shr[4];
    unsigned long long kmin = NONE, kmax = 0;
    rs_compact_pairs(n, words, tile_base, [&](int64_t p, bool r0, bool r1, long long o) {
        const longlong2 v2 = ld_pair(value, p, n, vec);
        longlong2 c2 = make_longlong2(0, 0);
        if (!WR) c2 = ld_pair(value2, p, n, vec);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (!(h ? r1 : r0)) continue;
            long long v = h ? v2.y : v2.x, cc = h ? c2.y : c2.x;
            if (WR) {
                a[o] = v; b[o] = 2 * p + h;
                kmin = min(kmin, ord(v)); kmax = max(kmax, ord(v));
            } else {
                if (v == JH_NIL && cc == 0) v = 0;        // a nil :value: no pairs
                else if (v < 0 || cc < 0 || v > half || cc > half - v) { atomicOr(&m->bad_range, 1u); v = 0; cc = 0; }
                a[o] = 2 * p + h; b[o] = v; c[o] = cc;
            }
            o++;
        }
    });
    if (WR) {
        kmin = block_reduce256(kmin, RedMin(), shr);
        kmax = block_reduce256(kmax, RedMax(), shr);
        if (threadIdx.x == 0 && kmin != NONE) { atomicMin(&m->kmin, kmin); atomicMax(&m->kmax, kmax); }
    }
}

// per read: shape, group, seen-mask, early / late. L lanes share a read (L a
// power of two <= 16 near n, so one load instruction of a read's lanes covers
// L consecutive pairs); lane `sub` takes the pairs sub, sub + L, ... and the L
// partial results are folded with shuffles. 256 is a multiple of L: the lanes
// of a read lie in one wave.
__global__ void __launch_bounds__(256) k_lf_reads(const int64_t *__restrict__ aux, const int64_t *__restrict__ row,
                                                  const int64_t *__restrict__ start, const int64_t *__restrict__ cnt,
                                                  int64_t R, long long n, int logL, long long *__restrict__ grp,
                                                  unsigned long long *__restrict__ mask, LMeta *m) {
    __shared__ unsigned long long sh[4];
    const unsigned long long full = n == 64 ? ~0ULL : (1ULL << n) - 1;
    const int L = 1 << logL;
    const bool vec = ((uintptr_t)aux & 15) == 0;                // aux holds int64 pairs: 16-byte aligned with it
    unsigned long long early = 0, late = 0, ent = 0, gmin = NONE, gmax = 0, ill = NONE;
    unsigned unsup = 0;
    const int64_t total = R << logL;
    for (int64_t t0 = blockIdx.x * 256LL; t0 < total; t0 += (int64_t)gridDim.x * 256) {   // block-uniform
        const int64_t t = t0 + threadIdx.x, r = t >> logL;
        const int sub = (int)(t & (L - 1));
        const bool have = r < R;
        const int64_t q0 = have ? start[r] : 0, c = have ? cnt[r] : 0;
        const longlong2 *pr = (const longlong2 *)aux + q0;
        unsigned any = 0, nils = 0;
        unsigned long long seen = 0, pos = 0, glo = NONE, ghi = 0;
        for (int64_t j = sub; j < c; j += L) {
            const longlong2 kv = vec ? pr[j] : make_longlong2(aux[2 * (q0 + j)], aux[2 * (q0 + j) + 1]);
            const bool nil = kv.y == JH_NIL;
            any |= !nil; nils |= nil;
            if (c == n) {
                long long g;
                int bit;
                floor_divmod(kv.x, n, g, bit);
                glo = min(glo, ord(g)); ghi = max(ghi, ord(g));
                pos |= 1ULL << bit;
                if (!nil) seen |= 1ULL << bit;
            }
        }
        for (int o = L >> 1; o > 0; o >>= 1) {
            any |= __shfl_xor(any, o); nils |= __shfl_xor(nils, o);
            seen |= __shfl_xor(seen, o); pos |= __shfl_xor(pos, o);
            glo = min(glo, (unsigned long long)__shfl_xor(glo, o)); ghi = max(ghi, (unsigned long long)__shfl_xor(ghi, o));
        }
        if (!have || sub != 0) continue;                          // nothing below is cross-lane
        early += !any; late += !nils; ent += (unsigned long long)c;
        if (c != n) {
            ill = min(ill, (unsigned long long)row[r]);
            grp[r] = 0; mask[r] = 0;
            continue;
        }
        if (glo != ghi || pos != full) unsup = 1;                // not the aligned group, or a key twice
        grp[r] = (long long)(glo ^ SIGN); mask[r] = seen;
        gmin = min(gmin, glo); gmax = max(gmax, ghi);
    }
    early = block_reduce256(early, RedSum(), sh);
    late = block_reduce256(late, RedSum(), sh);
    ent = block_reduce256(ent, RedSum(), sh);
    gmin = block_reduce256(gmin, RedMin(), sh);
    gmax = block_reduce256(gmax, RedMax(), sh);
    ill = block_reduce256(ill, RedMin(), sh);
    unsup = (unsigned)block_reduce256((unsigned long long)unsup, RedOr(), sh);
    if (threadIdx.x == 0) {
        if (early) atomicAdd(&m->reads_early, early);
        if (late) atomicAdd(&m->reads_late, late);
        if (ent) atomicAdd(&m->entries, ent);
        if (gmin != NONE) { atomicMin(&m->gmin, gmin); atomicMax(&m->gmax, gmax); }
        if (ill != NONE) atomicMin(&m->ill1_row, ill);
        if (unsup) atomicOr(&m->unsup, 1u);
    }
}

// ---------------------------------------------------------------------------
// 2. multiple writes
__global__ void __launch_bounds__(256) k_lf_fill(unsigned long long *__restrict__ p, int64_t cnt, unsigned long long v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

__global__ void __launch_bounds__(256) k_lf_first(const int64_t *__restrict__ wkey, const int64_t *__restrict__ wrow,
                                                  int64_t W, unsigned long long kmin,
                                                  unsigned long long *__restrict__ first) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < W; i += (int64_t)gridDim.x * blockDim.x)
        atomicMin(&first[(unsigned long long)wkey[i] - kmin], (unsigned long long)wrow[i]);
}

__global__ void __launch_bounds__(256) k_lf_repeat(const int64_t *__restrict__ wkey, const int64_t *__restrict__ wrow,
                                                   int64_t W, unsigned long long kmin,
                                                   const unsigned long long *__restrict__ first, LMeta *m) {
    __shared__ unsigned long long sh[4];
    unsigned long long best = NONE;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < W; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long r = (unsigned long long)wrow[i];
        if (first[(unsigned long long)wkey[i] - kmin] != r) best = min(best, r);
    }
    best = block_reduce256(best, RedMin(), sh);
    if (threadIdx.x == 0 && best != NONE) atomicMin(&m->mw_row, best);
}

// sparse: the keys key - min and the positions 0..W-1 (rows ascend with them)
__global__ void __launch_bounds__(256) k_lf_wkeys(const int64_t *__restrict__ wkey, int64_t W, unsigned long long kmin,
                                                  unsigned long long *__restrict__ keys, uint32_t *__restrict__ idx) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < W; i += (int64_t)gridDim.x * blockDim.x) {
        keys[i] = (unsigned long long)wkey[i] - kmin;
        idx[i] = (uint32_t)i;
    }
}

__global__ void __launch_bounds__(256) k_lf_repeat_sorted(const unsigned long long *__restrict__ keys,
                                                          const uint32_t *__restrict__ idx,
                                                          const int64_t *__restrict__ wrow, int64_t W, LMeta *m) {
    __shared__ unsigned long long sh[4];
    unsigned long long best = NONE;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < W; i += (int64_t)gridDim.x * blockDim.x)
        if (i > 0 && keys[i] == keys[i - 1]) best = min(best, (unsigned long long)wrow[idx[i]]);
    best = block_reduce256(best, RedMin(), sh);
    if (threadIdx.x == 0 && best != NONE) atomicMin(&m->mw_row, best);
}

// ---------------------------------------------------------------------------
// 3. group slots
__global__ void __launch_bounds__(256) k_lf_slot_dense(const long long *__restrict__ grp, int64_t R,
                                                       unsigned long long gmin, uint32_t *__restrict__ slot) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x)
        slot[r] = (uint32_t)((unsigned long long)grp[r] - gmin);
}

__global__ void __launch_bounds__(256) k_lf_gkeys(const long long *__restrict__ grp, int64_t R, unsigned long long gmin,
                                                  unsigned long long *__restrict__ keys, uint32_t *__restrict__ idx) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
        keys[r] = (unsigned long long)grp[r] - gmin;
        idx[r] = (uint32_t)r;
    }
}

__global__ void __launch_bounds__(256) k_lf_starts(const unsigned long long *__restrict__ keys, int64_t R,
                                                   uint32_t *__restrict__ st) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= R; i += (int64_t)gridDim.x * blockDim.x)
        st[i] = i < R && i > 0 && keys[i] != keys[i - 1];       // st[R] = 0: the scan's total is the last rank
}

__global__ void __launch_bounds__(256) k_lf_scatter(const uint32_t *__restrict__ rank, const uint32_t *__restrict__ idx,
                                                    int64_t R, uint32_t *__restrict__ slot) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < R; i += (int64_t)gridDim.x * blockDim.x)
        slot[idx[i]] = rank[i];
}

// ---------------------------------------------------------------------------
// 4. Pass A over the R * n pairs, L lanes per read as in k_lf_reads (no
// division: the bit is key - group * n). Lanes of a wave that hit one counter
// are combined into one atomicAdd (reads of one group follow each other
// closely in a history: same-address atomics serialise in L2).
__global__ void __launch_bounds__(256) k_lf_count(const int64_t *__restrict__ aux, const int64_t *__restrict__ start,
                                                  const long long *__restrict__ grp, const uint32_t *__restrict__ slot,
                                                  int64_t R, long long n, int logL, unsigned *__restrict__ cnt,
                                                  long long *__restrict__ val, LMeta *m) {
    const int lane = threadIdx.x & 63;
    const int L = 1 << logL;
    const int steps = (int)((n + L - 1) >> logL);
    const bool vec = ((uintptr_t)aux & 15) == 0;
    const int64_t total = R << logL;
    for (int64_t t0 = blockIdx.x * 256LL; t0 < total; t0 += (int64_t)gridDim.x * 256) {   // block-uniform
        const int64_t t = t0 + threadIdx.x, r = t >> logL;
        const int sub = (int)(t & (L - 1));
        const bool have = r < R;
        const int64_t q0 = have ? start[r] : 0;
        const unsigned long long gbase = have ? (unsigned long long)grp[r] * (unsigned long long)n : 0;
        const unsigned long long sbase = have ? (unsigned long long)slot[r] * (unsigned long long)n : 0;
        for (int s = 0; s < steps; s++) {                     // wave-uniform
            const long long j = sub + ((long long)s << logL);
            bool live = have && j < n;
            unsigned long long idx = NONE;
            long long v = JH_NIL;
            if (live) {
                const int64_t q = q0 + j;
                const longlong2 kv = vec ? ((const longlong2 *)aux)[q] : make_longlong2(aux[2 * q], aux[2 * q + 1]);
                v = kv.y;
                live = v != JH_NIL;
                idx = sbase + ((unsigned long long)kv.x - gbase);
            }
            unsigned long long todo = __ballot(live);
            while (todo) {                                    // wave-uniform: one round per distinct counter
                const int leader = __ffsll((long long)todo) - 1;
                const unsigned long long li = __shfl(idx, leader);
                const unsigned long long peers = __ballot(live && idx == li);
                if (lane == leader) atomicAdd(&cnt[li], (unsigned)__popcll(peers));
                todo &= ~peers;
            }
            if (live) {
                long long old = __atomic_load_n(&val[idx], __ATOMIC_RELAXED);
                if (old == JH_NIL)
                    old = (long long)atomicCAS((unsigned long long *)&val[idx], (unsigned long long)JH_NIL, (unsigned long long)v);
                if (old != JH_NIL && old != v) { atomicOr(&cnt[idx], CONFLICT); m->conflict = 1; }
            }
        }
    }
}

// the smallest row of a read that holds a value for a key with two distinct values
__global__ void __launch_bounds__(256) k_lf_conflict_row(const int64_t *__restrict__ aux, const int64_t *__restrict__ row,
                                                         const int64_t *__restrict__ start,
                                                         const uint32_t *__restrict__ slot, int64_t R, long long n,
                                                         const unsigned *__restrict__ cnt, LMeta *m) {
    __shared__ unsigned long long sh[4];
    unsigned long long best = NONE;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
        for (long long j = 0; j < n; j++) {
            const int64_t q = start[r] + j;
            if (aux[2 * q + 1] == JH_NIL) continue;
            long long g;
            int bit;
            floor_divmod(aux[2 * q], n, g, bit);
            if (cnt[(unsigned long long)slot[r] * (unsigned long long)n + bit] & CONFLICT)
                best = min(best, (unsigned long long)row[r]);
        }
    }
    best = block_reduce256(best, RedMin(), sh);
    if (threadIdx.x == 0 && best != NONE) atomicMin(&m->ill2_row, best);
}

// Pass B. The masks of a group form a chain under inclusion exactly when no
// read has min(cnt over its set bits) <= max(cnt over its clear bits).
__global__ void __launch_bounds__(256) k_lf_test(const unsigned long long *__restrict__ mask,
                                                 const uint32_t *__restrict__ slot, int64_t R, int n,
                                                 const unsigned *__restrict__ cnt, unsigned *__restrict__ gbits,
                                                 LMeta *m) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long mk = mask[r];
        const uint32_t s = slot[r];
        const unsigned *c = cnt + (unsigned long long)s * (unsigned long long)n;
        long long lo = LLONG_MAX, hi = -1;
        for (int b = 0; b < n; b++) {
            const long long x = c[b];
            if ((mk >> b) & 1) lo = min(lo, x);
            else hi = max(hi, x);
        }
        if (lo <= hi) {
            const unsigned bit = 1u << (s & 31);
            const unsigned old = atomicOr(&gbits[s >> 5], bit);
            if (!(old & bit)) atomicAdd(&m->fork_groups, 1ULL);
            m->any_fail = 1;
        }
    }
}

// ---------------------------------------------------------------------------
// 5. listing
__global__ void __launch_bounds__(256) k_lf_suspect(const uint32_t *__restrict__ slot, int64_t R,
                                                    const unsigned *__restrict__ gbits, uint8_t *__restrict__ flag) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t s = slot[r];
        flag[r] = (gbits[s >> 5] >> (s & 31)) & 1;
    }
}

__global__ void __launch_bounds__(256) k_lf_suskeys(const uint32_t *__restrict__ sus, int64_t S,
                                                    const uint32_t *__restrict__ slot, uint32_t *__restrict__ skey) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < S; i += (int64_t)gridDim.x * blockDim.x)
        skey[i] = slot[sus[i]];
}

__global__ void __launch_bounds__(256) k_lf_gather(const uint32_t *__restrict__ sus, int64_t S,
                                                   const unsigned long long *__restrict__ mask,
                                                   const int64_t *__restrict__ row, unsigned long long *__restrict__ smask,
                                                   int64_t *__restrict__ srow) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < S; i += (int64_t)gridDim.x * blockDim.x) {
        smask[i] = mask[sus[i]];
        srow[i] = row[sus[i]];
    }
}

// One wave per suspect i; its lanes stride over the later suspects of i's
// group (contiguous after the sort). WRITE = 0: pc[i] = the number of
// incomparable partners. WRITE = 1: the pairs, from off[i] on, below cap.
template <int WRITE>
__global__ void __launch_bounds__(256) k_lf_pairs(const uint32_t *__restrict__ skey,
                                                  const unsigned long long *__restrict__ smask,
                                                  const int64_t *__restrict__ srow, int64_t S,
                                                  long long *__restrict__ pc, const long long *__restrict__ off,
                                                  int64_t cap, int64_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = (1ULL << lane) - 1;
    const int64_t nw = (int64_t)gridDim.x * 4;
    for (int64_t i = blockIdx.x * 4LL + (threadIdx.x >> 6); i < S; i += nw) {
        const long long base = WRITE ? off[i] : 0;
        if (WRITE && base >= cap) continue;                   // wave-uniform
        const uint32_t s = skey[i];
        const unsigned long long ma = smask[i];
        const int64_t ra = WRITE ? srow[i] : 0;
        long long total = 0;
        for (int64_t j0 = i + 1; j0 < S; j0 += 64) {
            const int64_t j = j0 + lane;
            const bool in = j < S && skey[j] == s;
            unsigned long long mb = ma;
            if (in) mb = smask[j];
            const bool inc = (ma & ~mb) != 0 && (mb & ~ma) != 0;
            const unsigned long long bal = __ballot(inc);
            if (WRITE && inc) {
                const long long p = base + total + __popcll(bal & lt);
                if (p < cap) { out[2 * p] = ra; out[2 * p + 1] = srow[j]; }
            }
            total += __popcll(bal);
            if (!(__ballot(in) >> 63)) break;                 // the group ends inside this step
        }
        if (!WRITE && lane == 0) pc[i] = total;
    }
}

int bits_of(unsigned long long x) {
    int b = 1;
    while (b < 64 && (x >> b)) b++;
    return b;
}

}  // namespace

void long_fork_check(jh_ctx *ctx, const jh_history *dh, const jh_long_fork_opts *opts, jh_long_fork_result *res,
                     int64_t *forks_out, int64_t fork_cap, hipStream_t st) {
    memset(res, 0, sizeof *res);
    res->valid = JH_VALID;
    res->multiple_key = JH_NIL;
    res->multiple_row = -1;
    res->illegal_row = -1;
    const int64_t n = dh->n;
    const long long gn = opts->n;
    if (dh->n_aux < 0 || (dh->n_aux & 1)) throw_jh(JH_EINVAL, "long-fork: n_aux must be even and >= 0 (pairs)");
    if (n == 0) return;
    if (n > 0x7fffffff00LL) throw_jh(JH_EUNSUPPORTED, "long-fork: more than 2^39 rows");
    DeviceTimer timer{ctx, st};
    timer.start();
    const int64_t half = dh->n_aux / 2;
    int logL = 0;
    while (logL < 4 && (2LL << logL) <= gn) logL++;               // L = 1, 2, 4, 8, 16 lanes per read: L <= n (< 2 L up to 16)

    // 1. the reads and the writes, in history order
    LMeta *m = ctx->ws<LMeta>(WS_LF_META, 1);
    k_lf_meta_init<<<1, 1, 0, st>>>(m);
    const int vec = (((uintptr_t)dh->type | (uintptr_t)dh->f | (uintptr_t)dh->value | (uintptr_t)dh->value2) & 15) == 0;
    const RowSel<2> sel = select_rows<2>(
        ctx, {WS_LF_WORDS, WS_LF_TCNT, WS_LF_TBASE, WS_LF_TMP}, n, 2 * RS_TILE, RS_WORDS,
        [&](int g, unsigned long long *words, long long *tile_cnt) {
            k_lf_flag<<<g, 256, 0, st>>>(dh->type, dh->f, n, vec, words, tile_cnt);
        }, st);
    const int g = sel.grid;
    const long long R = sel.count[0], W = sel.count[1];
    res->reads_count = R;
    if (R > L_MAX_COUNT) throw_jh(JH_EUNSUPPORTED, "long-fork: more than 2^31 - 2 reads");
    if (W > L_MAX_COUNT) throw_jh(JH_EUNSUPPORTED, "long-fork: more than 2^31 - 2 write invocations");
    if (R > 0 && half > 0 && !dh->aux) throw_jh(JH_EINVAL, "long-fork: n_aux > 0 without aux");

    int64_t *row = nullptr, *start = nullptr, *cnt = nullptr;
    long long *grp = nullptr;
    unsigned long long *mask = nullptr;
    if (R > 0) {
        row = ctx->ws<int64_t>(WS_LF_ROW, R);
        start = ctx->ws<int64_t>(WS_LF_START, R);
        cnt = ctx->ws<int64_t>(WS_LF_CNT, R);
        grp = ctx->ws<long long>(WS_LF_GRP, R);
        mask = ctx->ws<unsigned long long>(WS_LF_MASK, R);
        k_lf_compact<0><<<g, 256, 0, st>>>(dh->value, dh->value2, n, vec, sel.words[0], sel.base[0], half, row, start, cnt, m);
        // a bad range was replaced by an empty one: the pass below stays inside aux
        k_lf_reads<<<grid_for(R << logL, 256, 4096), 256, 0, st>>>(dh->aux, row, start, cnt, R, gn, logL, grp, mask, m);
    }
    int64_t *wkey = nullptr, *wrow = nullptr;
    if (W > 0) {
        wkey = ctx->ws<int64_t>(WS_LF_WKEY, W);
        wrow = ctx->ws<int64_t>(WS_LF_WROW, W);
        k_lf_compact<1><<<g, 256, 0, st>>>(dh->value, dh->value2, n, vec, sel.words[1], sel.base[1], half, wkey, wrow, nullptr, m);
    }
    LMeta mh = fetch(m, st);
    if (mh.bad_range) throw_jh(JH_EINVAL, "long-fork: a read's pair range leaves [0, n_aux / 2) or has a negative count");
    if (mh.unsup)
        throw_jh(JH_EUNSUPPORTED, "long-fork: a read of n keys that are not one aligned group, or that names a key twice");
    res->early_count = (int64_t)mh.reads_early;
    res->late_count = (int64_t)mh.reads_late;
    res->entries = (int64_t)mh.entries;
    int path = opts->path;

    // 2. multiple writes
    if (W > 1) {
        const unsigned long long kmin = mh.kmin ^ SIGN, width = mh.kmax - mh.kmin;   // span - 1: cannot wrap
        int p2 = path;
        if (p2 == 0) p2 = width < 4ULL * (unsigned long long)W + 1024 && width < DENSE_MAX ? 1 : 2;
        if (p2 == 1 && width >= DENSE_MAX) throw_jh(JH_EINVAL, "long-fork dense path: the written keys span more than 2^28 values");
        if (p2 == 1) {
            unsigned long long *first = ctx->ws<unsigned long long>(WS_LF_FIRST, width + 1);
            k_lf_fill<<<grid_for((int64_t)width + 1, 256, 2048), 256, 0, st>>>(first, (int64_t)width + 1, NONE);
            k_lf_first<<<grid_for(W, 256, 2048), 256, 0, st>>>(wkey, wrow, W, kmin, first);
            k_lf_repeat<<<grid_for(W, 256, 2048), 256, 0, st>>>(wkey, wrow, W, kmin, first, m);
        } else {
            unsigned long long *keys = ctx->ws<unsigned long long>(WS_LF_KEYS, 2 * W);
            uint32_t *idx = ctx->ws<uint32_t>(WS_LF_IDX, 2 * W);
            k_lf_wkeys<<<grid_for(W, 256, 2048), 256, 0, st>>>(wkey, W, kmin, keys, idx);
            hipcub::DoubleBuffer<unsigned long long> kb(keys, keys + W);
            hipcub::DoubleBuffer<uint32_t> vb(idx, idx + W);
            sort_pairs(ctx, WS_LF_TMP, kb, vb, (int)W, bits_of(width), st);
            k_lf_repeat_sorted<<<grid_for(W, 256, 2048), 256, 0, st>>>(kb.Current(), vb.Current(), wrow, W, m);
        }
        mh = fetch(m, st);
        if (mh.mw_row != NONE) {
            res->valid = JH_UNKNOWN;
            res->cause = JH_CAUSE_MULTIPLE_WRITES;
            res->multiple_row = (int64_t)mh.mw_row;
            HIP_TRY(hipMemcpyAsync(&res->multiple_key, dh->value + mh.mw_row, sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            res->device_ms = timer.stop();
            return;
        }
    }
    if (R == 0) { res->device_ms = timer.stop(); return; }
    if (mh.ill1_row != NONE) {
        res->valid = JH_UNKNOWN;
        res->cause = JH_CAUSE_ILLEGAL_HISTORY;
        res->illegal_kind = 1;
        res->illegal_row = (int64_t)mh.ill1_row;
        res->device_ms = timer.stop();
        return;
    }

    // 3. group slots: every read has n pairs from here on
    const unsigned long long gmin = mh.gmin ^ SIGN, gwidth = mh.gmax - mh.gmin;
    const unsigned long long E = (unsigned long long)R * (unsigned long long)gn;
    // dense tables hold (gwidth + 1) * n counters and values: at most 4 per pair entry in auto mode
    const bool dense_fits = gwidth < DENSE_MAX && (gwidth + 1) * (unsigned long long)gn <= DENSE_MAX;
    if (path == 0) path = dense_fits && (gwidth + 1) * (unsigned long long)gn <= 4 * E + 1024 ? 1 : 2;
    if (path == 1 && !dense_fits) throw_jh(JH_EINVAL, "long-fork dense path: the groups span more than 2^28 table entries");
    res->path = path;
    uint32_t *slot = ctx->ws<uint32_t>(WS_LF_SLOT, R);
    const int gr = grid_for(R, 256, 2048);
    unsigned long long G;
    if (path == 1) {
        k_lf_slot_dense<<<gr, 256, 0, st>>>(grp, R, gmin, slot);
        G = gwidth + 1;
    } else {
        unsigned long long *keys = ctx->ws<unsigned long long>(WS_LF_KEYS, 2 * R);
        uint32_t *idx = ctx->ws<uint32_t>(WS_LF_IDX, 2 * R);
        uint32_t *stf = ctx->ws<uint32_t>(WS_LF_RANK, 2 * (R + 1));
        uint32_t *rank = stf + R + 1;
        k_lf_gkeys<<<gr, 256, 0, st>>>(grp, R, gmin, keys, idx);
        hipcub::DoubleBuffer<unsigned long long> kb(keys, keys + R);
        hipcub::DoubleBuffer<uint32_t> vb(idx, idx + R);
        sort_pairs(ctx, WS_LF_TMP, kb, vb, (int)R, bits_of(gwidth), st);
        k_lf_starts<<<grid_for(R + 1, 256, 2048), 256, 0, st>>>(kb.Current(), R, stf);
        excl_sum(ctx, WS_LF_TMP, as_input(stf), rank, (int)(R + 1), st);
        // the exclusive sum at i + 1 is the inclusive rank of i; at R it is the last rank
        k_lf_scatter<<<gr, 256, 0, st>>>(rank + 1, vb.Current(), R, slot);
        G = (unsigned long long)fetch(rank + R, st) + 1;
    }

    // 4. the chain test
    const unsigned long long T = G * (unsigned long long)gn;
    unsigned *ctab = ctx->ws<unsigned>(WS_LF_CTAB, T);
    long long *vtab = ctx->ws<long long>(WS_LF_VTAB, T);
    const int64_t gw = (int64_t)((G + 31) / 32);
    unsigned *gbits = ctx->ws<unsigned>(WS_LF_GBITS, gw);
    HIP_TRY(hipMemsetAsync(ctab, 0, sizeof(unsigned) * T, st));
    HIP_TRY(hipMemsetAsync(gbits, 0, sizeof(unsigned) * gw, st));
    k_lf_fill<<<grid_for((int64_t)T, 256, 2048), 256, 0, st>>>((unsigned long long *)vtab, (int64_t)T, (unsigned long long)JH_NIL);
    k_lf_count<<<grid_for(R << logL, 256, 4096), 256, 0, st>>>(dh->aux, start, grp, slot, R, gn, logL, ctab, vtab, m);
    mh = fetch(m, st);
    if (mh.conflict) {
        k_lf_conflict_row<<<gr, 256, 0, st>>>(dh->aux, row, start, slot, R, gn, ctab, m);
        mh = fetch(m, st);
        res->valid = JH_UNKNOWN;
        res->cause = JH_CAUSE_ILLEGAL_HISTORY;
        res->illegal_kind = 2;
        res->illegal_row = (int64_t)mh.ill2_row;
        res->device_ms = timer.stop();
        return;
    }
    k_lf_test<<<gr, 256, 0, st>>>(mask, slot, R, (int)gn, ctab, gbits, m);
    mh = fetch(m, st);
    if (!mh.any_fail) { res->device_ms = timer.stop(); return; }

    // 5. the forks of the flagged groups
    res->valid = JH_INVALID;
    res->fork_groups = (int64_t)mh.fork_groups;
    uint8_t *flag = ctx->ws<uint8_t>(WS_LF_FLAG, R);
    uint32_t *sus = ctx->ws<uint32_t>(WS_LF_IDX, 2 * R);
    k_lf_suspect<<<gr, 256, 0, st>>>(slot, R, gbits, flag);
    select_flagged(ctx, WS_LF_TMP, hipcub::CountingInputIterator<uint32_t>(0), flag, sus, &m->n_sel, (int)R, st);
    mh = fetch(m, st);
    const int64_t S = mh.n_sel;
    uint32_t *skey = ctx->ws<uint32_t>(WS_LF_SKEY, 2 * S);
    const int gsu = grid_for(S, 256, 2048);
    k_lf_suskeys<<<gsu, 256, 0, st>>>(sus, S, slot, skey);
    hipcub::DoubleBuffer<uint32_t> kb(skey, skey + S), vb(sus, sus + R);
    sort_pairs(ctx, WS_LF_TMP, kb, vb, (int)S, bits_of(G), st);
    unsigned long long *smask = ctx->ws<unsigned long long>(WS_LF_SMASK, S);
    int64_t *srow = ctx->ws<int64_t>(WS_LF_SROW, S);
    long long *pc = ctx->ws<long long>(WS_LF_PC, 2 * (S + 1));
    long long *off = pc + S + 1;
    k_lf_gather<<<gsu, 256, 0, st>>>(vb.Current(), S, mask, row, smask, srow);
    HIP_TRY(hipMemsetAsync(pc + S, 0, sizeof(long long), st));
    const int gp = grid_for(S, 4, 8192);
    k_lf_pairs<0><<<gp, 256, 0, st>>>(kb.Current(), smask, srow, S, pc, nullptr, 0, nullptr);
    excl_sum(ctx, WS_LF_TMP, as_input(pc), off, (int)(S + 1), st);
    const long long total = fetch(off + S, st);
    res->fork_count = total;
    const int64_t k = forks_out ? std::min<int64_t>(total, fork_cap) : 0;
    if (k > 0) {
        int64_t *out = ctx->ws<int64_t>(WS_LF_OUT, 2 * k);
        k_lf_pairs<1><<<gp, 256, 0, st>>>(kb.Current(), smask, srow, S, nullptr, off, k, out);
        HIP_TRY(hipMemcpyAsync(forks_out, out, sizeof(int64_t) * 2 * k, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    res->device_ms = timer.stop();
}
