// jh_uids.hip -- checker/unique-ids on MI355X.
//
// unique-ids, jepsen/src/jepsen/checker.clj:631-676, over the whole history:
//   attempted = :invoke :generate rows, acks = the :value of every :ok
//   :generate row (nil is an id like any other), dups = ids acknowledged more
//   than once with their number of occurrences, range = [lowest highest]
//   under compare (nil below everything).
//
// Pipeline:
//   1. k_uid_scan      one streaming pass over type / f / value (24 B/row, row
//                      pairs in 16-byte loads): attempted, nil acks, min / max
//                      of the non-nil acked ids, and the non-nil acked ids
//                      compacted into a dense list (row order inside a tile;
//                      one counter atomic per 4096-row tile)
//      k_uid_scan_fin  block partials -> meta; one host readback
//   2. dense path      (span <= 64 ids per ack) k_uid_mark: bit id - lo of a
//                      zeroed bitmap with a returning atomicOr; an occurrence
//                      whose bit was already set goes to `extra`. A valid
//                      history leaves extra empty and the call ends there.
//      sorted path     hipcub radix sort of the keys id - lo
//   3. k_uid_runs      neighbour tests on the sorted keys (the sorted list, or
//                      the sorted extra): run starts / ends, compacted in
//                      order; their count is duplicated-count
//   4. selection       everything when it fits dup_cap, else a stable radix
//                      sort by count of the list ascending by id, the last
//                      dup_cap entries, emitted in ascending id -- the
//                      reference's (sort-by val) / reverse / (take 48)
// nil is never marked or sorted: it is a duplicated id with count nil_count
// when nil_count >= 2, and takes part in the selection as the smallest id.
#include "jh_prims.h"

namespace {
constexpr int U_PAIRS = 8;                  // row pairs per thread per tile
constexpr int U_TILE = 256 * U_PAIRS;       // row pairs per tile (4096 rows)

struct UMeta {
    long long lo, hi;                   // non-nil acked ids
    long long attempted, nil_count;
    unsigned long long n_list;          // non-nil acks (the compacted list)
    unsigned long long n_extra;         // dense path: duplicate occurrences
    unsigned long long n_runs;          // duplicated non-nil ids
    int n_sel[2];                       // DeviceSelect counts (starts, ends)
};

// One tile = 256 threads x U_PAIRS row pairs, pair p0 + u * 256 + thread, so
// every wave-instruction loads 1 KiB. The tile's non-nil acked ids go to the
// list in row order: per (u, wave) two ballots give each lane its position,
// the 32 (u, wave) counts are scanned by wave 0, and one atomic per tile
// reserves the range (a per-wave atomic on the one counter would bound the
// pass: a single word takes about 88 returning atomics per microsecond).
__global__ void __launch_bounds__(256) k_uid_scan(const int64_t *__restrict__ type, const int64_t *__restrict__ f,
                                                  const int64_t *__restrict__ value, int64_t n, int64_t fgen,
                                                  int vec, int64_t *__restrict__ list, UMeta *m, long long *parts) {
    __shared__ unsigned sh_cnt[U_PAIRS * 4];
    __shared__ unsigned long long sh_base;
    __shared__ long long sh[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt = (1ULL << lane) - 1;
    const int64_t np = (n + 1) / 2, n_tiles = (np + U_TILE - 1) / U_TILE;
    long long lo = LLONG_MAX, hi = LLONG_MIN, att = 0, nil = 0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t p0 = tile * U_TILE + threadIdx.x;
        longlong2 t2[U_PAIRS], f2[U_PAIRS], v2[U_PAIRS];
#pragma unroll
        for (int u = 0; u < U_PAIRS; u++) {
            const int64_t p = p0 + u * 256;
            if (p < np) {
                t2[u] = ld_pair(type, p, n, vec); f2[u] = ld_pair(f, p, n, vec); v2[u] = ld_pair(value, p, n, vec);
            } else {
                t2[u] = make_longlong2(-1, -1); f2[u] = t2[u]; v2[u] = t2[u];
            }
        }
        unsigned ack = 0, pos[U_PAIRS];
#pragma unroll
        for (int u = 0; u < U_PAIRS; u++) {
            const int64_t p = p0 + u * 256;
            const bool g0 = p < np && f2[u].x == fgen, g1 = 2 * p + 1 < n && f2[u].y == fgen;
            att += (g0 && t2[u].x == T_INVOKE) + (g1 && t2[u].y == T_INVOKE);
            const bool k0 = g0 && t2[u].x == T_OK, k1 = g1 && t2[u].y == T_OK;
            const bool a0 = k0 && v2[u].x != JH_NIL, a1 = k1 && v2[u].y != JH_NIL;
            nil += (k0 && !a0) + (k1 && !a1);
            if (a0) { lo = min(lo, (long long)v2[u].x); hi = max(hi, (long long)v2[u].x); }
            if (a1) { lo = min(lo, (long long)v2[u].y); hi = max(hi, (long long)v2[u].y); }
            const unsigned long long b0 = __ballot(a0), b1 = __ballot(a1);
            pos[u] = __popcll(b0 & lt) + __popcll(b1 & lt);
            ack |= ((unsigned)a0 << (2 * u)) | ((unsigned)a1 << (2 * u + 1));
            if (lane == 0) sh_cnt[u * 4 + wave] = __popcll(b0) + __popcll(b1);
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const unsigned c = lane < U_PAIRS * 4 ? sh_cnt[lane] : 0;
            unsigned inc = c;
#pragma unroll
            for (int d = 1; d < U_PAIRS * 4; d <<= 1) {
                const unsigned o = __shfl_up(inc, d);
                if (lane >= d) inc += o;
            }
            if (lane < U_PAIRS * 4) sh_cnt[lane] = inc - c;
            if (lane == U_PAIRS * 4 - 1) sh_base = inc ? atomicAdd(&m->n_list, (unsigned long long)inc) : 0ULL;
        }
        __syncthreads();
        const unsigned long long base = sh_base;
#pragma unroll
        for (int u = 0; u < U_PAIRS; u++) {
            unsigned long long w = base + sh_cnt[u * 4 + wave] + pos[u];
            if ((ack >> (2 * u)) & 1) list[w++] = v2[u].x;
            if ((ack >> (2 * u + 1)) & 1) list[w] = v2[u].y;
        }
        __syncthreads();                                  // sh_cnt / sh_base are reused by the next tile
    }
    lo = block_reduce256(lo, RedMin(), sh);
    hi = block_reduce256(hi, RedMax(), sh);
    att = block_reduce256(att, RedSum(), sh);
    nil = block_reduce256(nil, RedSum(), sh);
    if (threadIdx.x == 0) {
        long long *pp = parts + 4 * blockIdx.x;
        pp[0] = lo; pp[1] = hi; pp[2] = att; pp[3] = nil;
    }
}

__global__ void __launch_bounds__(256) k_uid_scan_fin(const long long *__restrict__ parts, int np, UMeta *m) {
    long long lo = LLONG_MAX, hi = LLONG_MIN, att = 0, nil = 0;
    for (int i = threadIdx.x; i < np; i += 256) {
        const long long *pp = parts + 4 * i;
        lo = min(lo, pp[0]); hi = max(hi, pp[1]); att += pp[2]; nil += pp[3];
    }
    __shared__ long long sh[4];
    lo = block_reduce256(lo, RedMin(), sh);
    hi = block_reduce256(hi, RedMax(), sh);
    att = block_reduce256(att, RedSum(), sh);
    nil = block_reduce256(nil, RedSum(), sh);
    if (threadIdx.x == 0) { m->lo = lo; m->hi = hi; m->attempted = att; m->nil_count = nil; }
}

// Dense path. Lanes of a wave that fall into one bitmap word are combined
// into one returning atomicOr (consecutive ids: one or two words per wave
// instead of 64 same-address atomics, which serialise in L2). Two lanes of
// one wave carrying the SAME bit have to be resolved before that: the OR
// holds the bit once, and the returned word says "clear" to both, so without
// this all but the first of them are counted here as duplicate occurrences
// by themselves -- `same` is the lanes with this lane's bit number (a 6-bit
// match from six ballots), `peers` the lanes in this lane's word.
// Duplicate occurrences are appended to `extra` (as keys id - lo) with one
// counter atomic per wave.
__global__ void __launch_bounds__(256) k_uid_mark(const int64_t *__restrict__ list, int64_t cnt, unsigned long long lo,
                                                  unsigned long long *__restrict__ bits,
                                                  unsigned long long *__restrict__ extra, UMeta *m) {
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = (1ULL << lane) - 1;
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    // the loop runs while any lane of the wave has an element: every lane
    // takes part in the ballots and shuffles
    for (int64_t w0 = i - lane; w0 < cnt; w0 += gs, i += gs) {
        const bool live = i < cnt;
        const unsigned long long off = live ? (unsigned long long)list[i] - lo : 0;
        const unsigned long long w = off >> 6;
        const unsigned b = (unsigned)(off & 63);
        unsigned long long same = ~0ULL;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const bool bj = (b >> j) & 1;
            const unsigned long long mj = __ballot(bj);
            same &= bj ? mj : ~mj;
        }
        unsigned long long todo = __ballot(live);
        bool dup = false;
        while (todo) {                                    // wave-uniform: one round per distinct word
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned long long lw = __shfl(w, leader);
            const bool mine = live && w == lw;
            const unsigned long long peers = __ballot(mine);
            unsigned long long comb = mine ? 1ULL << b : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) comb |= __shfl_xor(comb, o);
            unsigned long long old = 0;
            if (lane == leader) old = atomicOr(&bits[lw], comb);
            old = __shfl(old, leader);
            if (mine) dup = ((old >> b) & 1) || (same & peers & lt) != 0;
            todo &= ~peers;
        }
        const unsigned long long dm = __ballot(dup);
        if (dm) {
            const int ldr = __ffsll((long long)dm) - 1;
            unsigned long long base = 0;
            if (lane == ldr) base = atomicAdd(&m->n_extra, (unsigned long long)__popcll(dm));
            base = __shfl(base, ldr);
            if (dup) extra[base + __popcll(dm & lt)] = off;
        }
    }
}

// sorted path: the order-preserving keys id - lo, in place
__global__ void __launch_bounds__(256) k_uid_keys(unsigned long long *__restrict__ list, int64_t cnt, unsigned long long lo) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x)
        list[i] -= lo;
}

// Runs of equal keys in a sorted list, by neighbour tests only (a run may span
// any number of blocks). each = 0 (the sorted acks): a run of two or more is a
// duplicated id -- i starts one iff it differs from i-1 and equals i+1, and
// ends one iff it equals i-1 and differs from i+1. each = 1 (the sorted extra
// occurrences): every run is one, runs of length 1 included.
// flag bit 0: start, bit 1: end.
__global__ void __launch_bounds__(256) k_uid_runs(const unsigned long long *__restrict__ keys, int64_t cnt, int each,
                                                  uint8_t *__restrict__ flag, UMeta *m) {
    long long starts = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long k = keys[i];
        const bool eq_prev = i > 0 && keys[i - 1] == k;
        const bool eq_next = i + 1 < cnt && keys[i + 1] == k;
        const bool st = !eq_prev && (each || eq_next), en = !eq_next && (each || eq_prev);
        flag[i] = (uint8_t)(st | (en << 1));
        starts += st;
    }
    __shared__ long long sh[4];
    starts = block_reduce256(starts, RedSum(), sh);
    if (threadIdx.x == 0 && starts) atomicAdd(&m->n_runs, (unsigned long long)starts);
}

struct FlagBit {
    int bit;
    __host__ __device__ uint8_t operator()(uint8_t x) const { return (x >> bit) & 1; }
};

// (id, count) of every duplicated id in ascending id, nil first (has_nil):
// count = run length, + 1 when the runs are of extra occurrences
__global__ void __launch_bounds__(256) k_uid_pairs(const unsigned long long *__restrict__ keys,
                                                   const int64_t *__restrict__ st, const int64_t *__restrict__ en,
                                                   int64_t n_runs, unsigned long long lo, int each, int has_nil,
                                                   long long nil_count, int64_t *__restrict__ pairs,
                                                   unsigned long long *__restrict__ cnt, uint32_t *__restrict__ idx) {
    const int64_t D = n_runs + has_nil;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < D; j += (int64_t)gridDim.x * blockDim.x) {
        int64_t id, c;
        if (has_nil && j == 0) { id = JH_NIL; c = nil_count; }
        else {
            const int64_t r = j - has_nil;
            id = (int64_t)(keys[st[r]] + lo);
            c = en[r] - st[r] + 1 + each;
        }
        pairs[2 * j] = id; pairs[2 * j + 1] = c;
        cnt[j] = (unsigned long long)c;
        idx[j] = (uint32_t)j;
    }
}

__global__ void __launch_bounds__(256) k_uid_gather(const int64_t *__restrict__ pairs, const uint32_t *__restrict__ sel,
                                                    int64_t k, int64_t *__restrict__ out) {
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < k; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = sel[j];
        out[2 * j] = pairs[2 * s]; out[2 * j + 1] = pairs[2 * s + 1];
    }
}

int bits_of(unsigned long long x) {
    int b = 1;
    while (b < 64 && (x >> b)) b++;
    return b;
}

// sorts cnt keys; returns the sorted array (keys or alt)
unsigned long long *sorted_keys(jh_ctx *ctx, unsigned long long *keys, unsigned long long *alt, int64_t cnt, int end_bit,
                              hipStream_t st) {
    hipcub::DoubleBuffer<unsigned long long> db(keys, alt);
    sort_keys(ctx, WS_U_TMP, db, (int)cnt, end_bit, st);
    return db.Current();
}

}  // namespace

void unique_ids_check(jh_ctx *ctx, const jh_history *dh, const jh_unique_ids_opts *opts, jh_unique_ids_result *res,
                      int64_t *dup_out, int64_t dup_cap, hipStream_t st) {
    memset(res, 0, sizeof *res);
    res->valid = JH_VALID;
    res->range_lo = res->range_hi = JH_NIL;
    const int64_t n = dh->n;
    if (n == 0) return;
    DeviceTimer timer{ctx, st};
    timer.start();
    UMeta *m = ctx->ws<UMeta>(WS_U_META, 1);
    long long *parts = ctx->ws<long long>(WS_U_PART, 4 * 2048);
    int64_t *list = ctx->ws<int64_t>(WS_U_LIST, n);           // every row may be an ack
    HIP_TRY(hipMemsetAsync(m, 0, sizeof *m, st));
    const int vec = (((uintptr_t)dh->type | (uintptr_t)dh->f | (uintptr_t)dh->value) & 15) == 0;
    const int64_t n_tiles = ((n + 1) / 2 + U_TILE - 1) / U_TILE;
    const int g = grid_for(n_tiles, 1, 2048);
    k_uid_scan<<<g, 256, 0, st>>>(dh->type, dh->f, dh->value, n, opts->f_generate, vec, list, m, parts);
    k_uid_scan_fin<<<1, 256, 0, st>>>(parts, g, m);
    UMeta mh = fetch(m, st);
    const int64_t k = (int64_t)mh.n_list;
    const unsigned long long n_ack = mh.n_list + (unsigned long long)mh.nil_count;
    if (n_ack > 0x7fffffffULL) throw_jh(JH_EUNSUPPORTED, "more than 2^31 - 1 acknowledged ids");
    res->attempted_count = mh.attempted;
    res->acknowledged_count = (int64_t)n_ack;
    res->nil_count = mh.nil_count;
    const int has_nil = mh.nil_count >= 2;
    if (k > 0) { res->range_lo = mh.nil_count > 0 ? JH_NIL : mh.lo; res->range_hi = mh.hi; }
    if (n_ack == 0) { res->device_ms = timer.stop(); return; }

    const unsigned long long lo = (unsigned long long)mh.lo;
    const unsigned long long width = k > 0 ? (unsigned long long)mh.hi - lo : 0;   // span - 1: cannot wrap
    const unsigned long long DENSE_MAX = 1ULL << 35;
    int path = opts->path;
    if (path == 0) path = (width < 64ULL * n_ack && width < DENSE_MAX) ? 1 : 2;   // span <= 64 n_ack
    if (path == 1 && width >= DENSE_MAX) throw_jh(JH_EINVAL, "dense path: the ids span more than 2^35 values");
    res->path = path;

    const unsigned long long *sorted = nullptr;      // sorted keys the runs are taken from
    int64_t n_sorted = 0;
    int each = 0;
    if (k > 0 && path == 1) {
        const int64_t nw = (int64_t)(width / 64 + 1);
        unsigned long long *bits = ctx->ws<unsigned long long>(WS_U_BITS, nw);
        unsigned long long *extra = ctx->ws<unsigned long long>(WS_U_ALT, k);
        HIP_TRY(hipMemsetAsync(bits, 0, sizeof(unsigned long long) * nw, st));
        k_uid_mark<<<grid_for(k, 256, 2048), 256, 0, st>>>(list, k, lo, bits, extra, m);
        mh = fetch(m, st);
        n_sorted = (int64_t)mh.n_extra;
        each = 1;
        if (n_sorted > 0) {
            unsigned long long *alt = ctx->ws<unsigned long long>(WS_U_ALT2, n_sorted);
            sorted = sorted_keys(ctx, extra, alt, n_sorted, bits_of(width), st);
        }
    } else if (k > 0) {
        unsigned long long *keys = (unsigned long long *)list;
        unsigned long long *alt = ctx->ws<unsigned long long>(WS_U_ALT, k);
        k_uid_keys<<<grid_for(k, 256, 2048), 256, 0, st>>>(keys, k, lo);
        sorted = sorted_keys(ctx, keys, alt, k, bits_of(width), st);
        n_sorted = k;
    }

    int64_t n_runs = 0;
    uint8_t *flag = nullptr;
    if (n_sorted > 0) {
        flag = ctx->ws<uint8_t>(WS_U_FLAG, n_sorted);
        k_uid_runs<<<grid_for(n_sorted, 256, 2048), 256, 0, st>>>(sorted, n_sorted, each, flag, m);
        mh = fetch(m, st);
        n_runs = (int64_t)mh.n_runs;
    }
    const int64_t D = n_runs + has_nil;
    res->duplicated_count = D;
    res->valid = D == 0 ? JH_VALID : JH_INVALID;
    const int64_t out_k = std::min<int64_t>(D, dup_cap);
    if (out_k > 0 && dup_out) {
        int64_t *se = ctx->ws<int64_t>(WS_U_RUNS, 2 * n_runs + 2);
        int64_t *starts = se, *ends = se + n_runs + 1;
        if (n_runs > 0) {
            hipcub::CountingInputIterator<int64_t> rows(0);
            hipcub::TransformInputIterator<uint8_t, FlagBit, const uint8_t *> f0(flag, FlagBit{0}), f1(flag, FlagBit{1});
            // one scratch buffer of the larger size for both calls
            auto sel_starts = JH_CUB(DeviceSelect::Flagged, rows, f0, starts, m->n_sel, (int)n_sorted, st);
            auto sel_ends = JH_CUB(DeviceSelect::Flagged, rows, f1, ends, m->n_sel + 1, (int)n_sorted, st);
            size_t tb = std::max(cub_size(sel_starts), cub_size(sel_ends));
            char *tmp = ctx->ws<char>(WS_U_TMP, tb);
            HIP_TRY(sel_starts(tmp, tb));
            HIP_TRY(sel_ends(tmp, tb));
        }
        int64_t *pairs = ctx->ws<int64_t>(WS_U_PAIRS, 2 * D);
        unsigned long long *cnt = ctx->ws<unsigned long long>(WS_U_CNT, 2 * D);
        uint32_t *idx = ctx->ws<uint32_t>(WS_U_IDX, 2 * D);
        k_uid_pairs<<<grid_for(D, 256, 2048), 256, 0, st>>>(sorted, starts, ends, n_runs, lo, each, has_nil,
                                                            mh.nil_count, pairs, cnt, idx);
        const int64_t *src = pairs;
        if (D > out_k) {
            // stable by count over the list ascending by id, keep the tail:
            // the largest counts, ties towards the larger id; then back to
            // ascending id (the positions are the id order)
            unsigned long long max_c = (unsigned long long)std::max<long long>(mh.nil_count, 2);
            max_c = std::max<unsigned long long>(max_c, (unsigned long long)n_sorted + 1);
            // one scratch buffer of the larger size for both sorts
            auto by_count = JH_CUB(DeviceRadixSort::SortPairs, cnt, cnt + D, idx, idx + D, (int)D, 0, bits_of(max_c), st);
            size_t tb = cub_size(by_count);
            uint32_t *sel = ctx->ws<uint32_t>(WS_U_SEL, out_k);
            auto by_id = JH_CUB(DeviceRadixSort::SortKeys, idx + D + (D - out_k), sel, (int)out_k, 0,
                                bits_of((unsigned long long)D), st);
            tb = std::max(tb, cub_size(by_id));
            char *tmp = ctx->ws<char>(WS_U_TMP, tb);
            HIP_TRY(by_count(tmp, tb));
            HIP_TRY(by_id(tmp, tb));
            int64_t *out = ctx->ws<int64_t>(WS_U_OUT, 2 * out_k);
            k_uid_gather<<<grid_for(out_k, 256, 2048), 256, 0, st>>>(pairs, sel, out_k, out);
            src = out;
        }
        HIP_TRY(hipMemcpyAsync(dup_out, src, sizeof(int64_t) * 2 * out_k, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    res->device_ms = timer.stop();
}
