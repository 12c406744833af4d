// jh_perf.hip -- the reduction behind checker/perf's three plots on MI355X.
//
// (checker/latency-graph) and (checker/rate-graph), jepsen/src/jepsen/checker.clj:
// 736-768, over checker/perf.clj (point-graph!, quantiles-graph!, rate-graph!) and
// util.clj:606-640 (history->latencies). The reference hashes every op map into
// an index and then groups and sorts the history three times; all three plots
// come from four integer reductions over (process, type, f, time) (include/jh.h):
//   1. k_pf_scan     one pass over the rows: the limits (a nil or negative time,
//                    an f outside [0, f_count)), t_max and the range of process
//      k_pf_keys     (process - min process, row | invoke << 31)
//      one stable radix sort on the bits of the process range (skipped for one
//      process): the per-process order
//      k_pf_pair     one sorted slot per lane: the pairing from the slot before
//                    and after, pair[], the counts and the latency range
//   2. raw points:   k_pf_ptkey gives every row f * 3 + (the completion's place
//                    in :ok :info :fail), or one key past the last for a row that
//                    is no paired invoke; one stable radix sort on those few bits
//                    leaves the paired invokes first, in series order; a
//                    run-length pass gives the series counts
//   3. quantiles:    the invoke rows (DeviceSelect over a counting iterator, in
//                    row order), k_pf_latkey their latency less the smallest one,
//                    a stable sort by latency, k_pf_gkey f << b | bucket, a
//                    stable sort by that: (f, bucket, latency) order in two
//                    sorts, since the key does not fit 64 bits. Run lengths are
//                    the groups, k_pf_quant picks four entries per group.
//   4. rate:         k_pf_ratekey (f * 4 + type) << b | bucket per non-invoke
//                    client row, one key past the last otherwise; a key-only
//                    sort and a run-length pass are the cells (k_pf_cells)
// The sorts and scans are hipcub's over named scratch slots (jh_prims.h); the
// ballot compaction of row_select.h is not used here, DeviceSelect takes its
// place for the one ordered compaction (DESIGN.md §4n says what was not tried).
#include "jh_prims.h"

namespace {
constexpr int PF_STEPS = 4;                   // sorted slots per thread per tile of the pairing kernel
constexpr int PF_TILE = 256 * PF_STEPS;       // PERF_TILE in _abi.py: the tests straddle it
constexpr uint32_t INV_BIT = 0x80000000u, ROW_MASK = 0x7fffffffu;
constexpr unsigned long long SIGN = 0x8000000000000000ULL, NONE = ~0ULL;
constexpr long long PF_MAX_ROWS = 0x7ffffffeLL;
constexpr long long PF_MAX_F = 1LL << 20;

// signed values travel through the unsigned atomics with the sign bit flipped
struct PMeta {
    unsigned bad_time, bad_f;
    unsigned long long t_max;                 // times are >= 0 when nothing is bad
    unsigned long long p_min, p_max;          // process ^ SIGN
    unsigned long long n_inv, n_paired, n_unp, first_unp;
    unsigned long long lat_min, lat_max;      // latency ^ SIGN
};

__global__ void k_pf_meta_init(PMeta *m) {
    memset(m, 0, sizeof *m);
    m->p_min = NONE;
    m->first_unp = NONE;
    m->lat_min = NONE;
}

// the reference's two double divisions, then truncation (perf.clj:26-30 over
// util/nanos->secs); correctly rounded fp64, no reciprocal
__host__ __device__ __forceinline__ int64_t pf_bucket(int64_t t, int64_t dt) {
    return (int64_t)(((double)t / 1e9) / (double)dt);
}

// ---------------------------------------------------------------------------
// 1. the limits and the ranges
__global__ void __launch_bounds__(256) k_pf_scan(const int64_t *__restrict__ process, const int64_t *__restrict__ f,
                                                 const int64_t *__restrict__ time, int64_t n, int64_t f_count, PMeta *m) {
    __shared__ unsigned long long shr[4];
    unsigned long long tmax = 0, pmin = NONE, pmax = 0;
    unsigned bad_t = 0, bad_f = 0;
    for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = time[row], ff = f[row];
        const unsigned long long p = (unsigned long long)process[row] ^ SIGN;
        if (t < 0) bad_t = 1;                                 // JH_NIL is negative too
        else tmax = max(tmax, (unsigned long long)t);
        if (ff < 0 || ff >= f_count) bad_f = 1;
        pmin = min(pmin, p);
        pmax = max(pmax, p);
    }
    tmax = block_reduce256(tmax, RedMax(), shr);
    pmin = block_reduce256(pmin, RedMin(), shr);
    pmax = block_reduce256(pmax, RedMax(), shr);
    const unsigned long long bad = block_reduce256((unsigned long long)(bad_t | bad_f << 1), RedOr(), shr);
    if (threadIdx.x == 0) {
        atomicMax(&m->t_max, tmax);
        atomicMin(&m->p_min, pmin);
        atomicMax(&m->p_max, pmax);
        if (bad & 1) atomicOr(&m->bad_time, 1u);
        if (bad & 2) atomicOr(&m->bad_f, 1u);
    }
}

// key = the process less the smallest one: exact in unsigned arithmetic whatever
// 63-bit values the column holds
__global__ void __launch_bounds__(256) k_pf_keys(const int64_t *__restrict__ process, const int64_t *__restrict__ type,
                                                 int64_t n, unsigned long long p_min,
                                                 unsigned long long *__restrict__ key, uint32_t *__restrict__ val) {
    for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x) {
        key[row] = ((unsigned long long)process[row] ^ SIGN) - p_min;
        val[row] = (uint32_t)row | (type[row] == T_INVOKE ? INV_BIT : 0u);
    }
}

// The pairing. The reference keeps a map process -> pending invoke: an invoke
// does assoc! (a pending one of the same process is overwritten and stays
// unpaired), a completion that finds its process in the map takes that invoke and
// does dissoc!. So the map holds a process exactly when the last row of that
// process was an invoke, and the closed form over the per-process order is: a
// non-invoke row pairs with the slot before it iff that slot is an invoke of the
// same process; an invoke is paired iff the slot after it is a non-invoke of the
// same process. Every slot decides for its own row, so no write is shared.
// Slots i - 1 and i + 1 are read straight from the sorted arrays (i > 0 and
// i + 1 < n are checked); rows in val are < n by construction.
__global__ void __launch_bounds__(256) k_pf_pair(const unsigned long long *__restrict__ key,
                                                 const uint32_t *__restrict__ val, const int64_t *__restrict__ time,
                                                 int64_t n, int64_t *__restrict__ pair, PMeta *m) {
    __shared__ unsigned long long shr[4];
    unsigned long long n_inv = 0, n_paired = 0, n_unp = 0, first = NONE, lmin = NONE, lmax = 0;
    const int64_t n_tiles = (n + PF_TILE - 1) / PF_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
#pragma unroll
        for (int u = 0; u < PF_STEPS; u++) {
            const int64_t i = tile * PF_TILE + u * 256 + threadIdx.x;
            if (i >= n) continue;                             // nothing below is cross-lane
            const uint32_t v = val[i], r = v & ROW_MASK;
            const unsigned long long k = key[i];
            int64_t partner = -1;
            if (v & INV_BIT) {
                n_inv++;
                if (i + 1 < n && key[i + 1] == k) {
                    const uint32_t nv = val[i + 1];
                    if (!(nv & INV_BIT)) partner = nv & ROW_MASK;
                }
                if (partner < 0) { n_unp++; first = min(first, (unsigned long long)r); }
                else n_paired++;
            } else if (i > 0 && key[i - 1] == k) {
                const uint32_t pv = val[i - 1];
                if (pv & INV_BIT) {
                    partner = pv & ROW_MASK;
                    const unsigned long long lat = (unsigned long long)(time[r] - time[partner]) ^ SIGN;
                    lmin = min(lmin, lat);
                    lmax = max(lmax, lat);
                }
            }
            pair[r] = partner;
        }
    }
    n_inv = block_reduce256(n_inv, RedSum(), shr);
    n_paired = block_reduce256(n_paired, RedSum(), shr);
    n_unp = block_reduce256(n_unp, RedSum(), shr);
    first = block_reduce256(first, RedMin(), shr);
    lmin = block_reduce256(lmin, RedMin(), shr);
    lmax = block_reduce256(lmax, RedMax(), shr);
    if (threadIdx.x == 0) {
        if (n_inv) atomicAdd(&m->n_inv, n_inv);
        if (n_paired) atomicAdd(&m->n_paired, n_paired);
        if (n_unp) atomicAdd(&m->n_unp, n_unp);
        if (first != NONE) atomicMin(&m->first_unp, first);
        if (lmin != NONE) { atomicMin(&m->lat_min, lmin); atomicMax(&m->lat_max, lmax); }
    }
}

// ---------------------------------------------------------------------------
// 2. raw points. The place of a completion type in perf.clj:173-175's [:ok :info :fail]
__device__ __forceinline__ uint32_t pf_type_place(int64_t t) { return t == T_OK ? 0u : t == T_INFO ? 1u : 2u; }

__global__ void __launch_bounds__(256) k_pf_ptkey(const int64_t *__restrict__ type, const int64_t *__restrict__ f,
                                                  const int64_t *__restrict__ pair, int64_t n, uint32_t sentinel,
                                                  uint32_t *__restrict__ key, uint32_t *__restrict__ row_out) {
    for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = pair[row];
        uint32_t k = sentinel;
        if (p >= 0 && type[row] == T_INVOKE) k = (uint32_t)f[row] * 3u + pf_type_place(type[p]);   // f < f_count <= 2^20
        key[row] = k;
        row_out[row] = (uint32_t)row;
    }
}

__global__ void __launch_bounds__(256) k_pf_widen(const uint32_t *__restrict__ in, int64_t cnt, int64_t *__restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) out[i] = in[i];
}

// ---------------------------------------------------------------------------
// 3. quantile groups
struct IsInvoke {
    const int64_t *type;
    __host__ __device__ bool operator()(uint32_t row) const { return type[row] == T_INVOKE; }
};

// every invoke is paired here (n_unpaired_invokes == 0), so pair[row] is a row
__global__ void __launch_bounds__(256) k_pf_latkey(const uint32_t *__restrict__ rows, const int64_t *__restrict__ pair,
                                                   const int64_t *__restrict__ time, int64_t cnt, unsigned long long lat_min,
                                                   unsigned long long *__restrict__ key) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t r = rows[i];
        key[i] = ((unsigned long long)(time[pair[r]] - time[r]) ^ SIGN) - lat_min;
    }
}

__global__ void __launch_bounds__(256) k_pf_gkey(const uint32_t *__restrict__ rows, const int64_t *__restrict__ f,
                                                 const int64_t *__restrict__ time, int64_t cnt, int64_t dt, int bbits,
                                                 unsigned long long *__restrict__ key) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t r = rows[i];
        key[i] = (unsigned long long)f[r] << bbits | (unsigned long long)pf_bucket(time[r], dt);
    }
}

// One group per thread: its records lie at lat[start .. start + count), sorted.
// (Math/floor (* n q)) is one rounded fp64 multiply (perf.clj:58).
__global__ void __launch_bounds__(256) k_pf_quant(const unsigned long long *__restrict__ uniq, const int *__restrict__ cnt,
                                                  const int *__restrict__ start, const unsigned long long *__restrict__ lat,
                                                  unsigned long long lat_min, int bbits, int64_t n_groups,
                                                  int64_t *__restrict__ out) {
    const double qs[4] = {0.5, 0.95, 0.99, 1.0};
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long k = uniq[g];
        const int64_t c = cnt[g], s = start[g];
        int64_t *o = out + 7 * g;
        o[0] = (int64_t)(k >> bbits);
        o[1] = (int64_t)(k & ((1ULL << bbits) - 1));
        o[2] = c;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t fl = (int64_t)floor((double)c * qs[j]), idx = fl < c - 1 ? fl : c - 1;
            o[3 + j] = (int64_t)((lat[s + idx] + lat_min) ^ SIGN);
        }
    }
}

// ---------------------------------------------------------------------------
// 4. rate cells
__global__ void __launch_bounds__(256) k_pf_ratekey(const int64_t *__restrict__ process, const int64_t *__restrict__ type,
                                                    const int64_t *__restrict__ f, const int64_t *__restrict__ time,
                                                    int64_t n, int64_t dt, int bbits, unsigned long long sentinel,
                                                    unsigned long long *__restrict__ key) {
    for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = type[row];
        unsigned long long k = sentinel;
        if (t != T_INVOKE && process[row] >= 0)
            k = ((unsigned long long)f[row] * 4 + (unsigned long long)(t & 3)) << bbits | (unsigned long long)pf_bucket(time[row], dt);
        key[row] = k;
    }
}

__global__ void __launch_bounds__(256) k_pf_cells(const unsigned long long *__restrict__ uniq, const int *__restrict__ cnt,
                                                  int bbits, int64_t n_cells, int64_t *__restrict__ out) {
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < n_cells; g += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long k = uniq[g], ft = k >> bbits;
        int64_t *o = out + 4 * g;
        o[0] = (int64_t)(ft >> 2);
        o[1] = (int64_t)(ft & 3);
        o[2] = (int64_t)(k & ((1ULL << bbits) - 1));
        o[3] = cnt[g];
    }
}

int pf_bits(unsigned long long x) {
    int b = 1;
    while (b < 64 && (x >> b)) b++;
    return b;
}

template <class K>
void pf_rle(jh_ctx *ctx, const K *in, K *uniq, int *cnt, int *n_runs, int n, hipStream_t st) {
    cub_run(ctx, WS_PF_TMP, JH_CUB(DeviceRunLengthEncode::Encode, in, uniq, cnt, n_runs, n, st));
}

// the first min(count, cap) records of `width` words, device to host
void pf_copy_out(int64_t *dst, const int64_t *src_dev, int64_t count, int64_t cap, int width, hipStream_t st) {
    const int64_t k = std::min(count, cap);
    if (dst && k > 0) HIP_TRY(hipMemcpyAsync(dst, src_dev, sizeof(int64_t) * width * k, hipMemcpyDeviceToHost, st));
}

}  // namespace

void perf_reduce(jh_ctx *ctx, const jh_history *dh, const int64_t *time, const jh_perf_opts *opts, jh_perf_result *res,
                 const PerfOut &out, hipStream_t st) {
    memset(res, 0, sizeof *res);
    res->first_unpaired_invoke = -1;
    const int64_t n = dh->n, F = opts->f_count;
    if (n == 0) return;
    if (n > PF_MAX_ROWS) throw_jh(JH_EUNSUPPORTED, "perf: more than 2^31 - 2 rows");
    if (F > PF_MAX_F) throw_jh(JH_EUNSUPPORTED, "perf: f_count above 2^20");
    const int want = opts->want ? opts->want : JH_PERF_ALL;
    const int64_t dtq = opts->dt_quantiles ? opts->dt_quantiles : 30, dtr = opts->dt_rate ? opts->dt_rate : 10;
    DeviceTimer timer{ctx, st};
    timer.start();

    // 1. limits, ranges, pairing
    PMeta *m = ctx->ws<PMeta>(WS_PF_META, 1);
    k_pf_meta_init<<<1, 1, 0, st>>>(m);
    const int gr = grid_for(n, 256 * 4, 8192);
    // the two reducing kernels end in a handful of atomics per block on the same words: four blocks per CU
    const int gred = grid_for(n, 256 * 4, 4 * ctx->n_cu);
    k_pf_scan<<<gred, 256, 0, st>>>(dh->process, dh->f, time, n, F, m);
    PMeta mh = fetch(m, st);
    if (mh.bad_time) throw_jh(JH_EUNSUPPORTED, "perf: a nil or negative :time");
    if (mh.bad_f) throw_jh(JH_EUNSUPPORTED, "perf: an f code outside [0, f_count)");
    res->t_max = (int64_t)mh.t_max;

    unsigned long long *k64a = ctx->ws<unsigned long long>(WS_PF_K64A, n);
    unsigned long long *k64b = ctx->ws<unsigned long long>(WS_PF_K64B, n);
    int64_t *pair = nullptr;
    if (want & (JH_PERF_PAIR | JH_PERF_POINTS | JH_PERF_QUANTILES)) {
        uint32_t *va = ctx->ws<uint32_t>(WS_PF_V32A, n), *vb = ctx->ws<uint32_t>(WS_PF_V32B, n);
        pair = ctx->ws<int64_t>(WS_PF_PAIR, n);
        k_pf_keys<<<gr, 256, 0, st>>>(dh->process, dh->type, n, mh.p_min, k64a, va);
        const unsigned long long *ks = k64a;
        const uint32_t *vs = va;
        if (mh.p_max != mh.p_min) {                           // one process: the history order is the process order
            sort_pairs(ctx, WS_PF_TMP, as_input(k64a), k64b, as_input(va), vb, (int)n, pf_bits(mh.p_max - mh.p_min), st);
            ks = k64b; vs = vb;
        }
        k_pf_pair<<<grid_for((n + PF_TILE - 1) / PF_TILE, 1, 4 * ctx->n_cu), 256, 0, st>>>(ks, vs, time, n, pair, m);
        mh = fetch(m, st);
        res->n_invokes = (int64_t)mh.n_inv;
        res->n_paired = (int64_t)mh.n_paired;
        res->n_unpaired_invokes = (int64_t)mh.n_unp;
        res->first_unpaired_invoke = mh.first_unp == NONE ? -1 : (int64_t)mh.first_unp;
        if (want & JH_PERF_PAIR) pf_copy_out(out.pair, pair, n, out.pair_cap, 1, st);
    }
    int *n_runs = ctx->ws<int>(WS_PF_NRUNS, 1);

    // 2. raw points
    if ((want & JH_PERF_POINTS) && res->n_paired > 0) {
        const int64_t P = res->n_paired;
        uint32_t *ka = ctx->ws<uint32_t>(WS_PF_K32A, 2 * n), *kb = ka + n;
        uint32_t *ra = ctx->ws<uint32_t>(WS_PF_K32B, 2 * n), *rb = ra + n;
        const uint32_t sentinel = (uint32_t)(3 * F);
        k_pf_ptkey<<<gr, 256, 0, st>>>(dh->type, dh->f, pair, n, sentinel, ka, ra);
        sort_pairs(ctx, WS_PF_TMP, as_input(ka), kb, as_input(ra), rb, (int)n, pf_bits(sentinel), st);
        // the series: at most 3 F + 1 runs
        const int64_t max_runs = std::min<int64_t>(n, 3 * F + 1);
        uint32_t *uniq = ctx->ws<uint32_t>(WS_PF_RUN_U, max_runs);
        int *cnt = ctx->ws<int>(WS_PF_RUN_C, max_runs);
        pf_rle(ctx, as_input(kb), uniq, cnt, n_runs, (int)n, st);
        const int R = fetch(n_runs, st);
        std::vector<uint32_t> hu(R);
        std::vector<int> hc(R);
        HIP_TRY(hipMemcpyAsync(hu.data(), uniq, sizeof(uint32_t) * R, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(hc.data(), cnt, sizeof(int) * R, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        static const int64_t place_type[3] = {T_OK, T_INFO, T_FAIL};
        int64_t S = 0;
        for (int i = 0; i < R; i++) {
            if (hu[i] == sentinel) continue;
            if (out.series && S < out.series_cap) {
                out.series[3 * S] = hu[i] / 3;
                out.series[3 * S + 1] = place_type[hu[i] % 3];
                out.series[3 * S + 2] = hc[i];
            }
            S++;
        }
        res->n_series = S;
        const int64_t k = std::min(P, out.pt_cap);
        if (out.pt_row && k > 0) {
            int64_t *wide = ctx->ws<int64_t>(WS_PF_OUT, k);
            k_pf_widen<<<grid_for(k, 256, 8192), 256, 0, st>>>(rb, k, wide);
            pf_copy_out(out.pt_row, wide, P, out.pt_cap, 1, st);
            HIP_TRY(hipStreamSynchronize(st));                // WS_PF_OUT is written again below
        }
    }

    // 3. quantile groups
    if ((want & JH_PERF_QUANTILES) && res->n_unpaired_invokes == 0) {
        res->has_quantiles = 1;
        const int64_t M = res->n_invokes;
        if (M > 0) {
            uint32_t *ra = ctx->ws<uint32_t>(WS_PF_V32A, n), *rb = ctx->ws<uint32_t>(WS_PF_V32B, n);
            select_if(ctx, WS_PF_TMP, hipcub::CountingInputIterator<uint32_t>(0), ra, n_runs, (int)n, IsInvoke{dh->type}, st);
            unsigned long long *lk = k64a, *lk_s = k64b;
            unsigned long long *gk = ctx->ws<unsigned long long>(WS_PF_K64C, M), *gk_s = ctx->ws<unsigned long long>(WS_PF_K64D, M);
            const int gm = grid_for(M, 256 * 4, 8192);
            k_pf_latkey<<<gm, 256, 0, st>>>(ra, pair, time, M, mh.lat_min, lk);
            sort_pairs(ctx, WS_PF_TMP, as_input(lk), lk_s, as_input(ra), rb, (int)M, pf_bits(mh.lat_max - mh.lat_min), st);
            const int bbits = pf_bits((unsigned long long)pf_bucket(res->t_max, dtq));
            k_pf_gkey<<<gm, 256, 0, st>>>(rb, dh->f, time, M, dtq, bbits, gk);
            // lk is free again: the latencies in (f, bucket, latency) order
            sort_pairs(ctx, WS_PF_TMP, as_input(gk), gk_s, as_input(lk_s), lk, (int)M, bbits + pf_bits((unsigned long long)(F - 1)), st);
            unsigned long long *uniq = ctx->ws<unsigned long long>(WS_PF_RUN_U, M);
            int *cnt = ctx->ws<int>(WS_PF_RUN_C, M), *start = ctx->ws<int>(WS_PF_RUN_S, M);
            pf_rle(ctx, as_input(gk_s), uniq, cnt, n_runs, (int)M, st);
            const int64_t G = fetch(n_runs, st);
            res->n_groups = G;
            const int64_t k = std::min(G, out.group_cap);
            if (out.groups && k > 0) {
                excl_sum(ctx, WS_PF_TMP, as_input(cnt), start, (int)G, st);
                int64_t *rec = ctx->ws<int64_t>(WS_PF_OUT, 7 * k);
                k_pf_quant<<<grid_for(k, 256, 8192), 256, 0, st>>>(uniq, cnt, start, lk, mh.lat_min, bbits, k, rec);
                pf_copy_out(out.groups, rec, G, out.group_cap, 7, st);
                HIP_TRY(hipStreamSynchronize(st));
            }
        }
    }

    // 4. rate cells
    if (want & JH_PERF_RATE) {
        const int bbits = pf_bits((unsigned long long)pf_bucket(res->t_max, dtr));
        const unsigned long long sentinel = (unsigned long long)(4 * F) << bbits;
        k_pf_ratekey<<<gr, 256, 0, st>>>(dh->process, dh->type, dh->f, time, n, dtr, bbits, sentinel, k64a);
        sort_keys(ctx, WS_PF_TMP, as_input(k64a), k64b, (int)n, pf_bits(sentinel), st);
        unsigned long long *uniq = ctx->ws<unsigned long long>(WS_PF_RUN_U, n);
        int *cnt = ctx->ws<int>(WS_PF_RUN_C, n);
        pf_rle(ctx, as_input(k64b), uniq, cnt, n_runs, (int)n, st);
        const int64_t R = fetch(n_runs, st);
        const int64_t C = R - (fetch(uniq + (R - 1), st) == sentinel ? 1 : 0);   // R >= 1: n > 0
        res->n_cells = C;
        const int64_t k = std::min(C, out.cell_cap);
        if (out.cells && k > 0) {
            int64_t *rec = ctx->ws<int64_t>(WS_PF_OUT, 4 * k);
            k_pf_cells<<<grid_for(k, 256, 8192), 256, 0, st>>>(uniq, cnt, bbits, k, rec);
            pf_copy_out(out.cells, rec, C, out.cell_cap, 4, st);
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    res->device_ms = timer.stop();
}
