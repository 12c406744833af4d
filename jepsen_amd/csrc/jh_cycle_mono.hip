// jh_cycle_mono.hip -- monotonic-key-graph of jepsen.tests.cycle on MI355X: per
// key the :ok rows grouped by the value they observed, the groups in value order,
// and every row of a group linked to every row of the key's next group.
//
// jepsen/src/jepsen/tests/cycle.clj:218-267. include/jh.h states the semantics
// ("JH_CY_MONOTONIC", "Map reads encoding"); DESIGN.md §4k the design.
//
//   1. k_mo_rows      a counting and a filling pass, one thread per row: validation
//                     and the (k, v, row) records at the rows' exclusive sums. v is
//                     stored with its sign bit flipped, so unsigned order is the
//                     signed one and JH_NIL (INT64_MIN) comes first.
//   2. sort           two stable radix sorts, by v and then by k: the records in
//                     (k, v) order, rows ascending within a group (they were
//                     emitted in row order).
//   3. k_mo_flag      a flag where (k, v) changes; its inclusive sum numbers the
//      k_mo_gstart    groups and gives their starts.
//   4. k_mo_cnt       per source record: the start and the size of the next group
//                     when it has the same key, else 0.
//   5. an exclusive 64-bit sum of the sizes: the edges' places and their number,
//      which the caller checks before any edge buffer is sized.
//   6. k_mo_fill      the hot kernel: pack(row_src, row_dst) at every place; no
//                     holes. A workgroup takes a tile of TILE consecutive edges
//                     and finds the tile's first and last source record once. A
//                     tile of few sources (wide groups) streams each source's
//                     run of destination rows: coalesced 4 B loads, consecutive
//                     8 B stores. A tile of many sources (chains) takes one
//                     thread per edge with a binary search inside the tile's
//                     source range only, the stores still consecutive.
#include "cycle_common.h"

namespace {
constexpr int TILE = 2048;                    // edges of a workgroup's tile (8 per thread)
constexpr int FEW = 16;                       // sources of a tile up to which their runs are streamed
constexpr u64 SIGN = 1ULL << 63;

struct MMeta {
    unsigned bad_range, bad_dup, unsup_pairs, pad;
};

// every device array of one call (host struct, passed by value)
struct MP {
    const int64_t *process, *type, *value, *value2, *aux;
    int64_t n, n_pairs;
    long long M;
    long long *cr, *ro;                       // rows: pair counts and their exclusive sums (n + 1)
    u64 *rk, *rv, *t0, *t1, *sk;              // records; sort scratch; the sorted keys (t0: the sorted values)
    int32_t *rrow, *srow;                     // the records' rows, in row order and sorted
    uint32_t *idx, *idx_s, *idx2;
    int32_t *flag, *gid, *gstart, *dstart;    // gid: the inclusive sum of flag (group + 1)
    long long *cnt, *eoff;                    // M + 1
    MMeta *m;
};

__global__ void k_mo_meta_init(MMeta *m) { memset(m, 0, sizeof *m); }

// 1. ---------------------------------------------------------------------------
template <bool FILL>
__global__ void __launch_bounds__(256) k_mo_rows(const MP a) {
    CY_LOOP(i, a.n + 1) {
        long long c = 0;
        if (i < a.n && a.type[i] == T_OK && a.process[i] != -1) {
            long long s = a.value[i];
            c = a.value2[i];
            if (c == 0) s = 0;                                // nil or empty: value is not looked at
            if (c < 0 || s < 0 || s > a.n_pairs || c > a.n_pairs - s) { if (!FILL) atomicOr(&a.m->bad_range, 1u); c = 0; }
            else if (c > JH_CY_MAX_MOPS) { if (!FILL) atomicOr(&a.m->unsup_pairs, 1u); c = 0; }
            const int64_t *p = a.aux + 2 * s;
            if (!FILL) {
                bool dup = false;
                for (int j = 1; j < c && !dup; j++)
                    for (int q = 0; q < j && !dup; q++) dup = p[2 * q] == p[2 * j];
                if (dup) { atomicOr(&a.m->bad_dup, 1u); c = 0; }
            } else {
                const long long r0 = a.ro[i];
                for (int j = 0; j < c; j++) {
                    a.rk[r0 + j] = (u64)p[2 * j]; a.rv[r0 + j] = (u64)p[2 * j + 1] ^ SIGN;
                    a.rrow[r0 + j] = (int32_t)i; a.idx[r0 + j] = (uint32_t)(r0 + j);
                }
            }
        }
        if (!FILL) a.cr[i] = c;
    }
}

// 2. ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mo_gather_k(const MP a) {
    CY_LOOP(i, a.M) a.t1[i] = a.rk[a.idx_s[i]];
}

__global__ void __launch_bounds__(256) k_mo_gather(const MP a) {
    CY_LOOP(i, a.M) {
        const uint32_t x = a.idx2[i];
        a.t0[i] = a.rv[x]; a.srow[i] = a.rrow[x];
    }
}

// 3. ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mo_flag(const MP a) {
    CY_LOOP(i, a.M) a.flag[i] = (i == 0 || a.sk[i] != a.sk[i - 1] || a.t0[i] != a.t0[i - 1]) ? 1 : 0;
}

// gstart[g] = the first record of group g; gstart[G] = gstart[G + 1] = M
__global__ void __launch_bounds__(256) k_mo_gstart(const MP a) {
    const int32_t G = a.gid[a.M - 1];
    CY_LOOP(i, a.M + 2) {
        if (i >= a.M) a.gstart[G + (i - a.M)] = (int32_t)a.M;
        else if (a.flag[i]) a.gstart[a.gid[i] - 1] = (int32_t)i;
    }
}

// 4. ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mo_cnt(const MP a) {
    const int32_t G = a.gid[a.M - 1];
    CY_LOOP(i, a.M + 1) {
        long long c = 0;
        if (i < a.M) {
            const int32_t g = a.gid[i] - 1;
            int32_t d = 0;
            if (g + 1 < G) {
                d = a.gstart[g + 1];
                if (a.sk[d] == a.sk[i]) c = a.gstart[g + 2] - d;
            }
            a.dstart[i] = d;
        }
        a.cnt[i] = c;
    }
}

// 6. ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mo_fill(const long long *__restrict__ eoff, const int32_t *__restrict__ dstart,
                                                 const int32_t *__restrict__ srow, long long M, long long total,
                                                 u64 *__restrict__ raw) {
    __shared__ long long s_i[2];
    const long long tiles = (total + TILE - 1) / TILE;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long long lo = t * TILE, hi = min(lo + TILE, total);
        __syncthreads();
        if (threadIdx.x < 2) s_i[threadIdx.x] = cy_owner(eoff, M, threadIdx.x ? hi - 1 : lo);
        __syncthreads();
        const long long i0 = s_i[0], i1 = s_i[1];
        if (i1 - i0 < FEW) {
            for (long long i = i0; i <= i1; i++) {
                const long long b = eoff[i], e0 = max(b, lo), e1 = min(eoff[i + 1], hi);
                if (e0 >= e1) continue;
                const u64 src = (u64)srow[i] << 32;
                const long long d0 = dstart[i] - b;           // the destination record of edge e is d0 + e
                for (long long e = e0 + threadIdx.x; e < e1; e += blockDim.x) raw[e] = src | (u64)(uint32_t)srow[d0 + e];
            }
        } else {
            for (long long e = lo + threadIdx.x; e < hi; e += blockDim.x) {
                long long l = i0, h = i1;                     // the last source of the tile with eoff <= e
                while (l < h) {
                    const long long mid = (l + h + 1) >> 1;
                    if (eoff[mid] <= e) l = mid;
                    else h = mid - 1;
                }
                raw[e] = pack(srow[l], srow[dstart[l] + (e - eoff[l])]);
            }
        }
    }
}
}  // namespace

MonoPlan mono_plan(jh_ctx *ctx, const jh_history *dh, jh_cycle_result *res, hipStream_t st) {
    MonoPlan plan;
    MP a = {};
    a.process = dh->process; a.type = dh->type; a.value = dh->value; a.value2 = dh->value2; a.aux = dh->aux;
    a.n = dh->n; a.n_pairs = dh->n_aux / 2;
    const int64_t n = a.n;
    a.m = ctx->ws<MMeta>(WS_CY_MO_META, 1);
    k_mo_meta_init<<<1, 1, 0, st>>>(a.m);
    carve(ctx, WS_CY_MO_ROWS, [&](Arena &r) { r.take(a.cr, n + 1); r.take(a.ro, n + 1); });
    const int g = grid_for(n + 1, 256, 2048);

    // 1. records
    k_mo_rows<false><<<g, 256, 0, st>>>(a);
    excl_sum(ctx, WS_CY_TMP, as_input(a.cr), a.ro, (int)(n + 1), st);
    HIP_TRY(hipMemcpyAsync(&a.M, a.ro + n, sizeof a.M, hipMemcpyDeviceToHost, st));
    const MMeta mh = fetch(a.m, st);
    if (mh.bad_range) throw_jh(JH_EINVAL, "cycle: a map's pair range leaves [0, n_aux / 2) or has a negative count");
    if (mh.bad_dup) throw_jh(JH_EINVAL, "cycle: a map that names one key twice");
    if (mh.unsup_pairs) throw_jh(JH_EUNSUPPORTED, "cycle: a map of more than JH_CY_MAX_MOPS pairs");
    const long long M = a.M;
    if (M > Y_MAX) throw_jh(JH_EUNSUPPORTED, "cycle: more than 2^31 - 2 records");
    res->entries = M;
    if (M == 0) return plan;
    carve(ctx, WS_CY_MO_RECS, [&](Arena &r) {
        r.take(a.rk, M); r.take(a.rv, M); r.take(a.t0, M); r.take(a.t1, M); r.take(a.sk, M);
        r.take(a.cnt, M + 1); r.take(a.eoff, M + 1);
        r.take(a.rrow, M); r.take(a.srow, M); r.take(a.idx, M); r.take(a.idx_s, M); r.take(a.idx2, M);
        r.take(a.flag, M); r.take(a.gid, M); r.take(a.gstart, M + 2); r.take(a.dstart, M);
    });
    const int gm = grid_for(M + 2, 256, 4096);
    k_mo_rows<true><<<g, 256, 0, st>>>(a);

    // 2. the records in (k, v) order
    sort_pairs(ctx, WS_CY_TMP, a.rv, a.t0, a.idx, a.idx_s, (int)M, 64, st);
    k_mo_gather_k<<<gm, 256, 0, st>>>(a);
    sort_pairs(ctx, WS_CY_TMP, a.t1, a.sk, a.idx_s, a.idx2, (int)M, 64, st);
    k_mo_gather<<<gm, 256, 0, st>>>(a);

    // 3-5. groups, the next group of every record, the edges' places
    k_mo_flag<<<gm, 256, 0, st>>>(a);
    incl_sum(ctx, WS_CY_TMP, a.flag, a.gid, (int)M, st);
    k_mo_gstart<<<gm, 256, 0, st>>>(a);
    k_mo_cnt<<<gm, 256, 0, st>>>(a);
    excl_sum(ctx, WS_CY_TMP, as_input(a.cnt), a.eoff, (int)(M + 1), st);
    const long long total = fetch(a.eoff + M, st);
    if (total > Y_MAX) throw_jh(JH_EUNSUPPORTED, "cycle: more than 2^31 - 2 vertices or edges");
    plan.records = M; plan.slots = total;
    plan.eoff = a.eoff; plan.dstart = a.dstart; plan.srow = a.srow;
    return plan;
}

void mono_fill(jh_ctx *ctx, const MonoPlan &plan, unsigned long long *raw, hipStream_t st) {
    if (plan.slots == 0) return;
    const long long tiles = (plan.slots + TILE - 1) / TILE;
    k_mo_fill<<<grid_for(tiles, 1, 16384), 256, 0, st>>>(plan.eoff, plan.dstart, plan.srow, plan.records, plan.slots, raw);
}
