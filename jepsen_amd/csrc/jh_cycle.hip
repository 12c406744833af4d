// jh_cycle.hip -- jepsen.tests.cycle on MI355X: dependency graphs over completion
// rows and their strongly connected components.
//
// jepsen/src/jepsen/tests/cycle.clj:150-160 (tarjan), :202-216 (combine),
// :271-300 (process-graph), :315-377 (realtime-graph), :703-779 (wr-graph),
// :911-934 (checker); txn/src/jepsen/txn.clj:5-28 (ext-reads / ext-writes).
// include/jh.h states the semantics; DESIGN.md §4i the design.
//
// Pipeline. An edge is one 64-bit word, src << 32 | dst (rows < 2^31).
//   1. builders       k_cy_txn (a counting and a filling pass): one thread per :ok txn,
//                     its external reads and writes as (k, v, row) records; the
//                     writes are sorted on a hash of (k, v), k_cy_wr_join looks
//                     every read up (collisions compare k and v).
//                     k_cy_pair over the rows in a stable sort by process: each
//                     invoke's completion, the pairing causes, and the process
//                     edges (an :ok row walks back to the process' previous :ok).
//                     realtime: a reverse min-scan gives R(c), a prefix count of
//                     invokes the number of edges, an exclusive sum their place,
//                     k_cy_rt_fill one thread per edge.
//                     appends-and-reads-graph (JH_CY_APPEND, in place of wr) is
//                     jh_cycle_append.hip: append_plan verifies and sizes,
//                     append_fill writes the wr / ww / rw slots.
//                     monotonic-key-graph (JH_CY_MONOTONIC) is jh_cycle_mono.hip:
//                     mono_plan sorts the (k, v, row) records and counts,
//                     mono_fill writes every edge.
//                     Builders leave holes (~0) where a slot has no edge; one
//                     select compacts process | realtime | wr | append |
//                     monotonic | extra.
//   2. regions        reach[dst] = max src over the back edges (atomicMax), an
//                     inclusive max-scan, boundary flags and their prefix sum:
//                     the regions of >= 2 vertices as [start, end] row intervals.
//                     The edges inside one region (self-loops dropped) are
//                     sorted into a CSR by source and one by destination.
//   3. k_cy_region    one workgroup per region, regions handed out by a counter.
//                     Worklist (Kahn) trimming on in- and out-degree; then, while
//                     a vertex is left: the smallest one is the pivot, its
//                     backward reach by worklist, its forward reach within that:
//                     the SCC, which is removed and seeds the next trimming.
//                     LDS = true: degrees, status and queue in LDS (regions of at
//                     most JH_CY_LDS_VERTICES vertices); false: the same code
//                     with them in HBM, indexed by row.
//   4. results        counts; the SCCs ordered by (size, smallest row) by two
//                     radix sorts (roots, members).
#include "cycle_common.h"
#include <algorithm>
#include <vector>

namespace {
constexpr int CAP = JH_CY_LDS_VERTICES;
constexpr int RT = 256;                       // threads of a region's workgroup
constexpr int REMOVED = 0x7fffffff;           // status: out of the region's graph
constexpr int BIG = 0x7fffffff;

struct YMeta {
    unsigned bad_range, unsup_f, unsup_mops, bad_type, over_work, pad;
    u64 dbl_row, orphan_row, unmatched_row, first_ok, multi_row;
    u64 edges[4], back, entries;
    u64 max_region, global_regions, scc_count, scc_vertices;
    long long unknown_key, unknown_value, unknown_rows[2];
    unsigned counter[2];
};

__global__ void k_cy_meta_init(YMeta *m) {
    memset(m, 0, sizeof *m);
    m->dbl_row = m->orphan_row = m->unmatched_row = m->first_ok = m->multi_row = NONE;
    m->unknown_key = m->unknown_value = JH_NIL;
    m->unknown_rows[0] = m->unknown_rows[1] = -1;
}


// ---------------------------------------------------------------------------
// 1a. rows: the sort key by process, :type check, the first :ok row
__global__ void __launch_bounds__(256) k_cy_rows(const int64_t *__restrict__ process, const int64_t *__restrict__ type,
                                                 int64_t n, int64_t *__restrict__ pkey, int32_t *__restrict__ prow,
                                                 int32_t *__restrict__ comp, YMeta *m) {
    CY_LOOP(i, n) {
        const int64_t t = type[i], p = process[i];
        if (t < 0 || t > 3) atomicOr(&m->bad_type, 1u);
        if (t == T_OK && p != -1) atomicMin(&m->first_ok, (u64)i);
        if (pkey) { pkey[i] = p; prow[i] = (int32_t)i; comp[i] = -1; }
    }
}

// over the rows sorted by process (stable: history order within a process)
__global__ void __launch_bounds__(256) k_cy_pair(const int64_t *__restrict__ skey, const int32_t *__restrict__ srow,
                                                 const int64_t *__restrict__ type, int64_t n, int do_process,
                                                 int32_t *__restrict__ comp, u64 *__restrict__ raw, YMeta *m) {
    __shared__ u64 sh[4];
    u64 ne = 0;
    CY_LOOP(j, n) {
        const int64_t p = skey[j];
        u64 e = HOLE;
        if (p != -1) {
            const int r = srow[j];
            const int64_t t = type[r];
            const bool has_prev = j > 0 && skey[j - 1] == p, has_next = j + 1 < n && skey[j + 1] == p;
            const int64_t tp = has_prev ? type[srow[j - 1]] : -1;
            if (t == T_INVOKE) {
                if (tp == T_INVOKE) atomicMin(&m->dbl_row, (u64)r);
                if (has_next && type[srow[j + 1]] != T_INVOKE) comp[r] = srow[j + 1];
            } else if ((t == T_OK || t == T_FAIL) && tp != T_INVOKE) {
                atomicMin(&m->orphan_row, (u64)r);
            }
            if (do_process && t == T_OK) {
                // back to the process' previous :ok. The walks of one process are disjoint, so the work is
                // linear in all, but one thread walks a whole run of non-:ok rows alone: a process with a very
                // long run (all :fail, say) bounds this kernel's latency by that run's length
                for (int64_t q = j - 1; q >= 0 && skey[q] == p; q--)
                    if (type[srow[q]] == T_OK) { e = pack(srow[q], r); ne++; break; }
            }
        }
        if (do_process) raw[j] = e;
    }
    ne = block_reduce256(ne, RedSum(), sh);
    if (threadIdx.x == 0 && ne) atomicAdd(&m->edges[0], ne);
}

// 1b. realtime. rev[n - 1 - i] = the completion row of an invoke at i whose
// completion is :ok (else n); isinv[i] = 1 for an invoke (isinv[n] = 0)
__global__ void __launch_bounds__(256) k_cy_rt_key(const int64_t *__restrict__ process, const int64_t *__restrict__ type,
                                                   const int32_t *__restrict__ comp, int64_t n, int32_t *__restrict__ rev,
                                                   int32_t *__restrict__ isinv, YMeta *m) {
    const u64 first_ok = m->first_ok;
    CY_LOOP(i, n + 1) {
        if (i == n) { isinv[i] = 0; continue; }
        const bool inv = type[i] == T_INVOKE && process[i] != -1;
        const int c = inv ? comp[i] : -1;
        isinv[i] = inv ? 1 : 0;
        rev[n - 1 - i] = (c >= 0 && type[c] == T_OK) ? c : (int32_t)n;
        if (inv && c < 0 && first_ok != NONE && (u64)i > first_ok) atomicMin(&m->unmatched_row, (u64)i);
    }
}

// cnt[c] = the invokes in (c, R(c)) for an :ok row c; icomp = the invokes' completions in row order
__global__ void __launch_bounds__(256) k_cy_rt_count(const int64_t *__restrict__ process, const int64_t *__restrict__ type,
                                                     const int32_t *__restrict__ comp, const int32_t *__restrict__ sufmin,
                                                     const int32_t *__restrict__ ip, int64_t n, long long *__restrict__ cnt,
                                                     int32_t *__restrict__ icomp) {
    CY_LOOP(i, n + 1) {
        long long c = 0;
        if (i < n && process[i] != -1) {
            if (type[i] == T_OK) c = ip[sufmin[n - 1 - i]] - ip[i + 1];
            else if (type[i] == T_INVOKE) icomp[ip[i]] = comp[i];
        }
        cnt[i] = c;
    }
}

__global__ void __launch_bounds__(256) k_cy_rt_fill(const long long *__restrict__ off, const int32_t *__restrict__ ip,
                                                    const int32_t *__restrict__ icomp, int64_t n, long long total,
                                                    u64 *__restrict__ raw) {
    CY_LOOP(e, total) {
        int64_t lo = 0, hi = n;                               // the last row with off[row] <= e
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (off[mid] <= e) lo = mid;
            else hi = mid - 1;
        }
        raw[e] = pack(lo, icomp[ip[lo + 1] + (e - off[lo])]);
    }
}

// 1c. wr. One thread per :ok txn row: validation and the numbers of its
// external reads and writes (FILL: the records, at the rows' exclusive sums)
template <bool FILL>
__global__ void __launch_bounds__(256) k_cy_txn(const int64_t *__restrict__ process, const int64_t *__restrict__ type,
                                                const int64_t *__restrict__ value, const int64_t *__restrict__ value2,
                                                const int64_t *__restrict__ aux, int64_t n, int64_t n_mops,
                                                long long *__restrict__ cr, long long *__restrict__ cw,
                                                int64_t *__restrict__ rk, int64_t *__restrict__ rv, int32_t *__restrict__ rrow,
                                                int64_t *__restrict__ wk, int64_t *__restrict__ wv, int32_t *__restrict__ wrow,
                                                u64 *__restrict__ whash, uint32_t *__restrict__ widx, YMeta *m) {
    __shared__ u64 sh[4];
    u64 ent = 0;
    CY_LOOP(i, n + 1) {
        long long nr = 0, nw = 0;
        if (i < n && type[i] == T_OK && process[i] != -1) {
            long long s = value[i], c = value2[i];
            if (c == 0) s = 0;                                // nil or empty: value is not looked at
            if (c < 0 || s < 0 || s > n_mops || c > n_mops - s) { if (!FILL) atomicOr(&m->bad_range, 1u); c = 0; }
            else if (c > JH_CY_MAX_MOPS) { if (!FILL) atomicOr(&m->unsup_mops, 1u); c = 0; }
            const int64_t *t = aux + 3 * s;
            long long ro = FILL ? cr[i] : 0, wo = FILL ? cw[i] : 0;
            ent += (u64)c;
            for (int j = 0; j < c; j++) {
                const int64_t f = t[3 * j], k = t[3 * j + 1];
                if (f != JH_F_READ && f != JH_F_WRITE) { if (!FILL) atomicOr(&m->unsup_f, 1u); continue; }
                bool keep = true;
                if (f == JH_F_READ) {
                    for (int q = 0; q < j && keep; q++) keep = t[3 * q + 1] != k;
                } else {
                    for (int q = j + 1; q < c && keep; q++) keep = !(t[3 * q + 1] == k && t[3 * q] == JH_F_WRITE);
                }
                if (!keep) continue;
                if (f == JH_F_READ) {
                    if (FILL) { rk[ro + nr] = k; rv[ro + nr] = t[3 * j + 2]; rrow[ro + nr] = (int32_t)i; }
                    nr++;
                } else {
                    if (FILL) {
                        const int64_t v = t[3 * j + 2];
                        wk[wo + nw] = k; wv[wo + nw] = v; wrow[wo + nw] = (int32_t)i;
                        whash[wo + nw] = cy_hash(k, v);
                        widx[wo + nw] = (uint32_t)(wo + nw);
                    }
                    nw++;
                }
            }
        }
        if (!FILL) { cr[i] = nr; cw[i] = nw; }
    }
    if (!FILL) {
        ent = block_reduce256(ent, RedSum(), sh);
        if (threadIdx.x == 0 && ent) atomicAdd(&m->entries, ent);
    }
}

// the writers of (k, v): their number, the first two in row order (the sort is stable)
__device__ __forceinline__ int cy_writers(const u64 *__restrict__ shash, const uint32_t *__restrict__ sidx,
                                          const int64_t *__restrict__ wk, const int64_t *__restrict__ wv,
                                          const int32_t *__restrict__ wrow, long long W, int64_t k, int64_t v, int *w0,
                                          int *w1) {
    const u64 h = cy_hash(k, v);
    long long lo = 0, hi = W;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (shash[mid] < h) lo = mid + 1;
        else hi = mid;
    }
    int cnt = 0;
    for (; lo < W && shash[lo] == h; lo++) {
        const uint32_t x = sidx[lo];
        if (wk[x] != k || wv[x] != v) continue;
        if (cnt == 0) *w0 = wrow[x];
        else if (cnt == 1) *w1 = wrow[x];
        cnt++;
    }
    return cnt;
}

__global__ void __launch_bounds__(256) k_cy_wr_join(const int64_t *__restrict__ rk, const int64_t *__restrict__ rv,
                                                    const int32_t *__restrict__ rrow, long long R,
                                                    const u64 *__restrict__ shash, const uint32_t *__restrict__ sidx,
                                                    const int64_t *__restrict__ wk, const int64_t *__restrict__ wv,
                                                    const int32_t *__restrict__ wrow, long long W, u64 *__restrict__ raw,
                                                    YMeta *m) {
    __shared__ u64 sh[4];
    u64 ne = 0;
    CY_LOOP(i, R) {
        int w0 = -1, w1 = -1;
        const int c = cy_writers(shash, sidx, wk, wv, wrow, W, rk[i], rv[i], &w0, &w1);
        u64 e = HOLE;
        if (c == 1) { e = pack(w0, rrow[i]); ne++; }
        else if (c > 1) atomicMin(&m->multi_row, (u64)rrow[i]);
        raw[i] = e;
    }
    ne = block_reduce256(ne, RedSum(), sh);
    if (threadIdx.x == 0 && ne) atomicAdd(&m->edges[2], ne);
}

// the smallest reader row of a pair with several writers: its first such pair in micro-op order
__global__ void k_cy_wr_unknown(const long long *__restrict__ roff, const int64_t *__restrict__ rk,
                                const int64_t *__restrict__ rv, const u64 *__restrict__ shash,
                                const uint32_t *__restrict__ sidx, const int64_t *__restrict__ wk,
                                const int64_t *__restrict__ wv, const int32_t *__restrict__ wrow, long long W, YMeta *m) {
    const u64 row = m->multi_row;
    if (row == NONE) return;
    for (long long i = roff[row]; i < roff[row + 1]; i++) {
        int w0 = -1, w1 = -1;
        if (cy_writers(shash, sidx, wk, wv, wrow, W, rk[i], rv[i], &w0, &w1) > 1) {
            m->unknown_key = rk[i]; m->unknown_value = rv[i];
            m->unknown_rows[0] = w0; m->unknown_rows[1] = w1;
            return;
        }
    }
}

struct NotHole {
    __host__ __device__ bool operator()(const u64 &x) const { return x != HOLE; }
};

// ---------------------------------------------------------------------------
// 2. regions
__global__ void __launch_bounds__(256) k_cy_iota(int32_t *__restrict__ p, int64_t cnt) {
    CY_LOOP(i, cnt) p[i] = (int32_t)i;
}

__global__ void __launch_bounds__(256) k_cy_reach(const u64 *__restrict__ edges, long long E, int32_t *__restrict__ reach,
                                                  YMeta *m) {
    __shared__ u64 sh[4];
    u64 nb = 0;
    CY_LOOP(e, E) {
        const int s = (int)(edges[e] >> 32), d = (int)(uint32_t)edges[e];
        if (d < s) { atomicMax(&reach[d], s); nb++; }
    }
    nb = block_reduce256(nb, RedSum(), sh);
    if (threadIdx.x == 0 && nb) atomicAdd(&m->back, nb);
}

// mx = the inclusive max-scan of reach. A region starts at v when nothing before
// v reaches it; it has two or more vertices when v itself reaches further
__global__ void __launch_bounds__(256) k_cy_starts(const int32_t *__restrict__ reach, const int32_t *__restrict__ mx,
                                                   int64_t n, int32_t *__restrict__ big) {
    CY_LOOP(v, n) big[v] = ((v == 0 || mx[v - 1] < v) && reach[v] > v) ? 1 : 0;
}

// bs = the inclusive sum of big: region bs[v] - 1 is the latest one that starts at or before v
__global__ void __launch_bounds__(256) k_cy_bounds(const int32_t *__restrict__ mx, const int32_t *__restrict__ big,
                                                   const int32_t *__restrict__ bs, int64_t n, int32_t *__restrict__ rstart,
                                                   int32_t *__restrict__ rend) {
    CY_LOOP(v, n) {
        const bool start = v == 0 || mx[v - 1] < v;
        if (big[v]) rstart[bs[v] - 1] = (int32_t)v;
        if (mx[v] == v && !start) rend[bs[v] - 1] = (int32_t)v;
    }
}

__global__ void __launch_bounds__(256) k_cy_region_stats(const int32_t *__restrict__ rstart, const int32_t *__restrict__ rend,
                                                         int64_t NR, int force_global, YMeta *m) {
    __shared__ u64 sh[4];
    u64 mxv = 0, ng = 0;
    CY_LOOP(r, NR) {
        const u64 V = (u64)(rend[r] - rstart[r] + 1);
        mxv = max(mxv, V);
        if (V > (u64)CAP || force_global) ng++;
    }
    mxv = block_reduce256(mxv, RedMax(), sh);
    ng = block_reduce256(ng, RedSum(), sh);
    if (threadIdx.x == 0) { if (mxv) atomicMax(&m->max_region, mxv); if (ng) atomicAdd(&m->global_regions, ng); }
}

// the edges inside one region, self-loops dropped; bwd = the same edges as dst << 32 | src
__global__ void __launch_bounds__(256) k_cy_intra(const u64 *__restrict__ edges, long long E, const int32_t *__restrict__ bs,
                                                  const int32_t *__restrict__ rend, u64 *__restrict__ fwd) {
    CY_LOOP(e, E) {
        const int s = (int)(edges[e] >> 32), d = (int)(uint32_t)edges[e];
        const int a = bs[s] - 1, b = bs[d] - 1;
        fwd[e] = (s != d && a >= 0 && a == b && s <= rend[a] && d <= rend[a]) ? edges[e] : HOLE;
    }
}

__global__ void __launch_bounds__(256) k_cy_swap(const u64 *__restrict__ in, long long E, u64 *__restrict__ out) {
    CY_LOOP(e, E) out[e] = (in[e] << 32) | (in[e] >> 32);
}

// off[v] = the sorted edges whose first half is below v, v = 0 .. n
__global__ void __launch_bounds__(256) k_cy_csr(const u64 *__restrict__ sorted, long long E, int64_t n,
                                                int32_t *__restrict__ off) {
    CY_LOOP(v, n + 1) {
        long long lo = 0, hi = E;
        const u64 key = (u64)v << 32;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (sorted[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        off[v] = (int32_t)lo;
    }
}

// ---------------------------------------------------------------------------
// 3. one workgroup per region
template <bool LDS>
__device__ __forceinline__ int y_ld(const int *p) {
    // the state is written by this workgroup's stores and atomics: the global
    // tier reads past the CU's L1, which atomics (done in L2) do not update
    if constexpr (LDS) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ void y_st(int *p, int v) {
    if constexpr (LDS) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ void y_sync() {
    if (!LDS) __threadfence();
    __syncthreads();
}

// Status of a vertex: REMOVED, or epoch * 4 + marks (2: backward-reached, 3: and
// forward-reached) of the pivot number `epoch`; marks of earlier pivots are stale.
// The queue holds local vertex numbers; every vertex enters it once per use: as
// a trimmed vertex (once in the region's life), in a pivot's backward search,
// and in its forward search, both of which start the queue afresh.
template <bool LDS>
__global__ void __launch_bounds__(RT) k_cy_region(const int32_t *__restrict__ rstart, const int32_t *__restrict__ rend, int NR,
                                                  const int32_t *__restrict__ foff, const u64 *__restrict__ fwd,
                                                  const int32_t *__restrict__ boff, const u64 *__restrict__ bwd,
                                                  int force_global, int *__restrict__ g_state, int64_t n,
                                                  int32_t *__restrict__ labels, int32_t *__restrict__ sccsize, YMeta *m) {
    __shared__ int s_din[LDS ? CAP : 1], s_dout[LDS ? CAP : 1], s_stat[LDS ? CAP : 1], s_q[LDS ? CAP : 1];
    __shared__ int s_r, s_head, s_tail, s_min;
    __shared__ u64 s_work;
    const int tid = threadIdx.x;
    for (;;) {
        __syncthreads();
        if (tid == 0) s_r = (int)atomicAdd(&m->counter[LDS ? 0 : 1], 1u);
        __syncthreads();
        const int r = s_r;
        if (r >= NR) return;
        const int a = rstart[r], V = rend[r] - a + 1;
        if ((V <= CAP && !force_global) != LDS) continue;
        int *din, *dout, *stat, *q;
        if constexpr (LDS) { din = s_din; dout = s_dout; stat = s_stat; q = s_q; }
        else { din = g_state + a; dout = g_state + n + a; stat = g_state + 2 * n + a; q = g_state + 3 * n + a; }
        const u64 cap = (u64)JH_CY_WORK_MULT * ((u64)V + (u64)(foff[a + V] - foff[a]));
        if (tid == 0) { s_head = 0; s_tail = 0; s_work = 0; }
        for (int u = tid; u < V; u += RT) {
            y_st<LDS>(din + u, boff[a + u + 1] - boff[a + u]);
            y_st<LDS>(dout + u, foff[a + u + 1] - foff[a + u]);
            y_st<LDS>(stat + u, 0);
        }
        y_sync<LDS>();
        for (int u = tid; u < V; u += RT)
            if (y_ld<LDS>(din + u) == 0 || y_ld<LDS>(dout + u) == 0) {
                y_st<LDS>(stat + u, REMOVED);
                y_st<LDS>(q + atomicAdd(&s_tail, 1), u);
            }
        int cursor = 0, epoch = 0;
        u64 w = 0;
        bool over = false;
        for (;;) {
            // trim: the queue's vertices are removed already; their neighbours lose a degree
            for (;;) {
                y_sync<LDS>();
                const int h = s_head, t = s_tail;
                __syncthreads();
                if (h == t) break;
                for (int i = h + tid; i < t; i += RT) {
                    const int x = y_ld<LDS>(q + i);
                    for (int e = foff[a + x]; e < foff[a + x + 1]; e++) {
                        const int y = (int)(uint32_t)fwd[e] - a;
                        if (atomicSub(din + y, 1) == 1 && atomicExch(stat + y, REMOVED) != REMOVED)
                            y_st<LDS>(q + atomicAdd(&s_tail, 1), y);
                    }
                    for (int e = boff[a + x]; e < boff[a + x + 1]; e++) {
                        const int z = (int)(uint32_t)bwd[e] - a;
                        if (atomicSub(dout + z, 1) == 1 && atomicExch(stat + z, REMOVED) != REMOVED)
                            y_st<LDS>(q + atomicAdd(&s_tail, 1), z);
                    }
                    w += (u64)(foff[a + x + 1] - foff[a + x]) + (u64)(boff[a + x + 1] - boff[a + x]);
                }
                if (tid == 0) s_head = t;
            }
            // the pivot: the smallest vertex left (the cursor never goes back)
            int pivot = -1;
            while (cursor < V) {
                if (tid == 0) s_min = BIG;
                __syncthreads();
                const int c = cursor + tid;
                if (c < V && y_ld<LDS>(stat + c) != REMOVED) atomicMin(&s_min, c);
                __syncthreads();
                const int got = s_min;
                __syncthreads();
                if (got != BIG) { pivot = got; cursor = got; break; }
                cursor += RT;
            }
            if (pivot < 0) break;
            if (w) { atomicAdd(&s_work, w); w = 0; }
            __syncthreads();
            if (s_work > cap || epoch >= (1 << 28)) { over = true; break; }
            epoch++;
            const int mb = epoch * 4 + 2, mf = epoch * 4 + 3;
            // backward reach over the vertices left
            __syncthreads();
            if (tid == 0) { y_st<LDS>(stat + pivot, mb); y_st<LDS>(q, pivot); s_head = 0; s_tail = 1; }
            for (;;) {
                y_sync<LDS>();
                const int h = s_head, t = s_tail;
                __syncthreads();
                if (h == t) break;
                for (int i = h + tid; i < t; i += RT) {
                    const int x = y_ld<LDS>(q + i);
                    for (int e = boff[a + x]; e < boff[a + x + 1]; e++) {
                        const int z = (int)(uint32_t)bwd[e] - a;
                        const int old = y_ld<LDS>(stat + z);
                        if (old == REMOVED || old == mb) continue;
                        if (atomicCAS(stat + z, old, mb) == old) y_st<LDS>(q + atomicAdd(&s_tail, 1), z);
                    }
                    w += (u64)(boff[a + x + 1] - boff[a + x]);
                }
                if (tid == 0) s_head = t;
            }
            // forward reach within it: the queue ends up holding the pivot's SCC
            if (tid == 0) { y_st<LDS>(stat + pivot, mf); y_st<LDS>(q, pivot); s_head = 0; s_tail = 1; }
            for (;;) {
                y_sync<LDS>();
                const int h = s_head, t = s_tail;
                __syncthreads();
                if (h == t) break;
                for (int i = h + tid; i < t; i += RT) {
                    const int x = y_ld<LDS>(q + i);
                    for (int e = foff[a + x]; e < foff[a + x + 1]; e++) {
                        const int y = (int)(uint32_t)fwd[e] - a;
                        if (y_ld<LDS>(stat + y) != mb) continue;
                        if (atomicCAS(stat + y, mb, mf) == mb) y_st<LDS>(q + atomicAdd(&s_tail, 1), y);
                    }
                    w += (u64)(foff[a + x + 1] - foff[a + x]);
                }
                if (tid == 0) s_head = t;
            }
            // remove the SCC; its members seed the next trimming
            const int size = s_tail;
            if (tid == 0) { s_min = BIG; s_head = 0; }
            __syncthreads();
            int mn = BIG;
            for (int i = tid; i < size; i += RT) mn = min(mn, y_ld<LDS>(q + i));
            if (mn != BIG) atomicMin(&s_min, mn);
            __syncthreads();
            const int label = a + s_min;
            for (int i = tid; i < size; i += RT) {
                const int x = y_ld<LDS>(q + i);
                y_st<LDS>(stat + x, REMOVED);
                if (size > 1) labels[a + x] = label;
            }
            if (tid == 0 && size > 1) sccsize[label] = size;
        }
        if (over && tid == 0) atomicOr(&m->over_work, 1u);
    }
}

// ---------------------------------------------------------------------------
// 4. results
__global__ void __launch_bounds__(256) k_cy_fill32(int32_t *__restrict__ p, int64_t cnt, int32_t v) {
    CY_LOOP(i, cnt) p[i] = v;
}

// keys (size << 32 | root): of the roots (ROOTS) or of every member row; holes elsewhere
template <bool ROOTS>
__global__ void __launch_bounds__(256) k_cy_keys(const int32_t *__restrict__ labels, const int32_t *__restrict__ sccsize,
                                                 int64_t n, u64 *__restrict__ keys, YMeta *m) {
    __shared__ u64 sh[4];
    u64 nc = 0, nv = 0;
    CY_LOOP(v, n) {
        u64 k = HOLE;
        if (ROOTS) {
            const int s = sccsize[v];
            if (s > 0) { k = ((u64)s << 32) | (u64)v; nc++; nv += (u64)s; }
        } else {
            const int l = labels[v];
            if (l >= 0) k = ((u64)sccsize[l] << 32) | (u64)l;
        }
        keys[v] = k;
    }
    if (ROOTS) {
        nc = block_reduce256(nc, RedSum(), sh);
        nv = block_reduce256(nv, RedSum(), sh);
        if (threadIdx.x == 0 && nc) { atomicAdd(&m->scc_count, nc); atomicAdd(&m->scc_vertices, nv); }
    }
}

struct Flag64 {
    const u64 *k;
    __host__ __device__ bool operator()(const int32_t &v) const { return k[v] != HOLE; }
};

int bits_of(u64 x) {
    int b = 1;
    while (b < 64 && (x >> b)) b++;
    return b;
}

// the words of `in` that are not holes, in order; returns their number
long long select_edges(jh_ctx *ctx, const u64 *in, u64 *out, long long cnt, hipStream_t st) {
    if (cnt == 0) return 0;
    long long *d_n = (long long *)ctx->ws<long long>(WS_CY_SEL, 1);
    select_if(ctx, WS_CY_TMP, in, out, d_n, (int)cnt, NotHole(), st);
    return fetch(d_n, st);
}

void init_result(jh_cycle_result *res) {
    memset(res, 0, sizeof *res);
    res->valid = JH_VALID;
    res->unknown_row = -1;
    res->unknown_key = res->unknown_value = JH_NIL;
    res->unknown_rows[0] = res->unknown_rows[1] = -1;
}

void empty_outputs(int64_t n, const CycleOut &out) {
    if (out.labels) std::fill(out.labels, out.labels + n, (int64_t)-1);
    if (out.scc_off) out.scc_off[0] = 0;
}

// host edge lists -> packed words (endpoints checked)
void pack_host(const int64_t *src, const int64_t *dst, int64_t cnt, int64_t n, std::vector<u64> &to, const char *what) {
    if (cnt > 0 && (!src || !dst)) throw_jh(JH_EINVAL, std::string(what) + ": null edge list");
    for (int64_t i = 0; i < cnt; i++) {
        if (src[i] < 0 || src[i] >= n || dst[i] < 0 || dst[i] >= n)
            throw_jh(JH_EINVAL, std::string(what) + ": an edge endpoint outside [0, n)");
        to.push_back(((u64)src[i] << 32) | (u64)dst[i]);
    }
}

// regions, SCCs and outputs of the E packed device edges over n vertices
void scc_core(jh_ctx *ctx, int64_t n, const u64 *edges, long long E, int path, jh_cycle_result *res, const CycleOut &out,
              YMeta *m, hipStream_t st) {
    const int g = grid_for(n, 256, 2048), ge = grid_for(E, 256, 4096);
    if (out.edges && out.edge_cap > 0 && E > 0) {
        const long long k = std::min<long long>(E, out.edge_cap);
        std::vector<u64> h(k);
        HIP_TRY(hipMemcpyAsync(h.data(), edges, sizeof(u64) * k, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (long long i = 0; i < k; i++) { out.edges[2 * i] = (int64_t)(h[i] >> 32); out.edges[2 * i + 1] = (int64_t)(uint32_t)h[i]; }
    }
    // 2. regions
    int32_t *reach = ctx->ws<int32_t>(WS_CY_REACH, 3 * n), *mx = reach + n, *big = reach + 2 * n;
    int32_t *bs = ctx->ws<int32_t>(WS_CY_BS, n);
    k_cy_iota<<<g, 256, 0, st>>>(reach, n);
    if (E > 0) k_cy_reach<<<ge, 256, 0, st>>>(edges, E, reach, m);
    incl_scan(ctx, WS_CY_TMP, reach, mx, hipcub::Max(), (int)n, st);
    k_cy_starts<<<g, 256, 0, st>>>(reach, mx, n, big);
    incl_sum(ctx, WS_CY_TMP, big, bs, (int)n, st);
    const int64_t NR = fetch(bs + (n - 1), st);
    res->regions = NR;
    if (NR == 0) {
        res->back_edges = (int64_t)fetch(m, st).back;
        empty_outputs(n, out);
        return;
    }
    int32_t *rstart = ctx->ws<int32_t>(WS_CY_REG, 2 * NR), *rend = rstart + NR;
    k_cy_bounds<<<g, 256, 0, st>>>(mx, big, bs, n, rstart, rend);
    k_cy_region_stats<<<grid_for(NR, 256, 1024), 256, 0, st>>>(rstart, rend, NR, path == 2, m);
    YMeta mh = fetch(m, st);
    res->back_edges = (int64_t)mh.back;
    res->max_region = (int64_t)mh.max_region;
    res->global_regions = (int64_t)mh.global_regions;
    if (path == 1 && mh.global_regions > 0)
        throw_jh(JH_EINVAL, "cycle on-chip path: a region of more than JH_CY_LDS_VERTICES vertices");
    res->path = mh.global_regions > 0 ? 2 : 1;

    // the regions' edges, by source and by destination
    u64 *fraw = ctx->ws<u64>(WS_CY_FWD, 2 * E), *fwd = fraw + E;
    k_cy_intra<<<ge, 256, 0, st>>>(edges, E, bs, rend, fraw);
    const long long EI = select_edges(ctx, fraw, fwd, E, st);
    u64 *bwd = ctx->ws<u64>(WS_CY_BWD, 2 * EI), *bwd_s = bwd + EI;
    int32_t *foff = ctx->ws<int32_t>(WS_CY_CSR, 2 * (n + 1)), *boff = foff + n + 1;
    const int eb = 32 + bits_of((u64)n);
    const u64 *fwd_s = fwd;
    if (EI > 0) {
        k_cy_swap<<<grid_for(EI, 256, 4096), 256, 0, st>>>(fwd, EI, bwd);
        sort_keys(ctx, WS_CY_TMP, fwd, fraw, (int)EI, eb, st);
        fwd_s = fraw;
        sort_keys(ctx, WS_CY_TMP, bwd, bwd_s, (int)EI, eb, st);
    }
    k_cy_csr<<<g, 256, 0, st>>>(fwd_s, EI, n, foff);
    k_cy_csr<<<g, 256, 0, st>>>(bwd_s, EI, n, boff);

    // 3. the regions
    int32_t *labels = ctx->ws<int32_t>(WS_CY_LABEL, n), *sccsize = ctx->ws<int32_t>(WS_CY_SIZE, n);
    k_cy_fill32<<<g, 256, 0, st>>>(labels, n, -1);
    HIP_TRY(hipMemsetAsync(sccsize, 0, sizeof(int32_t) * n, st));
    const int64_t n_lds = NR - (int64_t)mh.global_regions;
    if (n_lds > 0)
        k_cy_region<true><<<grid_for(NR, 1, 4096), RT, 0, st>>>(rstart, rend, (int)NR, foff, fwd_s, boff, bwd_s, path == 2,
                                                                 nullptr, n, labels, sccsize, m);
    if (mh.global_regions > 0) {
        int *state = ctx->ws<int>(WS_CY_STATE, 4 * n);
        k_cy_region<false><<<grid_for(NR, 1, 1024), RT, 0, st>>>(rstart, rend, (int)NR, foff, fwd_s, boff, bwd_s, path == 2,
                                                                  state, n, labels, sccsize, m);
    }

    // 4. results
    u64 *keys = ctx->ws<u64>(WS_CY_KEYS, 2 * n), *keys_s = keys + n;
    k_cy_keys<true><<<g, 256, 0, st>>>(labels, sccsize, n, keys, m);
    mh = fetch(m, st);
    if (mh.over_work) throw_jh(JH_EUNSUPPORTED, "cycle: a region past the work cap JH_CY_WORK_MULT * (vertices + edges)");
    res->scc_count = (int64_t)mh.scc_count;
    res->scc_vertices = (int64_t)mh.scc_vertices;
    res->valid = mh.scc_count ? JH_INVALID : JH_VALID;
    if (out.labels) {
        std::vector<int32_t> h(n);
        HIP_TRY(hipMemcpyAsync(h.data(), labels, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int64_t i = 0; i < n; i++) out.labels[i] = h[i];
    }
    if (out.scc_off) out.scc_off[0] = 0;
    const long long S = (long long)mh.scc_count;
    const long long n_list = out.scc_off ? std::min<long long>(S, std::max<int64_t>(out.scc_cap, 0)) : 0;
    if (n_list == 0) return;
    const long long got = select_edges(ctx, keys, keys_s, n, st);          // the roots' keys
    if (got != S) throw_jh(JH_EDEVICE, "cycle: SCC roots and counts disagree");
    sort_keys(ctx, WS_CY_TMP, keys_s, keys, (int)S, eb, st);
    std::vector<u64> hk(n_list);
    HIP_TRY(hipMemcpyAsync(hk.data(), keys, sizeof(u64) * n_list, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    long long total = 0;
    for (long long i = 0; i < n_list; i++) { total += (long long)(hk[i] >> 32); out.scc_off[i + 1] = total; }
    const long long n_rows = out.scc_rows ? std::min<long long>(total, std::max<int64_t>(out.rows_cap, 0)) : 0;
    if (n_rows == 0) return;
    // the member rows: selected in row order, then sorted (stably) on their SCC's key
    const long long NV = (long long)mh.scc_vertices;
    k_cy_keys<false><<<g, 256, 0, st>>>(labels, sccsize, n, keys, m);
    int32_t *rows = ctx->ws<int32_t>(WS_CY_VALS, 3 * n), *rows_m = rows + n, *rows_s = rows + 2 * n;
    k_cy_iota<<<g, 256, 0, st>>>(rows, n);
    long long *d_n = ctx->ws<long long>(WS_CY_SEL, 1);
    select_if(ctx, WS_CY_TMP, rows, rows_m, d_n, (int)n, Flag64{keys}, st);
    if (select_edges(ctx, keys, keys_s, n, st) != NV) throw_jh(JH_EDEVICE, "cycle: SCC members and counts disagree");
    sort_pairs(ctx, WS_CY_TMP, keys_s, keys, rows_m, rows_s, (int)NV, eb, st);
    std::vector<int32_t> hr(n_rows);
    HIP_TRY(hipMemcpyAsync(hr.data(), rows_s, sizeof(int32_t) * n_rows, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (long long i = 0; i < n_rows; i++) out.scc_rows[i] = hr[i];
}


}  // namespace

void scc_check(jh_ctx *ctx, int64_t n, const int64_t *src, const int64_t *dst, int64_t n_edges, const jh_cycle_opts *opts,
               jh_cycle_result *res, const CycleOut &out, hipStream_t st) {
    init_result(res);
    if (n > Y_MAX || n_edges > Y_MAX) throw_jh(JH_EUNSUPPORTED, "scc: more than 2^31 - 2 vertices or edges");
    std::vector<u64> h;
    h.reserve((size_t)n_edges);
    pack_host(src, dst, n_edges, n, h, "scc");
    res->edge_count[3] = n_edges;
    empty_outputs(n, out);
    if (n == 0) return;
    DeviceTimer timer{ctx, st};
    timer.start();
    YMeta *m = ctx->ws<YMeta>(WS_CY_META, 1);
    k_cy_meta_init<<<1, 1, 0, st>>>(m);
    u64 *edges = ctx->ws<u64>(WS_CY_EDGES, n_edges);
    if (n_edges > 0) HIP_TRY(hipMemcpyAsync(edges, h.data(), sizeof(u64) * n_edges, hipMemcpyHostToDevice, st));
    scc_core(ctx, n, edges, n_edges, opts->path, res, out, m, st);
    res->device_ms = timer.stop();
}

void cycle_check(jh_ctx *ctx, const jh_history *dh, const jh_cycle_opts *opts, jh_cycle_result *res, const CycleOut &out,
                 hipStream_t st) {
    init_result(res);
    const int64_t n = dh->n;
    const int an = opts->analyzers;
    if (n > Y_MAX || opts->n_extra > Y_MAX) throw_jh(JH_EUNSUPPORTED, "cycle: more than 2^31 - 2 vertices or edges");
    std::vector<u64> extra;
    pack_host(opts->extra_src, opts->extra_dst, opts->n_extra, n, extra, "cycle");
    res->edge_count[3] = opts->n_extra;
    empty_outputs(n, out);
    if (n == 0) return;
    DeviceTimer timer{ctx, st};
    timer.start();
    YMeta *m = ctx->ws<YMeta>(WS_CY_META, 1);
    k_cy_meta_init<<<1, 1, 0, st>>>(m);
    const int g = grid_for(n + 1, 256, 2048);
    const bool pairs = (an & (JH_CY_PROCESS | JH_CY_REALTIME)) != 0;

    // rows; the txns' external reads and writes, counted
    int64_t *pkey = pairs ? ctx->ws<int64_t>(WS_CY_PKEY, 2 * n) : nullptr, *pkey_s = pairs ? pkey + n : nullptr;
    int32_t *prow = pairs ? ctx->ws<int32_t>(WS_CY_PROW, 2 * n) : nullptr, *prow_s = pairs ? prow + n : nullptr;
    int32_t *comp = pairs ? ctx->ws<int32_t>(WS_CY_COMP, n) : nullptr;
    k_cy_rows<<<g, 256, 0, st>>>(dh->process, dh->type, n, pkey, prow, comp, m);
    long long *cr = nullptr, *cw = nullptr, *ro = nullptr, *wo = nullptr;
    if (an & JH_CY_WR) {
        cr = ctx->ws<long long>(WS_CY_TXN, 4 * (n + 1));
        cw = cr + (n + 1); ro = cr + 2 * (n + 1); wo = cr + 3 * (n + 1);
        k_cy_txn<false><<<g, 256, 0, st>>>(dh->process, dh->type, dh->value, dh->value2, dh->aux, n, dh->n_aux / 3, cr, cw,
                                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, m);
        excl_sum(ctx, WS_CY_TMP, as_input(cr), ro, (int)(n + 1), st);
        excl_sum(ctx, WS_CY_TMP, as_input(cw), wo, (int)(n + 1), st);
    }
    YMeta mh = fetch(m, st);
    if (mh.bad_type) throw_jh(JH_EINVAL, "cycle: a :type outside 0..3");
    if (mh.bad_range) throw_jh(JH_EINVAL, "cycle: a txn's range leaves [0, n_aux / 3) or has a negative count");
    if (mh.unsup_mops) throw_jh(JH_EUNSUPPORTED, "cycle: a txn of more than JH_CY_MAX_MOPS micro-ops");
    if (mh.unsup_f) throw_jh(JH_EUNSUPPORTED, "cycle: a micro-op that is neither a read nor a write");
    res->entries = (int64_t)mh.entries;
    auto unknown = [&](int cause, u64 row) {
        res->valid = JH_UNKNOWN; res->cause = cause; res->unknown_row = (int64_t)row;
        res->device_ms = timer.stop();
    };

    // pairs, process edges, realtime edge counts
    long long n_rt = 0;
    int32_t *ip = nullptr, *icomp = nullptr;
    long long *rt_off = nullptr;
    const long long n_proc_slots = (an & JH_CY_PROCESS) ? n : 0;
    u64 *proc_raw = nullptr;
    if (pairs) {
        sort_pairs(ctx, WS_CY_TMP, pkey, pkey_s, prow, prow_s, (int)n, 64, st);
        // (process slots live in their own buffer until the total is known)
        proc_raw = ctx->ws<u64>(WS_CY_KEYS, n);
        k_cy_pair<<<g, 256, 0, st>>>(pkey_s, prow_s, dh->type, n, (an & JH_CY_PROCESS) ? 1 : 0, comp, proc_raw, m);
    }
    if (an & JH_CY_REALTIME) {
        int32_t *rev = ctx->ws<int32_t>(WS_CY_REV, 2 * n), *sufmin = rev + n;
        ip = ctx->ws<int32_t>(WS_CY_IP, 2 * (n + 1));
        int32_t *isinv = ip + (n + 1);
        k_cy_rt_key<<<g, 256, 0, st>>>(dh->process, dh->type, comp, n, rev, isinv, m);
        mh = fetch(m, st);
        if (mh.dbl_row != NONE) return unknown(JH_CAUSE_DOUBLE_INVOKE, mh.dbl_row);
        if (mh.orphan_row != NONE) return unknown(JH_CAUSE_ORPHAN, mh.orphan_row);
        if (mh.unmatched_row != NONE) return unknown(JH_CAUSE_UNMATCHED_INVOKE, mh.unmatched_row);
        excl_scan(ctx, WS_CY_TMP, rev, sufmin, hipcub::Min(), (int32_t)n, (int)n, st);
        excl_sum(ctx, WS_CY_TMP, as_input(isinv), ip, (int)(n + 1), st);
        int32_t n_inv = 0;
        HIP_TRY(hipMemcpyAsync(&n_inv, ip + n, sizeof n_inv, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        icomp = ctx->ws<int32_t>(WS_CY_ICOMP, n_inv);
        long long *cnt = ctx->ws<long long>(WS_CY_CNT, 2 * (n + 1));
        rt_off = cnt + (n + 1);
        k_cy_rt_count<<<g, 256, 0, st>>>(dh->process, dh->type, comp, sufmin, ip, n, cnt, icomp);
        excl_sum(ctx, WS_CY_TMP, as_input(cnt), rt_off, (int)(n + 1), st);
        HIP_TRY(hipMemcpyAsync(&n_rt, rt_off + n, sizeof n_rt, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    // appends-and-reads: the verification passes and the number of its slots (jh_cycle_append.hip)
    AppendPlan ap;
    if (an & JH_CY_APPEND) {
        ap = append_plan(ctx, dh, res, st);
        if (ap.cause) { res->device_ms = timer.stop(); return; }
    }
    // monotonic-key: the sorted records and the number of its edges (jh_cycle_mono.hip)
    MonoPlan mp;
    if (an & JH_CY_MONOTONIC) mp = mono_plan(ctx, dh, res, st);
    long long R = 0, W = 0;
    if (an & JH_CY_WR) {
        HIP_TRY(hipMemcpyAsync(&R, ro + n, sizeof R, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&W, wo + n, sizeof W, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    const long long n_raw = n_proc_slots + n_rt + R + ap.slots + mp.slots + (long long)extra.size();
    if (n_rt > Y_MAX || R > Y_MAX || W > Y_MAX || n_raw > Y_MAX)
        throw_jh(JH_EUNSUPPORTED, "cycle: more than 2^31 - 2 vertices or edges");

    // every builder's slots in one buffer: process | realtime | wr | append | monotonic | extra
    u64 *raw = ctx->ws<u64>(WS_CY_RAW, n_raw);
    u64 *raw_rt = raw + n_proc_slots, *raw_wr = raw_rt + n_rt, *raw_ap = raw_wr + R, *raw_mo = raw_ap + ap.slots;
    u64 *raw_x = raw_mo + mp.slots;
    const long long ap_links = (an & JH_CY_APPEND) ? append_fill(ctx, ap, raw_ap, st) : 0;
    mono_fill(ctx, mp, raw_mo, st);
    if (n_proc_slots) HIP_TRY(hipMemcpyAsync(raw, proc_raw, sizeof(u64) * n, hipMemcpyDeviceToDevice, st));
    if (n_rt > 0) k_cy_rt_fill<<<grid_for(n_rt, 256, 4096), 256, 0, st>>>(rt_off, ip, icomp, n, n_rt, raw_rt);
    if (R > 0) {
        int64_t *rk = ctx->ws<int64_t>(WS_CY_REC, 2 * (R + W)), *rv = rk + R, *wk = rv + R, *wv = wk + W;
        int32_t *rrow = ctx->ws<int32_t>(WS_CY_HIDX, R + 3 * W + 4), *wrow = rrow + R;
        uint32_t *widx = (uint32_t *)(wrow + W), *widx_s = widx + W;
        u64 *whash = ctx->ws<u64>(WS_CY_HASH, 2 * W + 2), *whash_s = whash + W;
        k_cy_txn<true><<<g, 256, 0, st>>>(dh->process, dh->type, dh->value, dh->value2, dh->aux, n, dh->n_aux / 3, ro, wo, rk,
                                          rv, rrow, wk, wv, wrow, whash, widx, m);
        if (W > 0) {
            sort_pairs(ctx, WS_CY_TMP, whash, whash_s, widx, widx_s, (int)W, 64, st);
        }
        k_cy_wr_join<<<grid_for(R, 256, 4096), 256, 0, st>>>(rk, rv, rrow, R, whash_s, widx_s, wk, wv, wrow, W, raw_wr, m);
        k_cy_wr_unknown<<<1, 1, 0, st>>>(ro, rk, rv, whash_s, widx_s, wk, wv, wrow, W, m);
    }
    if (!extra.empty())
        HIP_TRY(hipMemcpyAsync(raw_x, extra.data(), sizeof(u64) * extra.size(), hipMemcpyHostToDevice, st));
    mh = fetch(m, st);
    if (mh.multi_row != NONE) {
        res->unknown_key = mh.unknown_key; res->unknown_value = mh.unknown_value;
        res->unknown_rows[0] = mh.unknown_rows[0]; res->unknown_rows[1] = mh.unknown_rows[1];
        return unknown(JH_CAUSE_MULTIPLE_WRITES, mh.multi_row);
    }
    res->edge_count[0] = (int64_t)mh.edges[0];
    res->edge_count[1] = n_rt;
    res->edge_count[2] = (an & JH_CY_APPEND) ? ap_links : (an & JH_CY_MONOTONIC) ? mp.slots : (int64_t)mh.edges[2];
    u64 *edges = ctx->ws<u64>(WS_CY_EDGES, n_raw);
    const long long E = select_edges(ctx, raw, edges, n_raw, st);
    scc_core(ctx, n, edges, E, opts->path, res, out, m, st);
    res->device_ms = timer.stop();
}
