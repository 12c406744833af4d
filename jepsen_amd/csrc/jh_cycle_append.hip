// jh_cycle_append.hip -- appends-and-reads-graph of jepsen.tests.cycle on MI355X:
// the version order of every key from its longest read, the verification passes,
// and the wr / ww / rw edges over history rows.
//
// jepsen/src/jepsen/tests/cycle.clj:381-699. include/jh.h states the semantics
// ("JH_CY_APPEND", "Append txn encoding"); DESIGN.md §4j the design.
//
// A position (row, micro-op) is one word, row << 6 | micro-op (JH_CY_MAX_MOPS = 64):
// "first" in the reference's reduce-mops order is the smallest such word, and the
// read and append records are numbered in that order too.
//
//   1. k_ap_txn       a counting and a filling pass, one thread per row: validation,
//                     the read records (k, off, len, position, counted) and the
//                     append records (k, v, position, type, hash of (k, v)).
//   2. k_ap_best      best[k] = max over the counted reads of len << 32 | ~record:
//                     the longest read L_k, ties to the first one.
//   3. k_ap_compare   the hot kernel. Every counted read but L_k itself is cut into
//                     tiles of 64 elements; a wave takes a tile (a binary search in
//                     the tiles' exclusive sum finds its read), a lane one element
//                     of the read and the one of L_k at the same place, 8 B each,
//                     coalesced. A mismatch flags the read and feeds badrow[k].
//   4. k_ap_lrec      (k, L_k[j]) records, one thread per element, sorted (stably) on
//      k_ap_ldup      the hash of (k, v): d_k = the smallest j whose element stands
//                     earlier in L_k. A counted prefix read of length c holds a
//                     duplicate iff c > d_k. The sorted table is also the position
//                     index of step 7.
//      k_ap_rdup      the reads that need the direct check instead (not counted, or
//      k_ap_direct    not a prefix): one workgroup each, the elements in LDS.
//   5. k_ap_adup      the append records sorted (stably) on the hash of (k, v): an
//                     :invoke record with an earlier :invoke record of its (k, v).
//   6. writers        the same sorted records: the last :ok / :info record of (k, v).
//   7. k_ap_wr        one slot per read, one per append; the counted reads sorted by
//      k_ap_ww        (k, len) give every append at position i its run of readers;
//      k_ap_rw        an exclusive sum of the runs' lengths, one thread per rw edge.
#include "cycle_common.h"

namespace {
constexpr int DIRECT = JH_CY_AP_DIRECT_READ;
constexpr int MOP_BITS = 6;
static_assert(JH_CY_MAX_MOPS <= (1 << MOP_BITS), "a position holds the micro-op in 6 bits");
constexpr uint32_t NO_DUP = 0xffffffffu;

struct AMeta {
    unsigned bad_range, bad_key, nil_elem, unsup_f, unsup_mops, unsup_direct;
    u64 entries, links;
    u64 dup_append, dup_read, no_writer;            // smallest positions of causes 13, 14, 16
    u64 bad_keys, min_bad_key;                      // cause 15
    long long key, value;                           // k_ap_report
};

__global__ void k_ap_meta_init(AMeta *m) {
    memset(m, 0, sizeof *m);
    m->dup_append = m->dup_read = m->no_writer = m->min_bad_key = NONE;
    m->key = m->value = JH_NIL;
}

// every device array of one call (host struct, passed by value)
struct AP {
    const int64_t *process, *type, *value, *value2, *aux;
    int64_t n, n_aux, n_keys;
    long long R, A, NL;
    // rows: counts and exclusive sums of the reads and appends (n + 1 each)
    long long *cr, *ca, *ro, *ao;
    // keys
    u64 *best;
    long long *llen, *loff;
    uint32_t *dk, *badrow;
    // reads
    int32_t *rk, *rlen, *dlist;
    int64_t *roff;
    u64 *rpos, *skey, *skey_s;
    uint8_t *rcnt, *rflag, *need;
    uint32_t *sidx, *sidx_s;
    long long *tcnt, *toff, *d_n;
    // appends
    int32_t *ak;
    int64_t *av;
    u64 *apos, *ahash, *ahash_s;
    uint8_t *atype;
    uint32_t *aidx, *aidx_s;
    long long *rwcnt, *rwoff, *rwlo;
    u64 *slots;
    // the elements of every L_k, key after key
    int32_t *lk;
    int64_t *lv;
    u64 *lhash, *lhash_s;
    uint32_t *lidx, *lidx_s;
    AMeta *m;
};

__device__ __forceinline__ uint32_t longest_of(const AP &a, int64_t k) { return 0xffffffffu - (uint32_t)a.best[k]; }

// 1. ---------------------------------------------------------------------------
template <bool FILL>
__global__ void __launch_bounds__(256) k_ap_txn(const AP a) {
    __shared__ u64 sh[4];
    u64 ent = 0;
    CY_LOOP(i, a.n + 1) {
        long long nr = 0, na = 0;
        if (i < a.n && a.process[i] != -1) {
            long long s = a.value[i], c = a.value2[i];
            const int64_t t = a.type[i];
            if (c == 0) s = 0;                                // nil or empty: value is not looked at
            if (c < 0 || s < 0 || s > a.n_aux || c > (a.n_aux - s) / 4) { if (!FILL) atomicOr(&a.m->bad_range, 1u); c = 0; }
            else if (c > JH_CY_MAX_MOPS) { if (!FILL) atomicOr(&a.m->unsup_mops, 1u); c = 0; }
            const int64_t *w = a.aux + s;
            const long long r0 = FILL ? a.ro[i] : 0, a0 = FILL ? a.ao[i] : 0;
            ent += (u64)c;
            for (int j = 0; j < c; j++) {
                const int64_t f = w[4 * j], k = w[4 * j + 1], x = w[4 * j + 2], b = w[4 * j + 3];
                if (f != JH_F_READ && f != JH_F_APPEND) { if (!FILL) atomicOr(&a.m->unsup_f, 1u); continue; }
                if (k < 0 || k >= a.n_keys) { if (!FILL) atomicOr(&a.m->bad_key, 1u); continue; }
                const u64 pos = ((u64)i << MOP_BITS) | (u64)j;
                if (f == JH_F_READ) {
                    if (b < 0 || b > Y_MAX || (b > 0 && (x < 0 || x > a.n_aux || b > a.n_aux - x))) {
                        if (!FILL) atomicOr(&a.m->bad_range, 1u);
                        continue;
                    }
                    ent += (u64)b;
                    if (FILL) {
                        const long long q = r0 + nr;
                        a.rk[q] = (int32_t)k; a.roff[q] = b ? x : 0; a.rlen[q] = (int32_t)b; a.rpos[q] = pos;
                        a.rcnt[q] = (t == T_OK || t == T_INFO) ? 1 : 0; a.rflag[q] = 0;
                    }
                    nr++;
                } else {
                    if (x == JH_NIL) { if (!FILL) atomicOr(&a.m->nil_elem, 1u); continue; }
                    if (FILL) {
                        const long long q = a0 + na;
                        a.ak[q] = (int32_t)k; a.av[q] = x; a.apos[q] = pos; a.atype[q] = (uint8_t)t;
                        a.ahash[q] = cy_hash(k, x); a.aidx[q] = (uint32_t)q;
                    }
                    na++;
                }
            }
        }
        if (!FILL) { a.cr[i] = nr; a.ca[i] = na; }
    }
    if (!FILL) {
        ent = block_reduce256(ent, RedSum(), sh);
        if (threadIdx.x == 0 && ent) atomicAdd(&a.m->entries, ent);
    }
}

// 2. ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ap_key_init(const AP a) {
    CY_LOOP(k, a.n_keys) { a.best[k] = 0; a.dk[k] = NO_DUP; a.badrow[k] = 0xffffffffu; }
}

__global__ void __launch_bounds__(256) k_ap_best(const AP a) {
    CY_LOOP(i, a.R)
        if (a.rcnt[i]) atomicMax(&a.best[a.rk[i]], ((u64)(uint32_t)a.rlen[i] << 32) | (u64)(0xffffffffu - (uint32_t)i));
}

// llen[k] = |L_k| (0 for a key no counted read names; llen[n_keys] = 0)
__global__ void __launch_bounds__(256) k_ap_llen(const AP a) {
    CY_LOOP(k, a.n_keys + 1) a.llen[k] = k < a.n_keys ? (long long)(a.best[k] >> 32) : 0;
}

// the tiles of every counted read that is not its key's L_k
__global__ void __launch_bounds__(256) k_ap_tiles(const AP a) {
    CY_LOOP(i, a.R + 1) {
        long long t = 0;
        if (i < a.R && a.rcnt[i] && a.rlen[i] > 0 && longest_of(a, a.rk[i]) != (uint32_t)i) t = ((long long)a.rlen[i] + 63) >> 6;
        a.tcnt[i] = t;
    }
}

// 3. ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ap_compare(const AP a) {
    const long long T = a.toff[a.R];
    const int lane = threadIdx.x & 63;
    const long long nw = (long long)gridDim.x * 4;
    for (long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += nw) {
        const long long i = cy_owner(a.toff, a.R, t);       // the same for the whole wave
        const int32_t k = a.rk[i];
        const long long e = ((t - a.toff[i]) << 6) + lane;
        bool bad = false, nil = false;
        if (e < a.rlen[i]) {                                 // rlen[i] <= |L_k|: both loads are inside their reads
            const int64_t x = a.aux[a.roff[i] + e], y = a.aux[a.roff[longest_of(a, k)] + e];
            bad = x != y;
            nil = x == JH_NIL;
        }
        const bool any_bad = __ballot(bad) != 0, any_nil = __ballot(nil) != 0;
        if (lane == 0 && any_bad) { a.rflag[i] = 1; atomicMin(&a.badrow[k], (uint32_t)(a.rpos[i] >> MOP_BITS)); }
        if (lane == 0 && any_nil) atomicOr(&a.m->nil_elem, 1u);
    }
}

// 4. ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ap_lrec(const AP a) {
    CY_LOOP(g, a.NL) {
        const long long k = cy_owner(a.loff, a.n_keys, g);
        const int64_t v = a.aux[a.roff[longest_of(a, k)] + (g - a.loff[k])];
        if (v == JH_NIL) atomicOr(&a.m->nil_elem, 1u);
        a.lk[g] = (int32_t)k; a.lv[g] = v; a.lhash[g] = cy_hash(k, v); a.lidx[g] = (uint32_t)g;
    }
}

// over the sorted elements: one with an equal (k, v) before it in its hash run stands later in L_k
__global__ void __launch_bounds__(256) k_ap_ldup(const AP a) {
    CY_LOOP(p, a.NL) {
        const uint32_t g = a.lidx_s[p];
        const u64 h = a.lhash_s[p];
        const int32_t k = a.lk[g];
        const int64_t v = a.lv[g];
        for (long long q = p - 1; q >= 0 && a.lhash_s[q] == h; q--) {
            const uint32_t g2 = a.lidx_s[q];
            if (a.lk[g2] == k && a.lv[g2] == v) { atomicMin(&a.dk[k], (uint32_t)(g - a.loff[k])); break; }
        }
    }
}

// the position of v in L_k (the first one), -1 when it is not there
__device__ __forceinline__ long long ap_pos(const AP &a, int64_t k, int64_t v) {
    const u64 h = cy_hash(k, v);
    for (long long p = cy_lower(a.lhash_s, a.NL, h); p < a.NL && a.lhash_s[p] == h; p++) {
        const uint32_t g = a.lidx_s[p];
        if (a.lk[g] == k && a.lv[g] == v) return (long long)g - a.loff[k];
    }
    return -1;
}

__global__ void __launch_bounds__(256) k_ap_rdup(const AP a) {
    __shared__ u64 sh[4];
    u64 first = NONE;
    CY_LOOP(i, a.R) {
        const int32_t len = a.rlen[i];
        uint8_t need = 0;
        if (len > 0) {
            if (a.rcnt[i] && !a.rflag[i]) { if ((u64)len > (u64)a.dk[a.rk[i]]) first = min(first, a.rpos[i]); }
            else if (len > DIRECT) atomicOr(&a.m->unsup_direct, 1u);
            else need = 1;
        }
        a.need[i] = need;
    }
    first = block_reduce256(first, RedMin(), sh);
    if (threadIdx.x == 0 && first != NONE) atomicMin(&a.m->dup_read, first);
}

// the smallest j < len with sv[j] == sv[i] for some i < j (len: none); s_min is shared
__device__ __forceinline__ int ap_first_dup(const int64_t *sv, int len, int *s_min) {
    if (threadIdx.x == 0) *s_min = len;
    __syncthreads();
    for (int j = threadIdx.x; j < len; j += blockDim.x) {
        if (j >= *s_min) break;
        const int64_t v = sv[j];
        for (int q = 0; q < j; q++)
            if (sv[q] == v) { atomicMin(s_min, j); break; }
    }
    __syncthreads();
    const int got = *s_min;
    __syncthreads();
    return got;
}

__global__ void __launch_bounds__(256) k_ap_direct(const AP a) {
    __shared__ int64_t sv[DIRECT];
    __shared__ int s_min;
    const long long cnt = *a.d_n;
    for (long long x = blockIdx.x; x < cnt; x += gridDim.x) {
        const int32_t i = a.dlist[x];
        const int len = a.rlen[i];                            // <= DIRECT (k_ap_rdup)
        bool nil = false;
        for (int j = threadIdx.x; j < len; j += blockDim.x) { sv[j] = a.aux[a.roff[i] + j]; nil |= sv[j] == JH_NIL; }
        if (nil) atomicOr(&a.m->nil_elem, 1u);
        __syncthreads();
        if (ap_first_dup(sv, len, &s_min) < len && threadIdx.x == 0) atomicMin(&a.m->dup_read, a.rpos[i]);
    }
}

// 5. ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ap_adup(const AP a) {
    __shared__ u64 sh[4];
    u64 first = NONE;
    CY_LOOP(p, a.A) {
        const uint32_t x = a.aidx_s[p];
        if (a.atype[x] != T_INVOKE) continue;
        const u64 h = a.ahash_s[p];
        for (long long q = p - 1; q >= 0 && a.ahash_s[q] == h; q--) {
            const uint32_t y = a.aidx_s[q];
            if (a.atype[y] == T_INVOKE && a.ak[y] == a.ak[x] && a.av[y] == a.av[x]) { first = min(first, a.apos[x]); break; }
        }
    }
    first = block_reduce256(first, RedMin(), sh);
    if (threadIdx.x == 0 && first != NONE) atomicMin(&a.m->dup_append, first);
}

__global__ void __launch_bounds__(256) k_ap_badkeys(const AP a) {
    __shared__ u64 sh[4];
    u64 cnt = 0, first = NONE;
    CY_LOOP(k, a.n_keys)
        if (a.badrow[k] != 0xffffffffu) { cnt++; first = min(first, (u64)k); }
    cnt = block_reduce256(cnt, RedSum(), sh);
    first = block_reduce256(first, RedMin(), sh);
    if (threadIdx.x == 0 && cnt) { atomicAdd(&a.m->bad_keys, cnt); atomicMin(&a.m->min_bad_key, first); }
}

// 6. the writer of (k, v): the row of its last :ok / :info record (the sort is stable), -1: none
__device__ __forceinline__ long long ap_writer(const AP &a, int64_t k, int64_t v) {
    const u64 h = cy_hash(k, v);
    long long w = -1;
    for (long long p = cy_lower(a.ahash_s, a.A, h); p < a.A && a.ahash_s[p] == h; p++) {
        const uint32_t x = a.aidx_s[p];
        if ((a.atype[x] == T_OK || a.atype[x] == T_INFO) && a.ak[x] == k && a.av[x] == v) w = (long long)(a.apos[x] >> MOP_BITS);
    }
    return w;
}

// 7. ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ap_skey(const AP a) {
    CY_LOOP(i, a.R) {
        a.skey[i] = a.rcnt[i] ? ((u64)(uint32_t)a.rk[i] << 32) | (u64)(uint32_t)a.rlen[i] : ~0ULL;
        a.sidx[i] = (uint32_t)i;
    }
}

__global__ void __launch_bounds__(256) k_ap_wr(const AP a) {
    __shared__ u64 sh[4];
    u64 links = 0, missing = NONE;
    CY_LOOP(i, a.R) {
        u64 e = HOLE;
        if (a.rcnt[i] && a.rlen[i] > 0) {
            const long long row = (long long)(a.rpos[i] >> MOP_BITS);
            const long long w = ap_writer(a, a.rk[i], a.aux[a.roff[i] + a.rlen[i] - 1]);
            if (w < 0) missing = min(missing, a.rpos[i]);
            else if (w != row) { e = pack(w, row); links++; }
        }
        a.slots[i] = e;
    }
    links = block_reduce256(links, RedSum(), sh);
    missing = block_reduce256(missing, RedMin(), sh);
    if (threadIdx.x == 0 && links) atomicAdd(&a.m->links, links);
    if (threadIdx.x == 0 && missing != NONE) atomicMin(&a.m->no_writer, missing);
}

__global__ void __launch_bounds__(256) k_ap_ww(const AP a) {
    __shared__ u64 sh[4];
    u64 links = 0, missing = NONE;
    CY_LOOP(x, a.A + 1) {
        u64 e = HOLE;
        long long cnt = 0, lo = 0;
        if (x < a.A && (a.atype[x] == T_OK || a.atype[x] == T_INFO)) {
            const int64_t k = a.ak[x];
            const long long row = (long long)(a.apos[x] >> MOP_BITS), j = ap_pos(a, k, a.av[x]);
            if (j > 0) {
                const long long w = ap_writer(a, k, a.lv[a.loff[k] + j - 1]);
                if (w < 0) missing = min(missing, a.apos[x]);
                else if (w != row) { e = pack(w, row); links++; }
            }
            if (j >= 0) {                                    // the counted reads of k of length j
                const u64 key = ((u64)(uint32_t)k << 32) | (u64)j;
                lo = cy_lower(a.skey_s, a.R, key);
                cnt = cy_lower(a.skey_s, a.R, key + 1) - lo;
            }
        }
        if (x < a.A) { a.slots[a.R + x] = e; a.rwlo[x] = lo; }
        a.rwcnt[x] = cnt;
    }
    links = block_reduce256(links, RedSum(), sh);
    missing = block_reduce256(missing, RedMin(), sh);
    if (threadIdx.x == 0 && links) atomicAdd(&a.m->links, links);
    if (threadIdx.x == 0 && missing != NONE) atomicMin(&a.m->no_writer, missing);
}

__global__ void __launch_bounds__(256) k_ap_rw(const AP a, long long total, u64 *__restrict__ raw) {
    __shared__ u64 sh[4];
    u64 links = 0;
    CY_LOOP(e, total) {
        const long long x = cy_owner(a.rwoff, a.A, e);
        const uint32_t reader = a.sidx_s[a.rwlo[x] + (e - a.rwoff[x])];
        const long long r = (long long)(a.rpos[reader] >> MOP_BITS), w = (long long)(a.apos[x] >> MOP_BITS);
        u64 word = HOLE;
        if (r != w) { word = pack(r, w); links++; }
        raw[e] = word;
    }
    links = block_reduce256(links, RedSum(), sh);
    if (threadIdx.x == 0 && links) atomicAdd(&a.m->links, links);
}

// key and value of cause 13, 14 or 16 at the position the cause's word names (one workgroup)
__global__ void __launch_bounds__(256) k_ap_report(const AP a, int cause) {
    __shared__ int64_t sv[DIRECT];
    __shared__ int s_min;
    const u64 pos = cause == JH_CAUSE_DUPLICATE_APPENDS ? a.m->dup_append
                    : cause == JH_CAUSE_DUPLICATE_ELEMENTS ? a.m->dup_read : a.m->no_writer;
    const long long row = (long long)(pos >> MOP_BITS);
    const int mop = (int)(pos & ((1 << MOP_BITS) - 1));
    const int64_t *w = a.aux + a.value[row];
    const int64_t f = w[4 * mop], k = w[4 * mop + 1], x = w[4 * mop + 2], b = w[4 * mop + 3];
    long long value = JH_NIL;
    if (cause == JH_CAUSE_DUPLICATE_APPENDS) {
        value = x;
    } else if (cause == JH_CAUSE_DUPLICATE_ELEMENTS) {
        long long i = a.ro[row];                             // this read's record
        for (int j = 0; j < mop; j++) i += w[4 * j] == JH_F_READ;
        if (a.rcnt[i] && !a.rflag[i]) {
            value = a.lv[a.loff[k] + a.dk[k]];
        } else {                                             // a direct read: b <= DIRECT
            for (int j = threadIdx.x; j < b; j += blockDim.x) sv[j] = a.aux[x + j];
            __syncthreads();
            value = sv[ap_first_dup(sv, (int)b, &s_min)];
        }
    } else if (f == JH_F_READ) {
        value = a.aux[x + b - 1];
    } else {
        value = a.lv[a.loff[k] + ap_pos(a, k, x) - 1];
    }
    if (threadIdx.x == 0) { a.m->key = k; a.m->value = value; }
}

void finish(jh_cycle_result *res, int valid, int cause, long long row, long long r0, long long key, long long value) {
    res->valid = valid; res->cause = cause; res->unknown_row = row;
    res->unknown_rows[0] = r0; res->unknown_rows[1] = -1;
    res->unknown_key = key; res->unknown_value = value;
}
}  // namespace

AppendPlan append_plan(jh_ctx *ctx, const jh_history *dh, jh_cycle_result *res, hipStream_t st) {
    AppendPlan plan;
    AP a = {};
    a.process = dh->process; a.type = dh->type; a.value = dh->value; a.value2 = dh->value2; a.aux = dh->aux;
    a.n = dh->n; a.n_aux = dh->n_aux; a.n_keys = dh->n_keys;
    const int64_t n = a.n, K = a.n_keys;
    if (K > Y_MAX) throw_jh(JH_EUNSUPPORTED, "cycle: more than 2^31 - 2 keys");
    a.m = ctx->ws<AMeta>(WS_CY_AP_META, 1);
    k_ap_meta_init<<<1, 1, 0, st>>>(a.m);
    carve(ctx, WS_CY_AP_ROWS, [&](Arena &r) {
        r.take(a.cr, n + 1); r.take(a.ca, n + 1); r.take(a.ro, n + 1); r.take(a.ao, n + 1);
        r.take(a.best, K); r.take(a.llen, K + 1); r.take(a.loff, K + 1); r.take(a.dk, K); r.take(a.badrow, K);
        r.take(a.d_n, 1);
    });
    const int g = grid_for(n + 1, 256, 2048), gk = grid_for(K + 1, 256, 2048);

    // 1. records
    k_ap_txn<false><<<g, 256, 0, st>>>(a);
    excl_sum(ctx, WS_CY_TMP, as_input(a.cr), a.ro, (int)(n + 1), st);
    excl_sum(ctx, WS_CY_TMP, as_input(a.ca), a.ao, (int)(n + 1), st);
    HIP_TRY(hipMemcpyAsync(&a.R, a.ro + n, sizeof a.R, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&a.A, a.ao + n, sizeof a.A, hipMemcpyDeviceToHost, st));
    AMeta mh = fetch(a.m, st);
    auto refuse = [&](const AMeta &h) {
        if (h.bad_range) throw_jh(JH_EINVAL, "cycle: a txn's or a read's range leaves [0, n_aux) or has a negative count");
        if (h.bad_key) throw_jh(JH_EINVAL, "cycle: a micro-op's key outside [0, n_keys)");
        if (h.nil_elem) throw_jh(JH_EINVAL, "cycle: an element equal to JH_NIL");
        if (h.unsup_mops) throw_jh(JH_EUNSUPPORTED, "cycle: a txn of more than JH_CY_MAX_MOPS micro-ops");
        if (h.unsup_f) throw_jh(JH_EUNSUPPORTED, "cycle: a micro-op that is neither a read nor an append");
        if (h.unsup_direct) throw_jh(JH_EUNSUPPORTED, "cycle: a read past JH_CY_AP_DIRECT_READ elements needs the direct duplicate check");
    };
    refuse(mh);
    res->entries = (int64_t)mh.entries;
    const long long R = a.R, A = a.A;
    if (R > Y_MAX || A > Y_MAX || R + A > Y_MAX) throw_jh(JH_EUNSUPPORTED, "cycle: more than 2^31 - 2 records");
    carve(ctx, WS_CY_AP_RECS, [&](Arena &r) {
        r.take(a.roff, R); r.take(a.rpos, R); r.take(a.skey, R); r.take(a.skey_s, R); r.take(a.tcnt, R + 1); r.take(a.toff, R + 1);
        r.take(a.rk, R); r.take(a.rlen, R); r.take(a.dlist, R); r.take(a.sidx, R); r.take(a.sidx_s, R);
        r.take(a.rcnt, R); r.take(a.rflag, R); r.take(a.need, R);
        r.take(a.av, A); r.take(a.apos, A); r.take(a.ahash, A); r.take(a.ahash_s, A);
        r.take(a.rwcnt, A + 1); r.take(a.rwoff, A + 1); r.take(a.rwlo, A);
        r.take(a.ak, A); r.take(a.aidx, A); r.take(a.aidx_s, A); r.take(a.atype, A);
        r.take(a.slots, R + A);
    });
    const int gr = grid_for(R + 1, 256, 4096), ga = grid_for(A + 1, 256, 4096);
    k_ap_key_init<<<gk, 256, 0, st>>>(a);
    k_ap_txn<true><<<g, 256, 0, st>>>(a);

    // 2. the longest read of every key; the tiles of the others
    if (R > 0) k_ap_best<<<gr, 256, 0, st>>>(a);
    k_ap_llen<<<gk, 256, 0, st>>>(a);
    excl_sum(ctx, WS_CY_TMP, as_input(a.llen), a.loff, (int)(K + 1), st);
    k_ap_tiles<<<gr, 256, 0, st>>>(a);
    excl_sum(ctx, WS_CY_TMP, as_input(a.tcnt), a.toff, (int)(R + 1), st);
    long long T = 0;
    HIP_TRY(hipMemcpyAsync(&T, a.toff + R, sizeof T, hipMemcpyDeviceToHost, st));
    a.NL = fetch(a.loff + K, st);
    if (a.NL > Y_MAX) throw_jh(JH_EUNSUPPORTED, "cycle: more than 2^31 - 2 records");
    const long long NL = a.NL;
    carve(ctx, WS_CY_AP_LONGEST, [&](Arena &r) {
        r.take(a.lv, NL); r.take(a.lhash, NL); r.take(a.lhash_s, NL); r.take(a.lk, NL); r.take(a.lidx, NL); r.take(a.lidx_s, NL);
    });

    // 3. the prefix compare
    if (T > 0) k_ap_compare<<<grid_for(T, 4, 16384), 256, 0, st>>>(a);

    // 4. positions and duplicates of every L_k; the reads' duplicates
    if (NL > 0) {
        k_ap_lrec<<<grid_for(NL, 256, 4096), 256, 0, st>>>(a);
        sort_pairs(ctx, WS_CY_TMP, a.lhash, a.lhash_s, a.lidx, a.lidx_s, (int)NL, 64, st);
        k_ap_ldup<<<grid_for(NL, 256, 4096), 256, 0, st>>>(a);
    }
    if (R > 0) {
        k_ap_rdup<<<gr, 256, 0, st>>>(a);
        select_flagged(ctx, WS_CY_TMP, hipcub::CountingInputIterator<int32_t>(0), a.need, a.dlist, a.d_n, (int)R, st);
        k_ap_direct<<<grid_for(R, 1, 1024), 256, 0, st>>>(a);
    }

    // 5. unique appends; the keys without a total order
    if (A > 0) {
        sort_pairs(ctx, WS_CY_TMP, a.ahash, a.ahash_s, a.aidx, a.aidx_s, (int)A, 64, st);
        k_ap_adup<<<ga, 256, 0, st>>>(a);
    }
    k_ap_badkeys<<<gk, 256, 0, st>>>(a);
    mh = fetch(a.m, st);
    refuse(mh);
    auto report = [&](int valid, int cause, u64 pos) {
        k_ap_report<<<1, 256, 0, st>>>(a, cause);
        const AMeta h = fetch(a.m, st);
        finish(res, valid, cause, (long long)(pos >> MOP_BITS), (long long)(pos & ((1 << MOP_BITS) - 1)), h.key, h.value);
        plan.cause = cause;
        return plan;
    };
    if (mh.dup_append != NONE) return report(JH_UNKNOWN, JH_CAUSE_DUPLICATE_APPENDS, mh.dup_append);
    if (mh.dup_read != NONE) return report(JH_INVALID, JH_CAUSE_DUPLICATE_ELEMENTS, mh.dup_read);
    if (mh.bad_keys) {
        const uint32_t row = fetch(a.badrow + mh.min_bad_key, st);
        finish(res, JH_INVALID, JH_CAUSE_NO_TOTAL_ORDER, row, (long long)mh.bad_keys, (long long)mh.min_bad_key, JH_NIL);
        plan.cause = JH_CAUSE_NO_TOTAL_ORDER;
        return plan;
    }

    // 6, 7. writers; the wr and ww slots; the rw runs
    if (R > 0) {
        k_ap_skey<<<gr, 256, 0, st>>>(a);
        sort_pairs(ctx, WS_CY_TMP, a.skey, a.skey_s, a.sidx, a.sidx_s, (int)R, 64, st);
        k_ap_wr<<<gr, 256, 0, st>>>(a);
    }
    k_ap_ww<<<ga, 256, 0, st>>>(a);
    excl_sum(ctx, WS_CY_TMP, as_input(a.rwcnt), a.rwoff, (int)(A + 1), st);
    long long RW = 0;
    HIP_TRY(hipMemcpyAsync(&RW, a.rwoff + A, sizeof RW, hipMemcpyDeviceToHost, st));
    mh = fetch(a.m, st);
    if (mh.no_writer != NONE) return report(JH_UNKNOWN, JH_CAUSE_NO_WRITER, mh.no_writer);
    if (RW > Y_MAX || R + A + RW > Y_MAX) throw_jh(JH_EUNSUPPORTED, "cycle: more than 2^31 - 2 vertices or edges");
    plan.reads = R; plan.appends = A; plan.rw = RW; plan.slots = R + A + RW;
    static_assert(sizeof(AP) <= sizeof plan.state, "AppendPlan::state holds an AP");
    memcpy(plan.state, &a, sizeof a);
    return plan;
}

long long append_fill(jh_ctx *ctx, const AppendPlan &plan, unsigned long long *raw, hipStream_t st) {
    AP a;
    memcpy(&a, plan.state, sizeof a);
    const long long RA = plan.reads + plan.appends;
    if (RA > 0) HIP_TRY(hipMemcpyAsync(raw, a.slots, sizeof(u64) * RA, hipMemcpyDeviceToDevice, st));
    if (plan.rw > 0) k_ap_rw<<<grid_for(plan.rw, 256, 4096), 256, 0, st>>>(a, plan.rw, raw + RA);
    return (long long)fetch(a.m, st).links;
}
