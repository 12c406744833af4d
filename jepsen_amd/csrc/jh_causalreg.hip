// jh_causalreg.hip -- the causal workload checker on MI355X.
//
// jepsen.tests.causal/check over (causal-register), lifted by
// independent/checker, jepsen/src/jepsen/tests/causal.clj:33-110, batched over
// the keys. The reference steps a register (value, counter, last-pos) through
// the key's :ok ops. In a valid prefix value = counter = the :ok writes so far
// and last-pos = the position of the key's previous :ok row, so a row's verdict
// needs two things only (include/jh.h): w, the key's :ok writes before the row,
// and p, the position of the key's previous :ok row. The key's first event row
// decides the key.
//
// Keys have about five rows each and there are millions of them, so the
// pipeline is flat:
//   1. k_cm_flag     type / key: the :ok rows as ballot words and their number
//                    per 2048-row tile, the key checks into the meta block
//                    (row_select.h does the scans)
//      k_cm_compact  the :ok rows in history order from the ballot words (no
//                    atomic) as (key | class << 30, row); class = read / write
//                    / read-init / other from f, read here in row order so that
//                    the judge does not gather it
//   2. one stable radix sort on the key bits alone (skipped for one key),
//      k_cm_bounds: per-key offsets by binary search
//   3. S = the inclusive sum of the write bits over the sorted slots (one scan
//      through a transform iterator: 4 B read, 4 B written per slot), so that
//      w = S[i] - S[off[key]] whatever number of tiles the key's run spans
//      k_cm_judge    one sorted slot per lane, CM_TILE slots per tile: gathers
//                    value, position and link, takes p from the slot before (in
//                    LDS; the tile's first slot gathers it), evaluates the event
//                    and its kind, atomicMin(slot << 3 | kind) per key
//   4. k_cm_finish   per key: the jh_causal_key record from the event slot, or
//                    from the run's last slot when the key is valid; the counts
#include "row_select.h"

namespace {
constexpr int F_STEPS = 8;                    // rows per thread per tile of the flag pass
constexpr int F_TILE = 256 * F_STEPS;         // rows per tile (2048)
constexpr int F_WORDS = F_TILE / 64;          // ballot words per tile (32)
constexpr int CM_STEPS = 4;                   // slots per thread per tile of the judge
constexpr int CM_TILE = 256 * CM_STEPS;       // CM_TILE in _abi.py: the tests straddle it
constexpr unsigned KEYBITS = 30, KEYMASK = (1u << KEYBITS) - 1;
constexpr unsigned CL_READ = 0, CL_WRITE = 1, CL_READ_INIT = 2, CL_OTHER = 3;
constexpr unsigned long long NONE = ~0ULL;
constexpr long long CM_MAX_COUNT = 0x7ffffffeLL;

struct MMeta {
    unsigned bad_key, unsup_key;
    unsigned long long invalid_keys, unknown_keys, first_row;
};

__global__ void k_cm_meta_init(MMeta *m) {
    memset(m, 0, sizeof *m);
    m->first_row = NONE;
}

// ---------------------------------------------------------------------------
// 1. Tile = 256 threads x F_STEPS rows, row tile * 2048 + u * 256 + thread: the
// ballot of wave w at step u is word tile * 32 + u * 4 + w, i.e. rows 64 j ..
// K = 0: an un-keyed history (every :ok row is key 0).
__global__ void __launch_bounds__(256) k_cm_flag(const int64_t *__restrict__ process, const int64_t *__restrict__ type,
                                                 const int64_t *__restrict__ key, int64_t n, int64_t K,
                                                 unsigned long long *__restrict__ words, long long *__restrict__ cnt,
                                                 MMeta *m) {
    __shared__ unsigned sh[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_tiles = (n + F_TILE - 1) / F_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        unsigned c = 0;
#pragma unroll
        for (int u = 0; u < F_STEPS; u++) {
            const int64_t row = tile * F_TILE + u * 256 + threadIdx.x;
            bool ok = row < n && type[row] == T_OK;
            if (ok && K > 0) {
                const int64_t kk = key[row];
                if (kk < 0) {
                    if (process[row] >= 0) atomicOr(&m->unsup_key, 1u);
                    ok = false;
                } else if (kk >= K) {
                    atomicOr(&m->bad_key, 1u);
                    ok = false;
                }
            }
            const unsigned long long b = __ballot(ok);
            c += __popcll(b);
            if (lane == 0) words[tile * F_WORDS + u * 4 + wave] = b;
        }
        if (lane == 0) sh[wave] = c;
        __syncthreads();
        if (threadIdx.x == 0) cnt[tile] = (long long)(sh[0] + sh[1] + sh[2] + sh[3]);
        __syncthreads();
    }
}

__device__ __forceinline__ unsigned cm_class(int64_t f) {
    return f == JH_F_READ ? CL_READ : f == JH_F_WRITE ? CL_WRITE : f == JH_F_READ_INIT ? CL_READ_INIT : CL_OTHER;
}

// The :ok rows in history order: every wave scans the tile's 32 ballot words
// itself; the exclusive prefix of their popcounts at word u * 4 + wave is where
// the wave's rows of step u go.
__global__ void __launch_bounds__(256) k_cm_compact(const int64_t *__restrict__ f, const int64_t *__restrict__ key,
                                                    int64_t n, int64_t K, const unsigned long long *__restrict__ words,
                                                    const long long *__restrict__ tile_base, uint32_t *__restrict__ kc,
                                                    uint32_t *__restrict__ rr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt = (1ULL << lane) - 1;
    const int64_t n_tiles = (n + F_TILE - 1) / F_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        unsigned long long w;
        unsigned excl;
        if (rs_word_prefix<F_WORDS>(words + tile * F_WORDS, lane, w, excl) == 0) continue;   // no :ok row in this tile
        const long long base = tile_base[tile];
#pragma unroll
        for (int u = 0; u < F_STEPS; u++) {
            const int wi = u * 4 + wave;
            const unsigned long long bits = __shfl(w, wi);
            const unsigned at = __shfl(excl, wi);
            if (!((bits >> lane) & 1)) continue;              // nothing below is cross-lane
            const int64_t row = tile * F_TILE + wi * 64 + lane;    // < n: only rows below n are flagged
            const long long o = base + at + __popcll(bits & lt);
            const unsigned k = K > 0 ? (unsigned)key[row] : 0u;     // in [0, K): the flag pass checked it
            kc[o] = k | cm_class(f[row]) << KEYBITS;
            rr[o] = (uint32_t)row;
        }
    }
}

// ---------------------------------------------------------------------------
// 2. off[k] = the number of sorted slots whose key is below k, k = 0 .. K
__global__ void __launch_bounds__(256) k_cm_bounds(const uint32_t *__restrict__ kc, int64_t cnt, int64_t K,
                                                   int32_t *__restrict__ off) {
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k <= K; k += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = cnt;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)(kc[mid] & KEYMASK) < k) lo = mid + 1;
            else hi = mid;
        }
        off[k] = (int32_t)lo;
    }
}

struct IsWrite {
    __host__ __device__ int operator()(uint32_t x) const { return (x >> KEYBITS) == CL_WRITE; }
};

// ---------------------------------------------------------------------------
// 3. One sorted slot per lane. S[i] = the write slots below i (S has M + 1
// entries), off[k] = the first slot of key k: both lie inside the buffers
// whatever the columns hold, and rows come from the compact pass (< n).
__global__ void __launch_bounds__(256) k_cm_judge(const uint32_t *__restrict__ kc, const uint32_t *__restrict__ rr,
                                                  const int32_t *__restrict__ S, const int32_t *__restrict__ off,
                                                  const int64_t *__restrict__ value, const int64_t *__restrict__ aux,
                                                  int64_t M, unsigned long long *__restrict__ ev) {
    __shared__ long long s_pos[CM_TILE];
    __shared__ uint32_t s_kc[CM_TILE];
    const int64_t n_tiles = (M + CM_TILE - 1) / CM_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t base = tile * CM_TILE;
        long long v[CM_STEPS], link[CM_STEPS];
#pragma unroll
        for (int u = 0; u < CM_STEPS; u++) {
            const int j = u * 256 + threadIdx.x;
            const int64_t i = base + j;
            uint32_t x = 0;
            long long pos = JH_NIL;
            v[u] = JH_NIL; link[u] = JH_NIL;
            if (i < M) {
                x = kc[i];
                const int64_t row = rr[i];
                v[u] = value[row];
                pos = aux[2 * row];
                link[u] = aux[2 * row + 1];
            }
            s_kc[j] = x;
            s_pos[j] = pos;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < CM_STEPS; u++) {
            const int j = u * 256 + threadIdx.x;
            const int64_t i = base + j;
            if (i >= M) continue;                             // nothing below is cross-lane
            const uint32_t x = s_kc[j], k = x & KEYMASK, cls = x >> KEYBITS;
            long long prev = JH_NIL;                          // the position of the key's previous :ok row
            if (j > 0) {
                if ((s_kc[j - 1] & KEYMASK) == k) prev = s_pos[j - 1];
            } else if (i > 0 && (kc[i - 1] & KEYMASK) == k) {
                prev = aux[2 * (int64_t)rr[i - 1]];           // the last slot of the tile before
            }
            const long long w = (long long)S[i] - S[off[k]];
            int kind = 0;
            if (link[u] != JH_CAUSAL_INIT && link[u] != prev) kind = 1;
            else if (cls == CL_WRITE) kind = v[u] == w + 1 ? 0 : 2;
            else if (cls == CL_READ_INIT) kind = (w == 0 && v[u] != 0) || (v[u] != JH_NIL && v[u] != w) ? 3 : 0;
            else if (cls == CL_READ) kind = v[u] != JH_NIL && v[u] != w ? 4 : 0;
            else kind = 5;
            if (kind) atomicMin(&ev[k], (unsigned long long)i << 3 | (unsigned)kind);
        }
        __syncthreads();                                      // the tile's LDS is read before the next one is written
    }
}

__global__ void __launch_bounds__(256) k_cm_fill64(unsigned long long *__restrict__ p, int64_t cnt, unsigned long long v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

// ---------------------------------------------------------------------------
// 4. One key per thread. M = 0: no buffer but out and the meta is touched.
__global__ void __launch_bounds__(256) k_cm_finish(const uint32_t *__restrict__ rr, const int32_t *__restrict__ S,
                                                   const int32_t *__restrict__ off, const int64_t *__restrict__ aux,
                                                   const unsigned long long *__restrict__ ev, int64_t K, int64_t M,
                                                   jh_causal_key *__restrict__ out, MMeta *m) {
    __shared__ unsigned long long shr[4];
    unsigned long long inv = 0, unk = 0, first = NONE;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < K; k += (int64_t)gridDim.x * blockDim.x) {
        jh_causal_key r = {JH_VALID, 0, -1, 0, JH_NIL};
        if (M > 0) {
            const int64_t b = off[k], e = off[k + 1];
            const unsigned long long x = ev[k];
            if (x != NONE) {
                const int64_t i = (int64_t)(x >> 3);
                r.kind = (int32_t)(x & 7);
                r.valid = r.kind == 5 ? JH_UNKNOWN : JH_INVALID;
                r.row = rr[i];
                r.counter = (long long)S[i] - S[b];
                if (i > b) r.last_pos = aux[2 * (int64_t)rr[i - 1]];
                if (r.kind == 5) unk++;
                else inv++;
                first = min(first, (unsigned long long)r.row);
            } else if (e > b) {
                r.counter = (long long)S[e] - S[b];
                r.last_pos = aux[2 * (int64_t)rr[e - 1]];
            }
        }
        out[k] = r;
    }
    inv = block_reduce256(inv, RedSum(), shr);
    unk = block_reduce256(unk, RedSum(), shr);
    first = block_reduce256(first, RedMin(), shr);
    if (threadIdx.x == 0) {
        if (inv) atomicAdd(&m->invalid_keys, inv);
        if (unk) atomicAdd(&m->unknown_keys, unk);
        if (first != NONE) atomicMin(&m->first_row, first);
    }
}

int bits_of(unsigned long long x) {
    int b = 1;
    while (b < 64 && (x >> b)) b++;
    return b;
}

}  // namespace

void causal_check(jh_ctx *ctx, const jh_history *dh, jh_causal_result *res, jh_causal_key *keys_out, hipStream_t st) {
    memset(res, 0, sizeof *res);
    res->valid = JH_VALID;
    res->first_event_row = -1;
    const int64_t n = dh->n;
    const bool keyed = dh->key != nullptr && dh->n_keys > 0;
    const int64_t K = keyed ? dh->n_keys : 1, n_out = std::max<int64_t>(dh->n_keys, 1);
    if (keys_out)
        for (int64_t k = 0; k < n_out; k++) keys_out[k] = jh_causal_key{JH_VALID, 0, -1, 0, JH_NIL};
    if (n == 0) return;
    if (K > (int64_t)KEYMASK) throw_jh(JH_EUNSUPPORTED, "causal: more than 2^30 - 1 keys");
    if (n > 0xffffffffLL) throw_jh(JH_EUNSUPPORTED, "causal: more than 2^32 - 1 rows");
    DeviceTimer timer{ctx, st};
    timer.start();

    // 1. the :ok rows, in history order
    MMeta *m = ctx->ws<MMeta>(WS_CM_META, 1);
    k_cm_meta_init<<<1, 1, 0, st>>>(m);
    const int64_t Kc = keyed ? K : 0;
    const RowSel<1> sel = select_rows<1>(
        ctx, {WS_CM_WORDS, WS_CM_TCNT, WS_CM_TBASE, WS_CM_TMP}, n, F_TILE, F_WORDS,
        [&](int g, unsigned long long *words, long long *tile_cnt) {
            k_cm_flag<<<g, 256, 0, st>>>(dh->process, dh->type, dh->key, n, Kc, words, tile_cnt, m);
        }, st);
    const long long M = sel.count[0];
    MMeta mh = fetch(m, st);
    if (mh.bad_key) throw_jh(JH_EINVAL, "causal: a key outside [0, n_keys)");
    if (mh.unsup_key) throw_jh(JH_EUNSUPPORTED, "causal: an :ok row of a client process without a key in a keyed history");
    if (M > CM_MAX_COUNT) throw_jh(JH_EUNSUPPORTED, "causal: more than 2^31 - 2 :ok rows");
    res->ok_count = M;

    jh_causal_key *out = ctx->ws<jh_causal_key>(WS_CM_OUT, K);
    const int gk = grid_for(K, 256, 2048);
    if (M > 0) {
        uint32_t *kc = ctx->ws<uint32_t>(WS_CM_KEY, 2 * M), *kc_s = kc + M;
        uint32_t *rr = ctx->ws<uint32_t>(WS_CM_ROW, 2 * M), *rr_s = rr + M;
        k_cm_compact<<<sel.grid, 256, 0, st>>>(dh->f, dh->key, n, Kc, sel.words[0], sel.base[0], kc, rr);

        // 2. buckets (one key: the compacted order is the bucket)
        const uint32_t *ks = kc, *rs = rr;
        if (K > 1) {
            sort_pairs(ctx, WS_CM_TMP, kc, kc_s, rr, rr_s, (int)M, bits_of((unsigned long long)(K - 1)), st);
            ks = kc_s; rs = rr_s;
        }
        int32_t *off = ctx->ws<int32_t>(WS_CM_OFF, K + 1);
        k_cm_bounds<<<grid_for(K + 1, 256, 2048), 256, 0, st>>>(ks, M, K, off);

        // 3. the write counts and the events
        int32_t *S = ctx->ws<int32_t>(WS_CM_SUM, M + 1);
        HIP_TRY(hipMemsetAsync(S, 0, sizeof(int32_t), st));
        incl_sum(ctx, WS_CM_TMP, hipcub::TransformInputIterator<int, IsWrite, const uint32_t *>(ks, IsWrite()), S + 1,
                 (int)M, st);
        unsigned long long *ev = ctx->ws<unsigned long long>(WS_CM_EV, K);
        k_cm_fill64<<<gk, 256, 0, st>>>(ev, K, NONE);
        k_cm_judge<<<grid_for((M + CM_TILE - 1) / CM_TILE, 1, 4096), 256, 0, st>>>(ks, rs, S, off, dh->value, dh->aux, M, ev);

        // 4. the keys
        k_cm_finish<<<gk, 256, 0, st>>>(rs, S, off, dh->aux, ev, K, M, out, m);
    } else {
        k_cm_finish<<<gk, 256, 0, st>>>(nullptr, nullptr, nullptr, nullptr, nullptr, K, 0, out, m);
    }
    if (keys_out) HIP_TRY(hipMemcpyAsync(keys_out, out, sizeof(jh_causal_key) * K, hipMemcpyDeviceToHost, st));
    mh = fetch(m, st);
    res->invalid_keys = (int64_t)mh.invalid_keys;
    res->unknown_keys = (int64_t)mh.unknown_keys;
    res->first_event_row = mh.first_row == NONE ? -1 : (int64_t)mh.first_row;
    res->valid = mh.invalid_keys ? JH_INVALID : mh.unknown_keys ? JH_UNKNOWN : JH_VALID;
    res->cause = mh.unknown_keys ? JH_CAUSE_BAD_F : JH_CAUSE_NONE;
    res->device_ms = timer.stop();
}
