// jh_g2.hip -- the Adya G2 workload checker on MI355X.
//
// jepsen.tests.adya/g2-checker, jepsen/src/jepsen/tests/adya.clj:62-88: at most
// one :insert completes :ok for any key. The reference's reduce over the history
// is a histogram over the keys (include/jh.h), so the device makes
//   1. k_g2_count   one pass over the rows (type, f, key: 24 B a row): every
//                   insert row adds 1 | ok << 32 to cnt[key] with one 64-bit
//                   atomic. The low word is the key's insert rows (present iff
//                   > 0), the high word its :ok inserts. The workload has about
//                   four insert rows per key, so an address is rarely contended.
//   2. k_g2_keys    one pass over the keys: key_count, the keys with an :ok
//                   insert and the illegal keys, and the illegal keys as ballot
//                   words for row_select.h's scan
//      k_g2_emit    the first illegal_cap pairs [key id, count] in key-id order
//                   from the ballot words (no atomic)
//   3. only when some key is illegal: k_g2_first<0> takes every key's smallest
//      :ok insert row (atomicMin), k_g2_first<1> the smallest :ok insert row of
//      an illegal key that is not that one.
#include "row_select.h"

namespace {
constexpr int G_STEPS = 8;                    // keys per thread per tile of the key pass
constexpr int G_TILE = 256 * G_STEPS;         // keys per tile (G2_TILE in _abi.py: the tests straddle it)
constexpr int G_WORDS = G_TILE / 64;          // ballot words per tile (32)
constexpr unsigned long long NONE = ~0ULL;
constexpr long long G_MAX_ROWS = 0x7ffffffeLL;

struct GMeta {
    unsigned bad_key, unsup_key;
    unsigned long long insert_rows, key_count, ok_keys, first_row;
};

__global__ void k_g2_meta_init(GMeta *m) {
    memset(m, 0, sizeof *m);
    m->first_row = NONE;
}

// K = 0: a history without a key column (every insert row is then un-keyed)
__global__ void __launch_bounds__(256) k_g2_count(const int64_t *__restrict__ type, const int64_t *__restrict__ f,
                                                  const int64_t *__restrict__ key, int64_t n, int64_t K,
                                                  unsigned long long *__restrict__ cnt, GMeta *m) {
    __shared__ unsigned long long shr[4];
    unsigned long long ins = 0;
    for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x) {
        if (f[row] != JH_F_INSERT) continue;
        ins++;
        const int64_t k = K > 0 ? key[row] : -1;
        if (k < 0) atomicOr(&m->unsup_key, 1u);
        else if (k >= K) atomicOr(&m->bad_key, 1u);
        else atomicAdd(&cnt[k], 1ULL | (unsigned long long)(type[row] == T_OK) << 32);
    }
    ins = block_reduce256(ins, RedSum(), shr);
    if (threadIdx.x == 0 && ins) atomicAdd(&m->insert_rows, ins);
}

// Tile = 256 threads x G_STEPS keys, key tile * 2048 + u * 256 + thread: the
// ballot of wave w at step u is word tile * 32 + u * 4 + w, i.e. keys 64 j ..
__global__ void __launch_bounds__(256) k_g2_keys(const unsigned long long *__restrict__ cnt, int64_t K,
                                                 unsigned long long *__restrict__ words, long long *__restrict__ tile_cnt,
                                                 GMeta *m) {
    __shared__ unsigned sh[4];
    __shared__ unsigned long long shr[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_tiles = (K + G_TILE - 1) / G_TILE;
    unsigned long long present = 0, okk = 0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        unsigned c = 0;
#pragma unroll
        for (int u = 0; u < G_STEPS; u++) {
            const int64_t k = tile * G_TILE + u * 256 + threadIdx.x;
            const unsigned long long x = k < K ? cnt[k] : 0;
            present += (unsigned)x > 0;
            okk += (x >> 32) > 0;
            const unsigned long long b = __ballot((x >> 32) > 1);
            c += __popcll(b);
            if (lane == 0) words[tile * G_WORDS + u * 4 + wave] = b;
        }
        if (lane == 0) sh[wave] = c;
        __syncthreads();
        if (threadIdx.x == 0) tile_cnt[tile] = (long long)(sh[0] + sh[1] + sh[2] + sh[3]);
        __syncthreads();
    }
    present = block_reduce256(present, RedSum(), shr);
    okk = block_reduce256(okk, RedSum(), shr);
    if (threadIdx.x == 0) {
        if (present) atomicAdd(&m->key_count, present);
        if (okk) atomicAdd(&m->ok_keys, okk);
    }
}

__global__ void __launch_bounds__(256) k_g2_emit(const unsigned long long *__restrict__ cnt, int64_t K,
                                                 const unsigned long long *__restrict__ words,
                                                 const long long *__restrict__ tile_base, long long cap,
                                                 int64_t *__restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt = (1ULL << lane) - 1;
    const int64_t n_tiles = (K + G_TILE - 1) / G_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        unsigned long long w;
        unsigned excl;
        if (rs_word_prefix<G_WORDS>(words + tile * G_WORDS, lane, w, excl) == 0) continue;   // no illegal key in this tile
        const long long base = tile_base[tile];
        if (base >= cap) continue;                            // block-uniform
#pragma unroll
        for (int u = 0; u < G_STEPS; u++) {
            const int wi = u * 4 + wave;
            const unsigned long long bits = __shfl(w, wi);
            const unsigned at = __shfl(excl, wi);
            if (!((bits >> lane) & 1)) continue;              // nothing below is cross-lane
            const int64_t k = tile * G_TILE + wi * 64 + lane;      // < K: only keys below K are flagged
            const long long o = base + at + __popcll(bits & lt);
            if (o < cap) { out[2 * o] = k; out[2 * o + 1] = (int64_t)(cnt[k] >> 32); }
        }
    }
}

// PASS 0: first[k] = the key's smallest :ok insert row. PASS 1: the smallest :ok
// insert row of an illegal key that is not first[k]. Every insert row's key is
// in [0, K) here: the count pass found no other.
template <int PASS>
__global__ void __launch_bounds__(256) k_g2_first(const int64_t *__restrict__ type, const int64_t *__restrict__ f,
                                                  const int64_t *__restrict__ key, int64_t n,
                                                  const unsigned long long *__restrict__ cnt,
                                                  unsigned *__restrict__ first, GMeta *m) {
    __shared__ unsigned long long shr[4];
    unsigned long long best = NONE;
    for (int64_t row = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; row < n; row += (int64_t)gridDim.x * blockDim.x) {
        if (f[row] != JH_F_INSERT || type[row] != T_OK) continue;
        const int64_t k = key[row];
        if ((cnt[k] >> 32) < 2) continue;
        if (PASS == 0) atomicMin(&first[k], (unsigned)row);
        else if (first[k] != (unsigned)row) best = min(best, (unsigned long long)row);
    }
    if (PASS == 1) {
        best = block_reduce256(best, RedMin(), shr);
        if (threadIdx.x == 0 && best != NONE) atomicMin(&m->first_row, best);
    }
}

}  // namespace

void g2_check(jh_ctx *ctx, const jh_history *dh, jh_g2_result *res, int64_t *illegal_out, int64_t illegal_cap,
              hipStream_t st) {
    memset(res, 0, sizeof *res);
    res->valid = JH_VALID;
    res->first_illegal_row = -1;
    const int64_t n = dh->n;
    if (n == 0) return;
    if (n > G_MAX_ROWS) throw_jh(JH_EUNSUPPORTED, "g2: more than 2^31 - 2 rows");
    const int64_t K = dh->key != nullptr && dh->n_keys > 0 ? dh->n_keys : 0;
    DeviceTimer timer{ctx, st};
    timer.start();

    // 1. the histogram
    GMeta *m = ctx->ws<GMeta>(WS_G2_META, 1);
    k_g2_meta_init<<<1, 1, 0, st>>>(m);
    unsigned long long *cnt = ctx->ws<unsigned long long>(WS_G2_CNT, K);
    HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * K, st));
    const int gr = grid_for(n, 256 * 4, 8192);
    k_g2_count<<<gr, 256, 0, st>>>(dh->type, dh->f, dh->key, n, K, cnt, m);
    GMeta mh = fetch(m, st);
    if (mh.bad_key) throw_jh(JH_EINVAL, "g2: a key outside [0, n_keys)");
    if (mh.unsup_key) throw_jh(JH_EUNSUPPORTED, "g2: an :insert without a key");
    res->insert_rows = (int64_t)mh.insert_rows;
    if (K == 0 || mh.insert_rows == 0) {
        res->device_ms = timer.stop();
        return;
    }

    // 2. the keys
    const RowSel<1> sel = select_rows<1>(
        ctx, {WS_G2_WORDS, WS_G2_TCNT, WS_G2_TBASE, WS_G2_TMP}, K, G_TILE, G_WORDS,
        [&](int g, unsigned long long *words, long long *tile_cnt) {
            k_g2_keys<<<g, 256, 0, st>>>(cnt, K, words, tile_cnt, m);
        }, st);
    const long long I = sel.count[0];
    mh = fetch(m, st);
    res->key_count = (int64_t)mh.key_count;
    res->illegal_count = I;
    res->legal_count = (int64_t)mh.ok_keys - I;
    res->valid = I > 0 ? JH_INVALID : JH_VALID;
    if (I > 0) {
        const long long cap = illegal_out ? std::min<long long>(I, std::max<int64_t>(illegal_cap, 0)) : 0;
        if (cap > 0) {
            int64_t *out = ctx->ws<int64_t>(WS_G2_OUT, 2 * cap);
            k_g2_emit<<<sel.grid, 256, 0, st>>>(cnt, K, sel.words[0], sel.base[0], cap, out);
            HIP_TRY(hipMemcpyAsync(illegal_out, out, sizeof(int64_t) * 2 * cap, hipMemcpyDeviceToHost, st));
        }
        // 3. the first failing op
        unsigned *first = ctx->ws<unsigned>(WS_G2_MIN, K);
        HIP_TRY(hipMemsetAsync(first, 0xff, sizeof(unsigned) * K, st));
        k_g2_first<0><<<gr, 256, 0, st>>>(dh->type, dh->f, dh->key, n, cnt, first, m);
        k_g2_first<1><<<gr, 256, 0, st>>>(dh->type, dh->f, dh->key, n, cnt, first, m);
        mh = fetch(m, st);
        res->first_illegal_row = mh.first_row == NONE ? -1 : (int64_t)mh.first_row;
    }
    HIP_TRY(hipStreamSynchronize(st));
    res->device_ms = timer.stop();
}
