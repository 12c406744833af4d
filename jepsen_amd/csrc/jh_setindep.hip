// jh_setindep.hip -- (independent/checker (checker/set)) on MI355X: every key
// of an independent history judged by checker.clj:182-233 in one call.
//
// Per key (its rows; in a keyed history no un-keyed row may matter, else the
// call refuses): attempts A = elements of :invoke :add, acknowledged D = those
// of :ok :add, R = the elements of the last :ok :read; ok = R n A, unexpected =
// R - A, lost = D - R, recovered = ok - D, as bitmaps over the key's own
// element span. Each key owns a whole number of words of the four output
// bitmaps (word_off = the running sum of the keys' word counts).
//
//   k_si_meta    one flat pass over the rows: per key the element min / max of
//                its add rows and its last :ok :read row; the refusals
//   k_si_range   one workgroup per key: the final read's element range folded
//                into min / max, the key's word count and tier
//   (scan)       word_off
//   k_si_lds     on-chip tier, one workgroup per key: A, D, R in LDS from the
//                key's rows (the stable key partition) and read elements, then
//                the four sets, the counts and the first lost row; every
//                output word written once, no HBM atomics, nothing to clear
//   k_si_mark_*, k_si_words, k_si_first_lost
//                global tier: A, D, R concatenated in HBM, marked row-parallel
//                with the LDS-merged atomicOr of jh_set.hip, then one pass over
//                the words that finds each word's key from word_off
//   k_si_finish  the jh_set_key records
#include "jh_set_bits.h"

// jh_lin.hip: the stable key partition left on the device (rows sorted by key,
// n_keys + 1 segment offsets; the un-keyed rows come last)
void key_partition_device(jh_ctx *ctx, const jh_history *dh, const uint32_t **rows, const uint32_t **off,
                          hipStream_t stream);

namespace {

constexpr int SI_WORDS = JH_SI_LDS_SPAN / 32;      // words per bitmap of the on-chip tier
constexpr int SI_CHUNK = 2048;                     // words per workgroup of k_si_words
constexpr int SI_TAB = 8;                          // keys a workgroup of k_si_words merges in LDS
constexpr unsigned long long SI_NONE = ~0ULL;

enum : int { SI_BAD_KEY = 1, SI_UNSUP_KEY = 2, SI_NIL_ADD = 4, SI_BAD_RANGE = 8, SI_UNSUP_SPAN = 16, SI_OVER = 32 };

struct SiKey {
    long long vmin, vmax;            // the add rows' elements, then the final read's folded in (vmin: base)
    long long final_row;             // last :ok :read row, -1: none
    long long roff, rcnt;            // its element range in aux
    long long n_words;
    unsigned long long first_lost;   // smallest row of an :ok :add whose element is lost
    unsigned long long cnt[6];       // attempt, acknowledged, ok, lost, recovered, unexpected
    int tier;                        // 0: nothing to judge (in no row, or never read), 1 on chip, 2 global
    int unknown;
};

struct SiMeta {
    int flags;
    int n_global;
    long long max_gcnt;              // longest final read of a global-tier key
    unsigned long long read_elems;   // final-read elements of the judged keys
};

__global__ void k_si_init(SiKey *keys, int64_t K, long long *nw, SiMeta *m) {
    const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (k == 0) { m->flags = 0; m->n_global = 0; m->max_gcnt = 0; m->read_elems = 0; nw[K] = 0; }
    if (k >= K) return;
    SiKey &r = keys[k];
    r.vmin = LLONG_MAX; r.vmax = LLONG_MIN; r.final_row = -1; r.roff = 0; r.rcnt = 0; r.n_words = 0;
    r.first_lost = SI_NONE;
    for (int i = 0; i < 6; i++) r.cnt[i] = 0;
    r.tier = 0; r.unknown = 0;
}

// min / max go to the key's record only when they move it: a stale read of the
// record is less extreme than its present value, so it never drops an update
__device__ __forceinline__ void si_commit(SiKey *kr, long long lo, long long hi, long long fr) {
    if (lo <= hi) {
        if (lo < *(volatile long long *)&kr->vmin) atomicMin(&kr->vmin, lo);
        if (hi > *(volatile long long *)&kr->vmax) atomicMax(&kr->vmax, hi);
    }
    if (fr >= 0) atomicMax(&kr->final_row, fr);
}

// One flat pass over the rows (type, f, key, value: 32 B per row, 16-byte
// loads). keyed == 0: every row is key 0. A wave whose rows all carry one key
// (an un-keyed history, rows grouped by key) is reduced by shuffles first and
// commits once; otherwise each lane commits its own row.
__global__ void __launch_bounds__(256) k_si_meta(const int64_t *__restrict__ type, const int64_t *__restrict__ f,
                                                 const int64_t *__restrict__ key, const int64_t *__restrict__ val,
                                                 int64_t n, int64_t K, int keyed, int vec, SiKey *keys, SiMeta *m) {
    const int64_t np = (n + 1) / 2;
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t i_lane0 = i - (threadIdx.x & 63);
    int flags = 0;
    // the loop runs while any lane of the wave has a pair: every lane takes part in the shuffles
    for (int64_t w0 = i_lane0; w0 < np; w0 += gs, i += gs) {
        const bool live = i < np;
        longlong2 t2 = make_longlong2(0, 0), f2 = t2, k2 = t2, v2 = t2;
        if (live) {
            t2 = ld_pair(type, i, n, vec); f2 = ld_pair(f, i, n, vec); v2 = ld_pair(val, i, n, vec);
            if (keyed) k2 = ld_pair(key, i, n, vec);
        }
        const int64_t tt[2] = {t2.x, t2.y}, ffs[2] = {f2.x, f2.y}, kks[2] = {k2.x, k2.y}, vv[2] = {v2.x, v2.y};
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int64_t r = 2 * i + h;
            long long kk = -1, lo = LLONG_MAX, hi = LLONG_MIN, fr = -1;
            if (live && r < n) {
                const int64_t ty = tt[h], ff = ffs[h];
                const bool add = ff == JH_F_ADD && (ty == T_INVOKE || ty == T_OK);
                const bool rd = ff == JH_F_READ && ty == T_OK;
                const int64_t k = keyed ? kks[h] : 0;
                if (k < 0) { if (add || rd) flags |= SI_UNSUP_KEY; }
                else if (k >= K) flags |= SI_BAD_KEY;
                else if (add) {
                    if (vv[h] == JH_NIL) flags |= SI_NIL_ADD;
                    else { kk = k; lo = hi = vv[h]; }
                } else if (rd) { kk = k; fr = r; }
            }
            const long long k0 = __shfl(kk, __ffsll((long long)__ballot(kk >= 0)) - 1);
            if (__all(kk < 0 || kk == k0)) {
                if (__any(kk >= 0)) {
                    for (int o = 32; o > 0; o >>= 1) {
                        lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); fr = max(fr, __shfl_xor(fr, o));
                    }
                    if ((threadIdx.x & 63) == 0) si_commit(&keys[k0], lo, hi, fr);
                }
            } else if (kk >= 0) {
                si_commit(&keys[kk], lo, hi, fr);
            }
        }
    }
    if (flags) atomicOr(&m->flags, flags);
}

// One workgroup per key: the final read's range checked and its elements
// folded into the key's min / max; the key's span, word count and tier.
__global__ void __launch_bounds__(256) k_si_range(SiKey *keys, int64_t K, const uint32_t *__restrict__ off, int64_t n,
                                                  const int64_t *__restrict__ val, const int64_t *__restrict__ val2,
                                                  const int64_t *__restrict__ aux, int64_t n_aux, int path,
                                                  long long *__restrict__ nw_out, SiMeta *m) {
    __shared__ long long s_off, s_cnt;
    __shared__ int s_state;            // 0: nothing to judge, 1: judged
    __shared__ long long sh[4];
    for (int64_t k = blockIdx.x; k < K; k += gridDim.x) {
        SiKey &kr = keys[k];
        if (threadIdx.x == 0) {
            const int64_t rows = off ? (int64_t)off[k + 1] - (int64_t)off[k] : n;
            const long long fr = kr.final_row;
            s_state = 0; s_off = 0; s_cnt = 0;
            if (rows > 0) {
                if (fr < 0 || val[fr] == JH_NIL) kr.unknown = 1;
                else {
                    const long long o = val[fr], c = val2[fr];
                    if (c < 0 || o < 0 || o > n_aux || c > n_aux - o || (c > 0 && !aux)) atomicOr(&m->flags, SI_BAD_RANGE);
                    else { s_state = 1; s_off = o; s_cnt = c; }
                }
            }
        }
        __syncthreads();
        const int state = s_state;
        const long long ro = s_off, rc = s_cnt;
        long long lo = LLONG_MAX, hi = LLONG_MIN;
        if (state)
            for (long long j = threadIdx.x; j < rc; j += blockDim.x) { const long long v = aux[ro + j]; lo = min(lo, v); hi = max(hi, v); }
        lo = block_reduce256(lo, RedMin(), sh);
        hi = block_reduce256(hi, RedMax(), sh);
        if (threadIdx.x == 0) {
            long long nw = 0;
            if (state) {
                lo = min(lo, kr.vmin); hi = max(hi, kr.vmax);
                if (lo > hi) { lo = 0; hi = 0; }
                const unsigned long long d = (unsigned long long)hi - (unsigned long long)lo;
                if (d >= (1ULL << 34)) atomicOr(&m->flags, SI_UNSUP_SPAN);
                else {
                    const unsigned long long span = d + 1;
                    nw = (long long)((span + 31) / 32);
                    int tier = path == 2 || span > (unsigned long long)JH_SI_LDS_SPAN ? 2 : 1;
                    if (path == 1 && tier == 2) { atomicOr(&m->flags, SI_OVER); tier = 0; nw = 0; }
                    kr.tier = tier;
                    kr.vmin = lo; kr.vmax = hi; kr.roff = ro; kr.rcnt = rc;
                    if (tier == 2) { atomicAdd(&m->n_global, 1); atomicMax(&m->max_gcnt, rc); }
                    if (tier) atomicAdd(&m->read_elems, (unsigned long long)rc);
                }
            }
            kr.n_words = nw;
            nw_out[k] = nw;
        }
        __syncthreads();
    }
}

// On-chip tier: one workgroup per key. The key's rows come through the stable
// key partition (rows == null: an un-keyed history, every row in order).
__global__ void __launch_bounds__(256) k_si_lds(SiKey *keys, int64_t K, const uint32_t *__restrict__ off,
                                                const uint32_t *__restrict__ rows, int64_t n,
                                                const int64_t *__restrict__ type, const int64_t *__restrict__ f,
                                                const int64_t *__restrict__ val, const int64_t *__restrict__ aux,
                                                const long long *__restrict__ word_off, int64_t total,
                                                uint32_t *__restrict__ outb) {
    __shared__ uint32_t sA[SI_WORDS], sD[SI_WORDS], sR[SI_WORDS];
    __shared__ long long sh[4];
    const int tid = threadIdx.x;
    for (int64_t k = blockIdx.x; k < K; k += gridDim.x) {
        SiKey &kr = keys[k];
        if (kr.tier != 1) continue;                        // (the same for every thread)
        const int nw = (int)kr.n_words;                    // <= SI_WORDS: the tier's span bound
        const long long base = kr.vmin;
        for (int w = tid; w < nw; w += 256) { sA[w] = 0; sD[w] = 0; sR[w] = 0; }
        __syncthreads();
        const int64_t r0 = off ? off[k] : 0, r1 = off ? off[k + 1] : n;
        for (int64_t i = r0 + tid; i < r1; i += 256) {
            const int64_t r = rows ? rows[i] : i;
            if (f[r] != JH_F_ADD) continue;
            const int64_t ty = type[r];
            if (ty != T_INVOKE && ty != T_OK) continue;
            const unsigned long long b = (unsigned long long)(val[r] - base);
            atomicOr(ty == T_INVOKE ? &sA[b >> 5] : &sD[b >> 5], 1u << (b & 31));
        }
        const long long ro = kr.roff, rc = kr.rcnt;
        for (long long j = tid; j < rc; j += 256) {
            const unsigned long long b = (unsigned long long)(aux[ro + j] - base);
            atomicOr(&sR[b >> 5], 1u << (b & 31));
        }
        __syncthreads();
        long long c[6] = {0, 0, 0, 0, 0, 0};
        const int64_t wo = word_off[k];
        for (int w = tid; w < nw; w += 256) {
            uint32_t x[4];
            set_algebra(sA[w], sD[w], sR[w], x);
            c[0] += __popc(sA[w]); c[1] += __popc(sD[w]);
            c[2] += __popc(x[0]); c[3] += __popc(x[1]); c[4] += __popc(x[3]); c[5] += __popc(x[2]);
#pragma unroll
            for (int s = 0; s < 4; s++) outb[s * total + wo + w] = x[s];
        }
#pragma unroll
        for (int q = 0; q < 6; q++) c[q] = block_reduce256(c[q], RedSum(), sh);
        long long best = LLONG_MAX;
        if (c[3] > 0)                                      // (block-wide value)
            for (int64_t i = r0 + tid; i < r1; i += 256) {
                const int64_t r = rows ? rows[i] : i;
                if (f[r] != JH_F_ADD || type[r] != T_OK) continue;
                const unsigned long long b = (unsigned long long)(val[r] - base);
                if (!((sR[b >> 5] >> (b & 31)) & 1)) best = min(best, (long long)r);
            }
        best = block_reduce256(best, RedMin(), sh);
        if (tid == 0) {
            for (int q = 0; q < 6; q++) kr.cnt[q] = (unsigned long long)c[q];
            kr.first_lost = best == LLONG_MAX ? SI_NONE : (unsigned long long)best;
        }
        __syncthreads();
    }
}

// Global tier, rows: :invoke :add elements into A, :ok :add elements into D,
// at the key's words of the concatenated bitmaps
__global__ void __launch_bounds__(256) k_si_mark_rows(const int64_t *__restrict__ type, const int64_t *__restrict__ f,
                                                      const int64_t *__restrict__ key, const int64_t *__restrict__ val,
                                                      int64_t n, const SiKey *__restrict__ keys,
                                                      const long long *__restrict__ word_off,
                                                      uint32_t *__restrict__ A, uint32_t *__restrict__ D) {
    __shared__ long long ta[MARK_SLOTS], td[MARK_SLOTS];
    __shared__ uint32_t ba[MARK_SLOTS], bd[MARK_SLOTS];
    mark_init(ta, ba);
    mark_init(td, bd);
    const int64_t c0 = (int64_t)blockIdx.x * MARK_CH, c1 = min(n, c0 + MARK_CH);
    for (int64_t base = c0; base < c1; base += blockDim.x) {      // same trip count for every lane
        const int64_t r = base + threadIdx.x;
        long long wa = -1, wd = -1;
        uint32_t bit = 0;
        if (r < c1 && f[r] == JH_F_ADD) {
            const int64_t ty = type[r];
            const int64_t k = key ? key[r] : 0;
            if ((ty == T_INVOKE || ty == T_OK) && k >= 0 && keys[k].tier == 2) {
                const uint64_t b = (uint64_t)(val[r] - keys[k].vmin);
                const long long w = word_off[k] + (long long)(b >> 5);
                bit = 1u << (b & 31);
                if (ty == T_INVOKE) wa = w; else wd = w;
            }
        }
        mark_bits(A, ta, ba, wa, bit);
        mark_bits(D, td, bd, wd, bit);
    }
    mark_flush(A, ta, ba);
    mark_flush(D, td, bd);
}

// Global tier, final reads: workgroup (x, y) takes chunk x of the reads of the
// keys y, y + gridDim.y, ...
__global__ void __launch_bounds__(256) k_si_mark_read(const SiKey *__restrict__ keys, int64_t K,
                                                      const int64_t *__restrict__ aux,
                                                      const long long *__restrict__ word_off, uint32_t *__restrict__ R) {
    __shared__ long long tr[MARK_SLOTS];
    __shared__ uint32_t br[MARK_SLOTS];
    for (int64_t k = blockIdx.y; k < K; k += gridDim.y) {
        const SiKey &kr = keys[k];
        const int64_t c0 = (int64_t)blockIdx.x * MARK_CH, c1 = min((int64_t)kr.rcnt, c0 + MARK_CH);
        if (kr.tier != 2 || c0 >= c1) continue;            // (the same for every thread)
        mark_init(tr, br);
        const long long wo = word_off[k], vmin = kr.vmin, ro = kr.roff;
        for (int64_t base = c0; base < c1; base += blockDim.x) {
            const int64_t i = base + threadIdx.x;
            long long w = -1;
            uint32_t bit = 0;
            if (i < c1) {
                const uint64_t b = (uint64_t)(aux[ro + i] - vmin);
                w = wo + (long long)(b >> 5);
                bit = 1u << (b & 31);
            }
            mark_bits(R, tr, br, w, bit);
        }
        mark_flush(R, tr, br);
        __syncthreads();
    }
}

// the key that owns word w: the last k with word_off[k] <= w (a key without
// words shares its offset with its successor and is never the last such k)
__device__ __forceinline__ int64_t si_key_of(const long long *__restrict__ word_off, int64_t K, long long w) {
    int64_t a = 0, b = K;               // word_off[a] <= w < word_off[b]
    while (b - a > 1) {
        const int64_t mid = (a + b) >> 1;
        if (word_off[mid] <= w) a = mid; else b = mid;
    }
    return a;
}

// Global tier, words: each workgroup takes SI_CHUNK consecutive words, writes
// the four result words of those that belong to a global-tier key and adds up
// the six counts per key: in LDS for the first SI_TAB keys of its chunk (a
// global-tier key is wider than a chunk unless the tier is forced), then one
// atomic per key and counter per workgroup.
__global__ void __launch_bounds__(256) k_si_words(SiKey *keys, int64_t K, const long long *__restrict__ word_off,
                                                  int64_t total, const uint32_t *__restrict__ A,
                                                  const uint32_t *__restrict__ D, const uint32_t *__restrict__ R,
                                                  uint32_t *__restrict__ outb) {
    __shared__ uint32_t tab[SI_TAB][6];
    __shared__ long long s_k0;
    const int tid = threadIdx.x;
    const int64_t w0 = (int64_t)blockIdx.x * SI_CHUNK;
    if (tid < SI_TAB * 6) tab[tid / 6][tid % 6] = 0;
    if (tid == 0) s_k0 = si_key_of(word_off, K, w0);
    __syncthreads();
    const int64_t k0 = s_k0;
    int64_t kc = -1, kend = -1;         // the current key and the end of its words
    bool kg = false;
    uint32_t c[6] = {0, 0, 0, 0, 0, 0};
    auto flush = [&]() {
        if (kc >= 0 && kg) {
#pragma unroll
            for (int q = 0; q < 6; q++) {
                if (!c[q]) continue;
                if (kc - k0 < SI_TAB) atomicAdd(&tab[kc - k0][q], c[q]);
                else atomicAdd(&keys[kc].cnt[q], (unsigned long long)c[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < 6; q++) c[q] = 0;
    };
    for (int i = 0; i < SI_CHUNK / 256; i++) {
        const int64_t w = w0 + i * 256 + tid;
        if (w >= total) break;
        if (w >= kend) {
            flush();
            kc = si_key_of(word_off, K, w);
            kend = word_off[kc + 1];
            kg = keys[kc].tier == 2;
        }
        if (!kg) continue;
        const uint32_t a = A[w], d = D[w], r = R[w];
        uint32_t x[4];
        set_algebra(a, d, r, x);
        c[0] += __popc(a); c[1] += __popc(d);
        c[2] += __popc(x[0]); c[3] += __popc(x[1]); c[4] += __popc(x[3]); c[5] += __popc(x[2]);
#pragma unroll
        for (int s = 0; s < 4; s++) outb[s * total + w] = x[s];
    }
    flush();
    __syncthreads();
    if (tid < SI_TAB * 6) {
        const int64_t k = k0 + tid / 6;
        const uint32_t v = tab[tid / 6][tid % 6];
        if (v && k < K) atomicAdd(&keys[k].cnt[tid % 6], (unsigned long long)v);
    }
}

// Global tier: the smallest row of an :ok :add whose element the final read lacks
__global__ void __launch_bounds__(256) k_si_first_lost(const int64_t *__restrict__ type, const int64_t *__restrict__ f,
                                                       const int64_t *__restrict__ key, const int64_t *__restrict__ val,
                                                       int64_t n, SiKey *keys, const long long *__restrict__ word_off,
                                                       const uint32_t *__restrict__ R) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        if (f[r] != JH_F_ADD || type[r] != T_OK) continue;
        const int64_t k = key ? key[r] : 0;
        if (k < 0 || keys[k].tier != 2) continue;
        const uint64_t b = (uint64_t)(val[r] - keys[k].vmin);
        if ((R[word_off[k] + (long long)(b >> 5)] >> (b & 31)) & 1) continue;
        if ((unsigned long long)r < *(volatile unsigned long long *)&keys[k].first_lost)
            atomicMin(&keys[k].first_lost, (unsigned long long)r);
    }
}

__global__ void k_si_finish(const SiKey *__restrict__ keys, int64_t K, const uint32_t *__restrict__ off, int64_t n,
                            const long long *__restrict__ word_off, jh_set_key *__restrict__ out) {
    const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (k >= K) return;
    const SiKey &kr = keys[k];
    jh_set_key o;
    memset(&o, 0, sizeof o);
    o.valid = JH_VALID; o.cause = JH_CAUSE_NONE;
    o.rows = off ? (int64_t)off[k + 1] - (int64_t)off[k] : n;
    o.first_fail_entry = -1;
    o.final_read_entry = kr.final_row;
    o.word_off = word_off[k];
    if (kr.unknown) { o.valid = JH_UNKNOWN; o.cause = JH_CAUSE_NIL_VALUE; }
    else if (kr.tier) {
        o.attempt_count = (int64_t)kr.cnt[0]; o.acknowledged_count = (int64_t)kr.cnt[1];
        o.ok_count = (int64_t)kr.cnt[2]; o.lost_count = (int64_t)kr.cnt[3];
        o.recovered_count = (int64_t)kr.cnt[4]; o.unexpected_count = (int64_t)kr.cnt[5];
        o.valid = kr.cnt[3] == 0 && kr.cnt[5] == 0 ? JH_VALID : JH_INVALID;
        if (kr.cnt[3]) o.first_fail_entry = kr.first_lost == SI_NONE ? -1 : (int64_t)kr.first_lost;
        else if (kr.cnt[5]) o.first_fail_entry = kr.final_row;
        o.base = kr.vmin; o.n_words = kr.n_words;
    }
    out[k] = o;
}
}  // namespace

void set_independent_check(jh_ctx *ctx, const jh_history *dh, const jh_set_indep_opts *opts, jh_set_indep_result *res,
                           jh_set_key *keys_out, uint32_t *bits_out[4], int64_t words_cap, hipStream_t st) {
    memset(res, 0, sizeof *res);
    res->valid = JH_VALID; res->cause = JH_CAUSE_NONE;
    res->first_fail_entry = -1;
    const int64_t n = dh->n;
    const bool keyed = dh->key != nullptr && dh->n_keys > 0;
    const int64_t K = keyed ? dh->n_keys : 1;
    if (K >= (1LL << 31) - 2) throw_jh(JH_EUNSUPPORTED, "set-independent: more than 2^31 - 3 keys");
    if (n >= (1LL << 31)) throw_jh(JH_EUNSUPPORTED, "set-independent: 2^31 rows or more");
    std::vector<jh_set_key> own;
    if (!keys_out) { own.resize((size_t)K); keys_out = own.data(); }
    if (n == 0) {                                            // no key is in any row
        for (int64_t k = 0; k < K; k++) {
            memset(&keys_out[k], 0, sizeof(jh_set_key));
            keys_out[k].valid = JH_VALID;
            keys_out[k].first_fail_entry = keys_out[k].final_read_entry = -1;
        }
        if (!keyed) { keys_out[0].valid = JH_UNKNOWN; keys_out[0].cause = JH_CAUSE_NIL_VALUE; }
        return;
    }
    DeviceTimer timer{ctx, st};
    timer.start();

    // 1. per-key metadata
    SiKey *keys = ctx->ws<SiKey>(WS_SI_KEYS, K);
    SiMeta *m = ctx->ws<SiMeta>(WS_SI_META, 1);
    long long *nw = ctx->ws<long long>(WS_SI_WORDS, 2 * (K + 1)), *word_off = nw + K + 1;
    k_si_init<<<grid_for(K, 256), 256, 0, st>>>(keys, K, nw, m);
    const int vec = ((uintptr_t)dh->type | (uintptr_t)dh->f | (uintptr_t)dh->value | (uintptr_t)(keyed ? dh->key : nullptr)) % 16 == 0;
    k_si_meta<<<grid_for((n + 1) / 2, 256, 8192), 256, 0, st>>>(dh->type, dh->f, dh->key, dh->value, n, K, keyed ? 1 : 0,
                                                               vec, keys, m);
    const uint32_t *rows = nullptr, *off = nullptr;
    if (keyed) key_partition_device(ctx, dh, &rows, &off, st);
    const int gk = grid_for(K, 1, 1 << 20);
    k_si_range<<<gk, 256, 0, st>>>(keys, K, off, n, dh->value, dh->value2, dh->aux, dh->n_aux, opts->path, nw, m);
    excl_sum(ctx, WS_SI_TMP, as_input(nw), word_off, (int)(K + 1), st);
    long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, word_off + K, sizeof total, hipMemcpyDeviceToHost, st));
    const SiMeta mh = fetch(m, st);
    if (mh.flags & SI_BAD_KEY) throw_jh(JH_EINVAL, "set-independent: a key outside [0, n_keys)");
    if (mh.flags & SI_UNSUP_KEY)
        throw_jh(JH_EUNSUPPORTED, "set-independent: an :add or an :ok :read without a key in a keyed history");
    if (mh.flags & SI_NIL_ADD) throw_jh(JH_EUNSUPPORTED, "set-independent: a nil :add element");
    if (mh.flags & SI_BAD_RANGE)
        throw_jh(JH_EINVAL, "set-independent: a final read's range leaves [0, n_aux) or has a negative count");
    if (mh.flags & SI_UNSUP_SPAN) throw_jh(JH_EUNSUPPORTED, "set-independent: a key's elements span more than 2^34");
    if (total > JH_SI_WORDS_MAX) throw_jh(JH_EUNSUPPORTED, "set-independent: more than JH_SI_WORDS_MAX bitmap words");
    if (mh.flags & SI_OVER) throw_jh(JH_EINVAL, "set-independent on-chip path: a key wider than JH_SI_LDS_SPAN");

    // 2. the keys
    uint32_t *outb = ctx->ws<uint32_t>(WS_SI_OUT, 4 * (size_t)total);
    const bool global = mh.n_global > 0;
    if (mh.n_global < K)
        k_si_lds<<<gk, 256, 0, st>>>(keys, K, off, rows, n, dh->type, dh->f, dh->value, dh->aux, word_off, total, outb);
    if (global) {
        uint32_t *bits = ctx->ws<uint32_t>(WS_SI_BITS, 3 * (size_t)total);
        uint32_t *A = bits, *D = bits + total, *R = bits + 2 * total;
        HIP_TRY(hipMemsetAsync(bits, 0, sizeof(uint32_t) * 3 * (size_t)total, st));
        const int64_t *kcol = keyed ? dh->key : nullptr;
        k_si_mark_rows<<<(unsigned)((n + MARK_CH - 1) / MARK_CH), 256, 0, st>>>(dh->type, dh->f, kcol, dh->value, n, keys,
                                                                               word_off, A, D);
        if (mh.max_gcnt > 0) {
            const dim3 g((unsigned)((mh.max_gcnt + MARK_CH - 1) / MARK_CH), (unsigned)std::min<int64_t>(K, 65535));
            k_si_mark_read<<<g, 256, 0, st>>>(keys, K, dh->aux, word_off, R);
        }
        k_si_words<<<(unsigned)((total + SI_CHUNK - 1) / SI_CHUNK), 256, 0, st>>>(keys, K, word_off, total, A, D, R, outb);
        k_si_first_lost<<<grid_for(n, 256, 16384), 256, 0, st>>>(dh->type, dh->f, kcol, dh->value, n, keys, word_off, R);
    }

    // 3. the records and the bitmaps
    jh_set_key *recs = ctx->ws<jh_set_key>(WS_SI_RECS, K);
    k_si_finish<<<grid_for(K, 256), 256, 0, st>>>(keys, K, off, n, word_off, recs);
    HIP_TRY(hipMemcpyAsync(keys_out, recs, sizeof(jh_set_key) * K, hipMemcpyDeviceToHost, st));
    const int64_t kw = std::min<int64_t>(total, std::max<int64_t>(words_cap, 0));
    for (int s = 0; s < 4; s++)
        if (kw > 0 && bits_out[s])
            HIP_TRY(hipMemcpyAsync(bits_out[s], outb + (int64_t)s * total, sizeof(uint32_t) * kw, hipMemcpyDeviceToHost, st));
    res->device_ms = timer.stop();                           // (the stream is drained here)
    int64_t judged = 0;
    for (int64_t k = 0; k < K; k++) {
        const jh_set_key &o = keys_out[k];
        if (o.rows == 0) continue;
        if (o.valid == JH_VALID) res->keys_valid++;
        else if (o.valid == JH_INVALID) res->keys_invalid++;
        else res->keys_unknown++;
        if (o.valid != JH_UNKNOWN) judged++;
        if (o.first_fail_entry >= 0 && (res->first_fail_entry < 0 || o.first_fail_entry < res->first_fail_entry))
            res->first_fail_entry = o.first_fail_entry;
    }
    if (res->keys_invalid) res->valid = JH_INVALID;
    else if (res->keys_unknown) { res->valid = JH_UNKNOWN; res->cause = JH_CAUSE_NIL_VALUE; }
    res->path = judged == 0 ? 0 : global ? 2 : 1;
    res->total_words = total;
    res->entries = n + (int64_t)mh.read_elems;
}
