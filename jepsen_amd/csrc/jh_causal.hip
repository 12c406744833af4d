// jh_causal.hip -- the causal-reverse ("sequential") workload checker on MI355X.
//
// jepsen.tests.causal-reverse/checker lifted by independent/checker,
// jepsen/src/jepsen/tests/causal_reverse.clj:21-84, batched over the keys. The
// reference's snapshots `expected[w]` are nested prefixes of the key's
// completion order, so per key (include/jh.h):
//   last_inv[v]  the last :invoke :write of v     first_ok[v]  its first :ok
//   a read of the set S:  M = max last_inv[w], w in S and invoked (none: -1)
//                         expected = {v : first_ok[v] < M}, c = |expected| =
//                         the rank of M in the completion order
//                         missing = expected - S
// Positions are indices into the key's own write list (history order), which
// compare like rows.
//
// Pipeline:
//   1. k_cr_flag      type / f: the :invoke / :ok write rows and the :ok read
//                     rows as ballot words (word j = rows 64 j .. 64 j + 63) and
//                     their numbers per 2048-row tile; exclusive scans (the
//                     host side and the per-wave prefix are row_select.h)
//      k_cr_compact   the flagged rows in history order from the ballot words
//                     (no atomic): writes as (key | ok << 31, value), reads as
//                     (key, row, first element, count), ranges bounds-checked
//   2. buckets        stable radix sorts on the key bits alone (writes carry
//                     their value, reads a permutation), k_cr_bounds: per-key
//                     offsets by binary search
//   3. k_cr_key<LDS>  one workgroup per key. It builds the key's value table
//                     (open addressing on the value: last_inv, first_ok, rank
//                     of first_ok) and the completion-order list, then one wave
//                     per read: a coalesced pass over the elements reduces
//                     c = rank(M) (each value's slot holds the rank of its
//                     last_inv) and keeps each element's rank in registers (the
//                     first 256 elements), the ranks < c are marked in a
//                     per-wave bitmap, missing_count = c - popcount.
//                     LDS = true: table and bitmaps in LDS, at most
//                     JH_CR_LDS_VALUES distinct values; a key that has more
//                     marks itself for the global tier. LDS = false: the same
//                     code, table and bitmaps in a per-key slice of HBM scratch.
//   4. exact order    exclusive sums over the failing reads (error index,
//                     missing offset), k_cr_emit writes the error rows;
//                     k_cr_key<LIST> reruns the failing reads of the invalid
//                     keys and lists the clear bits, one segmented radix sort
//                     puts each read's values in ascending order.
#include "row_select.h"

namespace {
constexpr int C_STEPS = 8;                    // rows per thread per tile
constexpr int C_TILE = 256 * C_STEPS;         // rows per tile (2048)
constexpr int C_WORDS = C_TILE / 64;          // ballot words per tile and kind (32)
constexpr int CAP = JH_CR_LDS_VALUES;         // distinct values of an on-chip key
constexpr int SLOTS = 2 * CAP;                // its table's slots (load <= 1/2; + 512 in flight < SLOTS)
constexpr int BMW = CAP / 32;                 // bitmap words per wave
constexpr int KT = 512, NW = KT / 64;         // threads and waves of a key's workgroup
constexpr int REG_STEPS = 4;                  // 64 * REG_STEPS elements of a read stay in registers
constexpr unsigned OKBIT = 1u << 31, KEYMASK = OKBIT - 1;
constexpr unsigned long long NONE = ~0ULL;
constexpr long long C_MAX_COUNT = 0x7ffffffeLL;
constexpr int NO_RANK = 0x7fffffff;

struct CMeta {
    unsigned bad_range, bad_key, unsup_key, unsup_nil, n_over, pad;
    unsigned long long entries, invalid_keys, first_err, list_end, n_seg;
};

__global__ void k_cr_meta_init(CMeta *m) {
    memset(m, 0, sizeof *m);
    m->first_err = NONE;
}

// ---------------------------------------------------------------------------
// 1. Tile = 256 threads x C_STEPS rows, row tile * 2048 + u * 256 + thread: the
// ballot of wave w at step u is word tile * 32 + u * 4 + w, i.e. rows 64 j ..
__global__ void __launch_bounds__(256) k_cr_flag(const int64_t *__restrict__ type, const int64_t *__restrict__ f,
                                                 int64_t n, unsigned long long *__restrict__ words_r,
                                                 unsigned long long *__restrict__ words_w,
                                                 long long *__restrict__ cnt_r, long long *__restrict__ cnt_w) {
    __shared__ unsigned sh[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_tiles = (n + C_TILE - 1) / C_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        unsigned cr = 0, cw = 0;
#pragma unroll
        for (int u = 0; u < C_STEPS; u++) {
            const int64_t row = tile * C_TILE + u * 256 + threadIdx.x;
            const bool in = row < n;
            const int64_t t = in ? type[row] : -1, ff = in ? f[row] : -1;
            const unsigned long long br = __ballot(t == T_OK && ff == JH_F_READ);
            const unsigned long long bw = __ballot((t == T_OK || t == T_INVOKE) && ff == JH_F_WRITE);
            cr += __popcll(br);
            cw += __popcll(bw);
            if (lane == 0) {
                words_r[tile * C_WORDS + u * 4 + wave] = br;
                words_w[tile * C_WORDS + u * 4 + wave] = bw;
            }
        }
        if (lane == 0) { sh[wave] = cr; sh[4 + wave] = cw; }
        __syncthreads();
        if (threadIdx.x == 0) {
            cnt_r[tile] = (long long)(sh[0] + sh[1] + sh[2] + sh[3]);
            cnt_w[tile] = (long long)(sh[4] + sh[5] + sh[6] + sh[7]);
        }
        __syncthreads();
    }
}

// The flagged rows of one kind, in history order: every wave scans the tile's
// 32 ballot words itself; the exclusive prefix of their popcounts at word
// u * 4 + wave is where the wave's rows of step u go.
// WR = 1: writes -> a32[o] = key | ok << 31, b[o] = value.
// WR = 0: reads  -> a32[o] = key, b[o] = row, c[o] = first element, d[o] = count.
// K = 0: an un-keyed history (key 0 for every row).
template <int WR>
__global__ void __launch_bounds__(256) k_cr_compact(const int64_t *__restrict__ type, const int64_t *__restrict__ key,
                                                    const int64_t *__restrict__ value,
                                                    const int64_t *__restrict__ value2, int64_t n, int64_t K,
                                                    int64_t n_aux, const unsigned long long *__restrict__ words,
                                                    const long long *__restrict__ tile_base,
                                                    uint32_t *__restrict__ a32, int64_t *__restrict__ b,
                                                    int64_t *__restrict__ c, int64_t *__restrict__ d, CMeta *m) {
    __shared__ unsigned long long shr[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt = (1ULL << lane) - 1;
    const int64_t n_tiles = (n + C_TILE - 1) / C_TILE;
    unsigned long long ent = 0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        unsigned long long w;
        unsigned excl;
        if (rs_word_prefix<C_WORDS>(words + tile * C_WORDS, lane, w, excl) == 0) continue;   // no such row in this tile
        const long long base = tile_base[tile];
#pragma unroll
        for (int u = 0; u < C_STEPS; u++) {
            const int wi = u * 4 + wave;
            const unsigned long long bits = __shfl(w, wi);
            const unsigned at = __shfl(excl, wi);
            if (!((bits >> lane) & 1)) continue;              // nothing below is cross-lane
            const int64_t row = tile * C_TILE + wi * 64 + lane;
            const long long o = base + at + __popcll(bits & lt);
            unsigned k = 0;
            if (K > 0) {
                const int64_t kk = key[row];
                if (kk < 0) atomicOr(&m->unsup_key, 1u);
                else if (kk >= K) atomicOr(&m->bad_key, 1u);
                else k = (unsigned)kk;
            }
            long long v = value[row];
            if (WR) {
                if (v == JH_NIL) atomicOr(&m->unsup_nil, 1u);
                a32[o] = k | (type[row] == T_OK ? OKBIT : 0u);
                b[o] = v;
            } else {
                long long cc = value2[row];
                if (cc == 0) v = 0;                           // nil or empty: value is not looked at
                else if (cc < 0 || v < 0 || v > n_aux || cc > n_aux - v) { atomicOr(&m->bad_range, 1u); v = 0; cc = 0; }
                a32[o] = k; b[o] = row; c[o] = v; d[o] = cc;
                ent += (unsigned long long)cc;
            }
        }
    }
    if (!WR) {
        ent = block_reduce256(ent, RedSum(), shr);
        if (threadIdx.x == 0 && ent) atomicAdd(&m->entries, ent);
    }
}

// ---------------------------------------------------------------------------
// 2. buckets
__global__ void __launch_bounds__(256) k_cr_iota(uint32_t *__restrict__ p, int64_t cnt) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = (uint32_t)i;
}

// off[k] = the number of sorted items whose key is below k, k = 0 .. K
__global__ void __launch_bounds__(256) k_cr_bounds(const uint32_t *__restrict__ keys, int64_t cnt, int64_t K,
                                                   int32_t *__restrict__ off) {
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k <= K; k += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = cnt;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)(keys[mid] & KEYMASK) < k) lo = mid + 1;
            else hi = mid;
        }
        off[k] = (int32_t)lo;
    }
}

// ---------------------------------------------------------------------------
// 3. The global tier's slice of scratch for a key of W write rows: a table of
// S = 2^ceil(log2(2 W)) >= 64 slots (value 8 B, last_inv / first_ok / rank 4 B
// each), the completion list (index 4 B, value 8 B, W entries) and one bitmap
// of W bits per wave, every part a multiple of 8 bytes.
__host__ __device__ inline long long cr_slots(long long W) {
    long long s = 64;
    while (s < 2 * W) s <<= 1;
    return s;
}
__host__ __device__ inline long long cr_even(long long x) { return (x + 1) & ~1LL; }
__host__ __device__ inline long long cr_bytes(long long W) {
    return cr_slots(W) * 20 + cr_even(W) * 12 + 8 /* NW */ * cr_even((W + 31) / 32) * 4;
}

__global__ void __launch_bounds__(256) k_cr_sizes(const int32_t *__restrict__ woff, const uint8_t *__restrict__ tier,
                                                  int64_t K, long long *__restrict__ bytes) {
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k <= K; k += (int64_t)gridDim.x * blockDim.x)
        bytes[k] = k < K && tier[k] == 2 ? cr_bytes(woff[k + 1] - woff[k]) : 0;
}

template <bool LDS, class T>
__device__ __forceinline__ T cr_ld(const T *p) {
    // the table is written by this workgroup's atomics: LDS reads see them; the
    // global tier reads past the CU's L1, which atomics (done in L2) do not update
    if constexpr (LDS) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS>
__device__ __forceinline__ void cr_sync() {
    if (!LDS) __threadfence();          // the workgroup's stores and atomics to HBM have landed
    __syncthreads();
}

template <bool LDS>
__device__ __forceinline__ int cr_find(const long long *vals, unsigned mask, long long v) {
    if (v == JH_NIL) return -1;
    unsigned h = (unsigned)jh_mix64((uint64_t)v) & mask;
    for (;;) {
        const long long cur = cr_ld<LDS>(vals + h);
        if (cur == v) return (int)h;
        if (cur == JH_NIL) return -1;
        h = (h + 1) & mask;
    }
}

// the slot of v, claimed if v is new (*n_distinct counts the claims); there is
// always a free slot: at most CAP + 512 (LDS) / W (global) values are inserted
template <bool LDS>
__device__ __forceinline__ int cr_insert(long long *vals, unsigned mask, long long v, int *n_distinct) {
    unsigned h = (unsigned)jh_mix64((uint64_t)v) & mask;
    for (;;) {
        long long cur = cr_ld<LDS>(vals + h);
        if (cur == JH_NIL) {
            cur = (long long)atomicCAS((unsigned long long *)(vals + h), (unsigned long long)JH_NIL, (unsigned long long)v);
            if (cur == JH_NIL) { atomicAdd(n_distinct, 1); return (int)h; }
        }
        if (cur == v) return (int)h;
        h = (h + 1) & mask;
    }
}

// One workgroup of KT threads per key of its tier (LDS: tier 1, else tier 2).
// LIST = false: judge every read of the key: exp[j] = c, miss[j] = the missing
// count and eflag[j] = (miss[j] > 0) at the read's index j in history order,
// kv[k], the meta's invalid_keys / first_err. A key of more than CAP distinct
// values (LDS only) moves itself to tier 2 instead.
// LIST = true: only the failing reads of invalid keys whose missing offset
// moff[j] is below list_cap: the values of the clear bits, in completion order,
// to mbuf[moff[j] ..].
// Per slot, lr = (last_inv, rank of first_ok); once the ranks are known last_inv
// is replaced by the number of completions before it, so a read needs one
// 8-byte word per element: c = the max of the first halves, and the second
// halves below c are marked.
template <bool LDS, bool LIST>
__global__ void __launch_bounds__(KT, 6) k_cr_key(const int32_t *__restrict__ woff, const int32_t *__restrict__ roff,
                                              const uint32_t *__restrict__ wk, const int64_t *__restrict__ wv,
                                              const uint32_t *__restrict__ rperm, const int64_t *__restrict__ rrow,
                                              const int64_t *__restrict__ rstart, const int64_t *__restrict__ rcnt,
                                              const int64_t *__restrict__ aux, int64_t K, uint8_t *__restrict__ tier,
                                              char *__restrict__ scratch, const long long *__restrict__ soff,
                                              int32_t *__restrict__ kv, int32_t *__restrict__ exp,
                                              long long *__restrict__ miss, long long *__restrict__ eflag,
                                              const long long *__restrict__ moff, long long list_cap,
                                              long long *__restrict__ mbuf, CMeta *m) {
    __shared__ long long s_vals[LDS ? SLOTS : 1];
    __shared__ int2 s_lr[LDS ? SLOTS : 1];
    __shared__ int s_fok[LDS ? SLOTS : 1];
    __shared__ int s_cidx[LDS ? CAP : 1];
    __shared__ long long s_cval[LDS && LIST ? CAP : 1];
    __shared__ unsigned s_bm[LDS ? NW * BMW : 1];
    __shared__ int s_cnt, s_err, s_w[NW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt = (1ULL << lane) - 1;
    for (int64_t k = blockIdx.x; k < K; k += gridDim.x) {     // everything that branches here is block-uniform
        if (tier[k] != (LDS ? 1 : 2)) continue;
        if (LIST && kv[k] != JH_INVALID) continue;
        const int w0 = woff[k], W = woff[k + 1] - w0, r0 = roff[k], r1 = roff[k + 1];
        long long *vals, *cval;
        int2 *lr;
        int *fok, *cidx;
        unsigned *bm;
        unsigned mask;
        int bmw;
        if constexpr (LDS) {
            vals = s_vals; lr = s_lr; fok = s_fok; cidx = s_cidx; cval = s_cval; bm = s_bm;
            mask = SLOTS - 1; bmw = BMW;
        } else {
            const long long S = cr_slots(W), We = cr_even(W);
            char *p = scratch + soff[k];
            vals = (long long *)p; p += S * 8;
            cval = (long long *)p; p += We * 8;
            lr = (int2 *)p; p += S * 8;
            fok = (int *)p; p += S * 4;
            cidx = (int *)p; p += We * 4;
            bm = (unsigned *)p;
            mask = (unsigned)(S - 1); bmw = (int)cr_even((W + 31) / 32);
        }
        __syncthreads();                                      // the last key's readers of s_cnt / s_err are done
        for (unsigned s = threadIdx.x; s <= mask; s += KT) { vals[s] = JH_NIL; lr[s] = make_int2(-1, NO_RANK); fok[s] = NO_RANK; }
        for (int s = threadIdx.x; s < NW * bmw; s += KT) bm[s] = 0;
        if (threadIdx.x == 0) { s_cnt = 0; s_err = 0; }
        cr_sync<LDS>();

        // the table: last_inv = max, first_ok = min of the positions in the key's write list
        bool over = false;
        for (int b0 = 0; b0 < W; b0 += KT) {
            const int i = b0 + threadIdx.x;
            if (i < W) {
                const long long v = wv[w0 + i];
                if (v != JH_NIL) {                            // (a nil write: the call ends JH_EUNSUPPORTED)
                    const int s = cr_insert<LDS>(vals, mask, v, &s_cnt);
                    if (wk[w0 + i] & OKBIT) atomicMin(&fok[s], i);
                    else atomicMax(&lr[s].x, i);
                }
            }
            cr_sync<LDS>();
            over = LDS && s_cnt > CAP;
            __syncthreads();                                  // everyone has read s_cnt before the next inserts
            if (over) break;
        }
        if (over) {
            if (threadIdx.x == 0) { tier[k] = 2; atomicAdd(&m->n_over, 1u); }
            continue;
        }

        // ranks: the first :ok of each value, in position order
        int n_comp = 0;
        for (int b0 = 0; b0 < W; b0 += KT) {
            const int i = b0 + threadIdx.x;
            int s = -1;
            long long v = JH_NIL;
            if (i < W && (wk[w0 + i] & OKBIT)) {
                v = wv[w0 + i];
                s = cr_find<LDS>(vals, mask, v);
                if (s >= 0 && cr_ld<LDS>(fok + s) != i) s = -1;
            }
            const unsigned long long bal = __ballot(s >= 0);
            if (lane == 0) s_w[wave] = __popcll(bal);
            __syncthreads();
            int before = n_comp;
#pragma unroll
            for (int q = 0; q < NW; q++) {
                if (q < wave) before += s_w[q];
                n_comp += s_w[q];
            }
            if (s >= 0) {
                const int r = before + __popcll(bal & lt);
                lr[s].y = r; cidx[r] = i;
                if (!LDS || LIST) cval[r] = v;
            }
            __syncthreads();                                  // s_w is read before the next step writes it
        }
        cr_sync<LDS>();
        // last_inv -> the completions before it (what a read of this value expects)
        for (unsigned s = threadIdx.x; s <= mask; s += KT) {
            if (cr_ld<LDS>(vals + s) == JH_NIL) continue;
            const int li = cr_ld<LDS>(&lr[s].x);
            int c = 0;
            for (int hi = n_comp; c < hi;) {
                const int mid = (c + hi) >> 1;
                if (cr_ld<LDS>(cidx + mid) < li) c = mid + 1;
                else hi = mid;
            }
            lr[s].x = c;
        }
        cr_sync<LDS>();

        // the reads: one wave each; the next read's elements are loaded while this one is marked and counted
        unsigned *wbm = bm + wave * bmw;
        int p = r0 + wave;
        int64_t j = 0, cnt = 0;
        const int64_t *el = aux;
        long long at = 0, ev[REG_STEPS];
        auto fetch = [&](int q) {                             // wave-uniform
            j = rperm ? rperm[q] : q;
            cnt = rcnt[j];
            el = aux + rstart[j];
            if (LIST) { at = moff[j]; if (miss[j] == 0 || at >= list_cap) cnt = -1; }
#pragma unroll
            for (int u = 0; u < REG_STEPS; u++) ev[u] = lane + 64 * u < cnt ? el[lane + 64 * u] : JH_NIL;
        };
        if (p < r1) fetch(p);
        while (p < r1) {
            const int64_t cj = j, ccnt = cnt;
            const int64_t *cel = el;
            const long long cat = at;
            const bool skip = LIST && ccnt < 0;
            int c = 0, reg[REG_STEPS];
#pragma unroll
            for (int u = 0; u < REG_STEPS; u++) {
                reg[u] = NO_RANK;
                const int s = skip ? -1 : cr_find<LDS>(vals, mask, ev[u]);
                if (s >= 0) {
                    const long long x = cr_ld<LDS>((const long long *)(lr + s));
                    c = max(c, (int)(unsigned)x); reg[u] = (int)(x >> 32);
                }
            }
            for (int64_t e = 64 * REG_STEPS + lane; e < ccnt; e += 64) {
                const int s = cr_find<LDS>(vals, mask, cel[e]);
                if (s >= 0) c = max(c, cr_ld<LDS>(&lr[s].x));
            }
            p += NW;                                          // the lookups are done: ev is free for the next read
            if (p < r1) fetch(p);
            if (skip) continue;
            for (int o = 32; o > 0; o >>= 1) c = max(c, __shfl_xor(c, o));
            long long n_miss = 0;
            if (c > 0) {
#pragma unroll
                for (int u = 0; u < REG_STEPS; u++)
                    if (reg[u] < c) atomicOr(&wbm[reg[u] >> 5], 1u << (reg[u] & 31));
                for (int64_t e = 64 * REG_STEPS + lane; e < ccnt; e += 64) {
                    const int s = cr_find<LDS>(vals, mask, cel[e]);
                    const int r = s >= 0 ? cr_ld<LDS>(&lr[s].y) : NO_RANK;
                    if (r < c) atomicOr(&wbm[r >> 5], 1u << (r & 31));
                }
                // the wave's marks land before its words are taken: LDS serves one wave's
                // instructions in order (only the compiler must not reorder them); HBM is fenced
                if (LDS) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                else __threadfence();
                const int words = (c + 31) >> 5;
                for (int d0 = 0; d0 < words; d0 += 64) {      // wave-uniform
                    const int d = d0 + lane;
                    unsigned clear = 0;
                    if (d < words) {
                        clear = ~atomicExch(&wbm[d], 0u);     // taken and cleared for the wave's next read
                        if (d == words - 1 && (c & 31)) clear &= (1u << (c & 31)) - 1;
                    }
                    int inc = __popc(clear);
                    const int own = inc;
                    if (LIST) {
#pragma unroll
                        for (int dd = 1; dd < 64; dd <<= 1) {
                            const int o = __shfl_up(inc, dd);
                            if (lane >= dd) inc += o;
                        }
                        long long o = cat + n_miss + (inc - own);
                        while (clear) {
                            const int bit = __ffs((int)clear) - 1;
                            clear &= clear - 1;
                            mbuf[o++] = cr_ld<LDS>(cval + (d * 32 + bit));
                        }
                        n_miss += __shfl(inc, 63);
                    } else {
                        for (int o = 32; o > 0; o >>= 1) inc += __shfl_xor(inc, o);
                        n_miss += inc;
                    }
                }
            }
            if (!LIST && lane == 0) {
                exp[cj] = c; miss[cj] = n_miss; eflag[cj] = n_miss > 0;
                if (n_miss > 0) { s_err = 1; atomicMin(&m->first_err, (unsigned long long)rrow[cj]); }
            }
        }
        if (!LIST) {
            __syncthreads();
            if (threadIdx.x == 0) {
                kv[k] = s_err ? JH_INVALID : JH_VALID;
                if (s_err) atomicAdd(&m->invalid_keys, 1ULL);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// 4. the error rows in history order; the segments of the missing list
__global__ void __launch_bounds__(256) k_cr_emit(const uint32_t *__restrict__ rkey, const int64_t *__restrict__ rrow,
                                                 const int32_t *__restrict__ exp, const long long *__restrict__ miss,
                                                 const long long *__restrict__ eidx, const long long *__restrict__ moff,
                                                 int64_t R, long long err_cap, long long list_cap,
                                                 int64_t *__restrict__ out, int32_t *__restrict__ seg_b,
                                                 int32_t *__restrict__ seg_e, CMeta *m) {
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < R; j += (int64_t)gridDim.x * blockDim.x) {
        const long long mc = miss[j];
        if (mc == 0) continue;
        const long long e = eidx[j], at = moff[j];
        if (e < err_cap) {
            int64_t *o = out + 5 * e;
            o[0] = rrow[j]; o[1] = rkey[j]; o[2] = exp[j]; o[3] = mc; o[4] = at;
        }
        if (at < list_cap) {
            seg_b[e] = (int32_t)at; seg_e[e] = (int32_t)(at + mc);
            atomicMax(&m->list_end, (unsigned long long)(at + mc));
            atomicMax(&m->n_seg, (unsigned long long)(e + 1));
        }
    }
}

__global__ void __launch_bounds__(256) k_cr_fill32(int32_t *__restrict__ p, int64_t cnt, int32_t v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

int bits_of(unsigned long long x) {
    int b = 1;
    while (b < 64 && (x >> b)) b++;
    return b;
}

}  // namespace

void causal_reverse_check(jh_ctx *ctx, const jh_history *dh, const jh_causal_reverse_opts *opts,
                          jh_causal_reverse_result *res, int32_t *key_valid, int64_t *errors_out, int64_t err_cap,
                          int64_t *missing_out, int64_t missing_cap, hipStream_t st) {
    memset(res, 0, sizeof *res);
    res->valid = JH_VALID;
    res->first_error_row = -1;
    const int64_t n = dh->n;
    const bool keyed = dh->key != nullptr && dh->n_keys > 0;
    const int64_t K = keyed ? dh->n_keys : 1, n_out = std::max<int64_t>(dh->n_keys, 1);
    if (key_valid) std::fill(key_valid, key_valid + n_out, (int32_t)JH_VALID);
    if (dh->n_aux < 0) throw_jh(JH_EINVAL, "causal-reverse: n_aux < 0");
    if (n == 0) return;
    if (K > (int64_t)KEYMASK) throw_jh(JH_EUNSUPPORTED, "causal-reverse: more than 2^31 - 1 keys");
    if (n > 0x7fffffff00LL) throw_jh(JH_EUNSUPPORTED, "causal-reverse: more than 2^39 rows");
    DeviceTimer timer{ctx, st};
    timer.start();

    // 1. the writes and the reads, in history order
    CMeta *m = ctx->ws<CMeta>(WS_CR_META, 1);
    k_cr_meta_init<<<1, 1, 0, st>>>(m);
    const RowSel<2> sel = select_rows<2>(
        ctx, {WS_CR_WORDS, WS_CR_TCNT, WS_CR_TBASE, WS_CR_TMP}, n, C_TILE, C_WORDS,
        [&](int g, unsigned long long *words, long long *tile_cnt) {      // kind 0: reads, kind 1: writes
            const int64_t n_tiles = (n + C_TILE - 1) / C_TILE;
            k_cr_flag<<<g, 256, 0, st>>>(dh->type, dh->f, n, words, words + n_tiles * C_WORDS, tile_cnt,
                                         tile_cnt + n_tiles + 1);
        }, st);
    const int g = sel.grid;
    const long long R = sel.count[0], W = sel.count[1];
    res->read_count = R;
    if (R > C_MAX_COUNT) throw_jh(JH_EUNSUPPORTED, "causal-reverse: more than 2^31 - 2 reads");
    if (W > C_MAX_COUNT) throw_jh(JH_EUNSUPPORTED, "causal-reverse: more than 2^31 - 2 writes");
    if (R > 0 && dh->n_aux > 0 && !dh->aux) throw_jh(JH_EINVAL, "causal-reverse: n_aux > 0 without aux");

    uint32_t *wkey = ctx->ws<uint32_t>(WS_CR_WKEY, 2 * W), *wkey_s = wkey + W;
    int64_t *wval = ctx->ws<int64_t>(WS_CR_WVAL, 2 * W), *wval_s = wval + W;
    uint32_t *rkey = ctx->ws<uint32_t>(WS_CR_RKEY, 2 * R), *rkey_s = rkey + R;
    uint32_t *rperm = ctx->ws<uint32_t>(WS_CR_RPERM, 2 * R), *rperm_s = rperm + R;
    int64_t *rrow = ctx->ws<int64_t>(WS_CR_RROW, 3 * R), *rstart = rrow + R, *rcnt = rrow + 2 * R;
    const int64_t Kc = keyed ? K : 0;
    if (W > 0)
        k_cr_compact<1><<<g, 256, 0, st>>>(dh->type, dh->key, dh->value, dh->value2, n, Kc, dh->n_aux, sel.words[1], sel.base[1],
                                           wkey, wval, nullptr, nullptr, m);
    if (R > 0)
        k_cr_compact<0><<<g, 256, 0, st>>>(dh->type, dh->key, dh->value, dh->value2, n, Kc, dh->n_aux, sel.words[0], sel.base[0],
                                           rkey, rrow, rstart, rcnt, m);
    CMeta mh = fetch(m, st);
    if (mh.bad_key) throw_jh(JH_EINVAL, "causal-reverse: a key outside [0, n_keys)");
    if (mh.bad_range) throw_jh(JH_EINVAL, "causal-reverse: a read's range leaves [0, n_aux) or has a negative count");
    if (mh.unsup_key)
        throw_jh(JH_EUNSUPPORTED, "causal-reverse: a write or an :ok read without a key in a keyed history");
    if (mh.unsup_nil) throw_jh(JH_EUNSUPPORTED, "causal-reverse: a write of nil");
    res->entries = (int64_t)mh.entries;

    // 2. buckets (one key: the compacted order is the bucket)
    const uint32_t *wk = wkey, *rp = nullptr;
    const int64_t *wv = wval;
    const uint32_t *rk_sorted = rkey;
    if (K > 1) {
        const int kb = bits_of((unsigned long long)(K - 1));
        if (W > 0) { sort_pairs(ctx, WS_CR_TMP, wkey, wkey_s, wval, wval_s, (int)W, kb, st); wk = wkey_s; wv = wval_s; }
        if (R > 0) {
            k_cr_iota<<<grid_for(R, 256, 2048), 256, 0, st>>>(rperm, R);
            sort_pairs(ctx, WS_CR_TMP, rkey, rkey_s, rperm, rperm_s, (int)R, kb, st);
            rp = rperm_s; rk_sorted = rkey_s;
        }
    }
    int32_t *woff = ctx->ws<int32_t>(WS_CR_OFF, 2 * (K + 1)), *roff = woff + K + 1;
    const int gk = grid_for(K + 1, 256, 2048);
    k_cr_bounds<<<gk, 256, 0, st>>>(wk, W, K, woff);
    k_cr_bounds<<<gk, 256, 0, st>>>(rk_sorted, R, K, roff);

    // 3. the keys
    int path = opts->path;
    uint8_t *tier = ctx->ws<uint8_t>(WS_CR_TIER, K);
    int32_t *kv = ctx->ws<int32_t>(WS_CR_KV, K);
    int32_t *exp = ctx->ws<int32_t>(WS_CR_EXP, R);
    long long *miss = ctx->ws<long long>(WS_CR_MISS, 4 * (R + 1));
    long long *eflag = miss + (R + 1), *moff = miss + 2 * (R + 1), *eidx = miss + 3 * (R + 1);
    HIP_TRY(hipMemsetAsync(tier, path == 2 ? 2 : 1, K, st));
    HIP_TRY(hipMemsetAsync(miss, 0, sizeof(long long) * 2 * (R + 1), st));
    HIP_TRY(hipMemsetAsync(exp, 0, sizeof(int32_t) * R, st));
    k_cr_fill32<<<grid_for(K, 256, 2048), 256, 0, st>>>(kv, K, JH_VALID);
    const int gkey = grid_for(K, 1, 65536);
    bool global = path == 2;
    if (path != 2) {
        k_cr_key<true, false><<<gkey, KT, 0, st>>>(woff, roff, wk, wv, rp, rrow, rstart, rcnt, dh->aux, K, tier, nullptr,
                                                   nullptr, kv, exp, miss, eflag, nullptr, 0, nullptr, m);
        mh = fetch(m, st);
        if (mh.n_over && path == 1)
            throw_jh(JH_EINVAL, "causal-reverse on-chip path: a key with more than JH_CR_LDS_VALUES distinct values");
        global = mh.n_over > 0;
    }
    char *scratch = nullptr;
    long long *soff = nullptr;
    if (global) {
        long long *sbytes = ctx->ws<long long>(WS_CR_SOFF, 2 * (K + 1));
        soff = sbytes + K + 1;
        k_cr_sizes<<<gk, 256, 0, st>>>(woff, tier, K, sbytes);
        excl_sum(ctx, WS_CR_TMP, as_input(sbytes), soff, (int)(K + 1), st);
        const long long total = fetch(soff + K, st);
        if (total > JH_CR_SCRATCH_MAX)
            throw_jh(JH_ENOMEM, "causal-reverse global tier: the value tables pass JH_CR_SCRATCH_MAX bytes");
        scratch = ctx->ws<char>(WS_CR_SCRATCH, (size_t)total);
        k_cr_key<false, false><<<gkey, KT, 0, st>>>(woff, roff, wk, wv, rp, rrow, rstart, rcnt, dh->aux, K, tier, scratch,
                                                    soff, kv, exp, miss, eflag, nullptr, 0, nullptr, m);
    }
    res->path = global ? 2 : 1;

    // 4. totals, and the outputs in history order
    excl_sum(ctx, WS_CR_TMP, as_input(eflag), eidx, (int)(R + 1), st);
    excl_sum(ctx, WS_CR_TMP, as_input(miss), moff, (int)(R + 1), st);
    long long E = 0, MT = 0;
    HIP_TRY(hipMemcpyAsync(&E, eidx + R, sizeof E, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&MT, moff + R, sizeof MT, hipMemcpyDeviceToHost, st));
    mh = fetch(m, st);
    res->error_count = E;
    res->missing_total = MT;
    res->invalid_keys = (int64_t)mh.invalid_keys;
    res->first_error_row = mh.first_err == NONE ? -1 : (int64_t)mh.first_err;
    res->valid = E > 0 ? JH_INVALID : JH_VALID;
    if (key_valid) HIP_TRY(hipMemcpyAsync(key_valid, kv, sizeof(int32_t) * K, hipMemcpyDeviceToHost, st));
    if (E == 0) {
        HIP_TRY(hipStreamSynchronize(st));
        res->device_ms = timer.stop();
        return;
    }
    const long long ecap = errors_out ? std::min<long long>(E, std::max<int64_t>(err_cap, 0)) : 0;
    const long long mcap = missing_out ? std::min<long long>(MT, std::max<int64_t>(missing_cap, 0)) : 0;
    if (ecap > 0 || mcap > 0) {
        int64_t *out = ctx->ws<int64_t>(WS_CR_OUT, 5 * ecap);
        int32_t *seg = ctx->ws<int32_t>(WS_CR_SEG, 2 * E);
        // (missing offsets below mcap fit int32 whenever the list does: checked below before they are used)
        k_cr_emit<<<grid_for(R, 256, 2048), 256, 0, st>>>(rkey, rrow, exp, miss, eidx, moff, R, ecap,
                                                          std::min<long long>(mcap, C_MAX_COUNT), out, seg, seg + E, m);
        if (ecap > 0) HIP_TRY(hipMemcpyAsync(errors_out, out, sizeof(int64_t) * 5 * ecap, hipMemcpyDeviceToHost, st));
        mh = fetch(m, st);
        if (mcap > 0) {
            // the reads that start below mcap are listed whole: at most mcap + one key's values
            if (mcap > C_MAX_COUNT || mh.list_end > (unsigned long long)C_MAX_COUNT)
                throw_jh(JH_ENOMEM, "causal-reverse: a missing list of more than 2^31 - 2 values");
            const long long L = (long long)mh.list_end;
            long long *mbuf = ctx->ws<long long>(WS_CR_MBUF, 2 * L), *mbuf_s = mbuf + L;
            k_cr_key<true, true><<<gkey, KT, 0, st>>>(woff, roff, wk, wv, rp, rrow, rstart, rcnt, dh->aux, K, tier, nullptr,
                                                      nullptr, kv, exp, miss, eflag, moff, mcap, mbuf, m);
            if (global)
                k_cr_key<false, true><<<gkey, KT, 0, st>>>(woff, roff, wk, wv, rp, rrow, rstart, rcnt, dh->aux, K, tier,
                                                           scratch, soff, kv, exp, miss, eflag, moff, mcap, mbuf, m);
            seg_sort_keys(ctx, WS_CR_TMP, mbuf, mbuf_s, (int)L, (int)mh.n_seg, seg, seg + E, st);
            HIP_TRY(hipMemcpyAsync(missing_out, mbuf_s, sizeof(int64_t) * mcap, hipMemcpyDeviceToHost, st));
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    res->device_ms = timer.stop();
}
