// row_select.h -- the preamble jh_bank.hip, jh_longfork.hip and jh_causal.hip open
// with: the wanted rows of a history, compacted IN HISTORY ORDER without an atomic.
//   flag     every wave ballots the wanted rows into 64-bit words, a fixed number
//            of words per tile and kind, and the tile's count goes to tile_cnt
//   scan     an exclusive sum of the tile counts (and the totals to the host)
//   compact  every wave scans its tile's ballot words itself (rs_word_prefix):
//            the prefix of their popcounts is where the wave's rows go
// Kind k's words lie at words + k * n_tiles * WORDS, its counts and bases at
// k * (n_tiles + 1). The pair layout (bank, long-fork) reads rows two at a time
// in 16-byte loads; causal-reverse's one-row-per-lane kernels keep their own
// loops over rs_word_prefix and select_rows.
#pragma once
#include "jh_prims.h"

namespace {
constexpr int RS_PAIRS = 8;                    // row pairs per thread per tile
constexpr int RS_TILE = 256 * RS_PAIRS;        // row pairs per tile (4096 rows: LF_TILE in _abi.py)
constexpr int RS_WORDS = RS_PAIRS * 4 * 2;     // ballot words per tile and kind (64)

// Pair layout, flag: tile = 256 threads x RS_PAIRS row pairs, pair p0 + u * 256 +
// thread; word ((tile * RS_PAIRS + u) * 4 + wave) * 2 + h holds the ballot of
// row 2p + h over the wave's 64 pairs. want(k, type, f): row is of kind k.
template <int KINDS, class Want>
__device__ __forceinline__ void rs_flag_pairs(const int64_t *__restrict__ type, const int64_t *__restrict__ f, int64_t n,
                                              int vec, unsigned long long *__restrict__ words,
                                              long long *__restrict__ tile_cnt, Want want) {
    __shared__ unsigned sh[KINDS][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t np = (n + 1) / 2, n_tiles = (np + RS_TILE - 1) / RS_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t p0 = tile * RS_TILE + threadIdx.x;
        longlong2 t2[RS_PAIRS], f2[RS_PAIRS];
#pragma unroll
        for (int u = 0; u < RS_PAIRS; u++) {
            const int64_t p = p0 + u * 256;
            if (p < np) { t2[u] = ld_pair(type, p, n, vec); f2[u] = ld_pair(f, p, n, vec); }
            else { t2[u] = make_longlong2(-1, -1); f2[u] = t2[u]; }
        }
        unsigned c[KINDS] = {};
#pragma unroll
        for (int u = 0; u < RS_PAIRS; u++) {
            const int64_t p = p0 + u * 256;
#pragma unroll
            for (int k = 0; k < KINDS; k++) {
                const bool r0 = p < np && want(k, t2[u].x, f2[u].x);
                const bool r1 = 2 * p + 1 < n && want(k, t2[u].y, f2[u].y);
                const unsigned long long b0 = __ballot(r0), b1 = __ballot(r1);
                c[k] += __popcll(b0) + __popcll(b1);
                if (lane < 2) words[k * n_tiles * RS_WORDS + ((tile * RS_PAIRS + u) * 4 + wave) * 2 + lane] = lane ? b1 : b0;
            }
        }
        if (lane == 0)
            for (int k = 0; k < KINDS; k++) sh[k][wave] = c[k];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < KINDS; k++)
                tile_cnt[k * (n_tiles + 1) + tile] = (long long)(sh[k][0] + sh[k][1] + sh[k][2] + sh[k][3]);
        __syncthreads();
    }
}

// A wave's scan of one tile's ballot words (WORDS <= 64 of them, lane j takes word
// j): w = my word, excl = the number of flagged rows in the words before it;
// returns the tile's total.
template <int WORDS>
__device__ __forceinline__ unsigned rs_word_prefix(const unsigned long long *__restrict__ tile_words, int lane,
                                                   unsigned long long &w, unsigned &excl) {
    w = lane < WORDS ? tile_words[lane] : 0;
    unsigned inc = __popcll(w);
    const unsigned own = inc;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    excl = inc - own;
    return __shfl(inc, 63);
}

// Pair layout, compact: the exclusive prefix at word 2 * (u * 4 + wave) is where
// the wave's rows of step u go. emit(p, r0, r1, o): rows 2p (r0) and 2p + 1 (r1)
// of pair p are wanted and go to positions o, o + 1 in that order; it does its
// own loads and stores.
template <class Emit>
__device__ __forceinline__ void rs_compact_pairs(int64_t n, const unsigned long long *__restrict__ words,
                                                 const long long *__restrict__ tile_base, Emit emit) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt = (1ULL << lane) - 1;
    const int64_t np = (n + 1) / 2, n_tiles = (np + RS_TILE - 1) / RS_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        unsigned long long w;
        unsigned excl;
        if (rs_word_prefix<RS_WORDS>(words + tile * RS_WORDS, lane, w, excl) == 0) continue;   // no such row in this tile
        const long long base = tile_base[tile];
        const int64_t p0 = tile * RS_TILE + threadIdx.x;
#pragma unroll
        for (int u = 0; u < RS_PAIRS; u++) {
            const int wi = 2 * (u * 4 + wave);
            const unsigned long long b0 = __shfl(w, wi), b1 = __shfl(w, wi + 1);
            const unsigned at = __shfl(excl, wi);
            if ((b0 | b1) == 0) continue;                     // wave-uniform
            const int64_t p = p0 + u * 256;
            const bool r0 = (b0 >> lane) & 1, r1 = (b1 >> lane) & 1;
            if (!(r0 || r1)) continue;                        // nothing below is cross-lane
            emit(p, r0, r1, base + at + __popcll(b0 & lt) + __popcll(b1 & lt));
        }
    }
}

// Host: the flag pass, the scans and the totals of KINDS kinds of row.
struct RowSlots {
    int words, tile_cnt, tile_base, tmp;       // workspace slots
};
template <int KINDS>
struct RowSel {
    int grid;                                   // of the flag kernel: the compact kernels take the same
    const unsigned long long *words[KINDS];
    const long long *base[KINDS];               // per tile: the rows of the kind before it
    long long count[KINDS];
};

// launch_flag(grid, words, tile_cnt) starts the caller's flag kernel
template <int KINDS, class Launch>
RowSel<KINDS> select_rows(jh_ctx *ctx, const RowSlots &slots, int64_t n, int rows_per_tile, int words_per_tile,
                          Launch launch_flag, hipStream_t st) {
    const int64_t n_tiles = (n + rows_per_tile - 1) / rows_per_tile;
    unsigned long long *words = ctx->ws<unsigned long long>(slots.words, KINDS * n_tiles * words_per_tile);
    long long *tile_cnt = ctx->ws<long long>(slots.tile_cnt, KINDS * (n_tiles + 1));
    long long *tile_base = ctx->ws<long long>(slots.tile_base, KINDS * (n_tiles + 1));
    RowSel<KINDS> sel;
    sel.grid = grid_for(n_tiles, 1, 2048);
    for (int k = 0; k < KINDS; k++)              // the scan's last input: its output there is the kind's total
        HIP_TRY(hipMemsetAsync(tile_cnt + k * (n_tiles + 1) + n_tiles, 0, sizeof(long long), st));
    launch_flag(sel.grid, words, tile_cnt);
    for (int k = 0; k < KINDS; k++) {
        const long long *cnt = tile_cnt + k * (n_tiles + 1);
        long long *base = tile_base + k * (n_tiles + 1);
        excl_sum(ctx, slots.tmp, cnt, base, (int)(n_tiles + 1), st);
        sel.words[k] = words + k * n_tiles * words_per_tile;
        sel.base[k] = base;
    }
    for (int k = 0; k < KINDS; k++)
        HIP_TRY(hipMemcpyAsync(&sel.count[k], sel.base[k] + n_tiles, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return sel;
}
}  // namespace
