// jh_set_bits.h -- the bitmap helpers jh_set.hip and jh_setindep.hip share:
// the LDS-merged atomicOr marking of a row chunk and the word-wise set algebra
// of (checker/set). Internal to the including file (anonymous namespace).
#pragma once
#include "jh_prims.h"

namespace {

// Marking: each workgroup takes a contiguous chunk of MARK_CH rows (or read
// elements) and merges its bits in LDS before touching HBM.
//  * Within a wave, lanes holding the same bitmap word are merged by a
//    segmented OR scan over lanes (shuffles); only the last lane of each run
//    writes. Jepsen's set elements are mostly written and read in ascending
//    order, so a wave's 64 elements fall into two or three words.
//  * Those few writes go to a direct-mapped LDS cache of words (tag + bits);
//    a word whose slot holds another word goes straight to HBM.
//  * At the end the cache is flushed: one global atomicOr per cached word.
// Any element order stays correct (unmerged lanes just write on their own).
constexpr int MARK_CH = 16384, MARK_SLOTS = 2048;
constexpr long long MARK_EMPTY = -1;

__device__ __forceinline__ void mark_bits(uint32_t *bm, long long *tag, uint32_t *lb, long long w, uint32_t bits) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long wn = __shfl_up(w, o);
        const uint32_t bn = (uint32_t)__shfl_up((int)bits, o);
        if (lane >= o && wn == w) bits |= bn;
    }
    const long long wnext = __shfl_down(w, 1);
    const bool tail = lane == 63 || wnext != w;
    if (w < 0 || !tail) return;
    const int sl = (int)(w & (MARK_SLOTS - 1));
    long long t = tag[sl];
    if (t == MARK_EMPTY)
        t = (long long)atomicCAS((unsigned long long *)&tag[sl], (unsigned long long)MARK_EMPTY, (unsigned long long)w);
    if (t == MARK_EMPTY || t == w) atomicOr(&lb[sl], bits);
    else atomicOr(&bm[w], bits);
}

__device__ __forceinline__ void mark_init(long long *tag, uint32_t *lb) {
    for (int i = threadIdx.x; i < MARK_SLOTS; i += blockDim.x) { tag[i] = MARK_EMPTY; lb[i] = 0; }
    __syncthreads();
}
__device__ __forceinline__ void mark_flush(uint32_t *bm, const long long *tag, const uint32_t *lb) {
    __syncthreads();
    for (int i = threadIdx.x; i < MARK_SLOTS; i += blockDim.x)
        if (tag[i] != MARK_EMPTY && lb[i]) atomicOr(&bm[tag[i]], lb[i]);
}

// the four result sets of one word: ok, lost, unexpected, recovered
// (checker.clj:210-223) from attempts a, acknowledged d and the final read r
__device__ __forceinline__ void set_algebra(uint32_t a, uint32_t d, uint32_t r, uint32_t out[4]) {
    const uint32_t ok = r & a;
    out[0] = ok;          // ok
    out[1] = d & ~r;      // lost
    out[2] = r & ~a;      // unexpected
    out[3] = ok & ~d;     // recovered
}
__device__ __forceinline__ void set_words(const uint32_t *A, const uint32_t *D, const uint32_t *R,
                                          int64_t w, int64_t nw, uint32_t out[4]) {
    set_algebra(A[w], D[w], R[w], out);
}
}  // namespace
