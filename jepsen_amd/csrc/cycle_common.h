// cycle_common.h -- what jh_cycle.hip, jh_cycle_append.hip and jh_cycle_mono.hip share: the packed
// edge word, the grid-stride loop, the (k, v) hash with its sorted-hash lookup,
// and the arena that lays a run of device arrays out behind one workspace slot.
// The hipcub calls (over the WS_CY_TMP scratch), fetch and the op-type constants
// come from jh_prims.h. Everything is internal to the including file (anonymous
// namespace).
#pragma once
#include "jh_prims.h"

namespace {
typedef unsigned long long u64;
constexpr u64 HOLE = ~0ULL, NONE = ~0ULL;
constexpr long long Y_MAX = 0x7ffffffeLL;

__device__ __forceinline__ u64 pack(int64_t s, int64_t d) { return ((u64)s << 32) | (u64)(uint32_t)d; }
#define CY_LOOP(i, cnt) for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < (cnt); i += (int64_t)gridDim.x * blockDim.x)

__device__ __forceinline__ u64 cy_hash(int64_t k, int64_t v) {
    return jh_mix64((u64)k * 0x9e3779b97f4a7c15ULL + jh_mix64((u64)v));
}

// the first position of the sorted words that is not below `key`
__device__ __forceinline__ long long cy_lower(const u64 *__restrict__ sorted, long long cnt, u64 key) {
    long long lo = 0, hi = cnt;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (sorted[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the last i in [0, cnt) with off[i] <= e (off ascending, off[0] <= e)
__device__ __forceinline__ long long cy_owner(const long long *__restrict__ off, long long cnt, long long e) {
    long long lo = 0, hi = cnt - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (off[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// a run of device arrays behind one workspace slot: laid out twice, to size and to place
struct Arena {
    char *p;
    size_t off = 0;
    template <class T>
    void take(T *&out, long long cnt) {
        off = (off + 15) & ~(size_t)15;
        out = p ? (T *)(p + off) : nullptr;
        off += sizeof(T) * (size_t)std::max<long long>(cnt, 1);
    }
};

template <class F>
void carve(jh_ctx *ctx, int slot, F layout) {
    Arena size{nullptr};
    layout(size);
    Arena place{ctx->ws<char>(slot, size.off)};
    layout(place);
}
}  // namespace
