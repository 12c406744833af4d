// cycle_common.h -- what jh_cycle.hip, jh_cycle_append.hip and jh_cycle_mono.hip share: the packed
// edge word, the grid-stride loop, the (k, v) hash with its sorted-hash lookup,
// the hipcub wrappers over the WS_CY_TMP scratch, and the arena that lays a run
// of device arrays out behind one workspace slot. Everything is internal to
// the including file (anonymous namespace).
#pragma once
#include "jh_internal.h"
#include <hipcub/hipcub.hpp>
#include <algorithm>

namespace {
typedef unsigned long long u64;
constexpr int T_INVOKE = JH_TYPE_INVOKE, T_OK = JH_TYPE_OK, T_FAIL = JH_TYPE_FAIL, T_INFO = JH_TYPE_INFO;
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

char *tmp(jh_ctx *ctx, size_t bytes) { return ctx->ws<char>(WS_CY_TMP, bytes); }

template <class T>
T fetch(const T *dev, hipStream_t st) {
    T h;
    HIP_TRY(hipMemcpyAsync(&h, dev, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return h;
}

template <class T>
void excl_sum(jh_ctx *ctx, const T *in, T *out, int64_t cnt, hipStream_t st) {
    size_t tb = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, in, out, (int)cnt, st));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp(ctx, tb), tb, in, out, (int)cnt, st));
}

void sort_keys(jh_ctx *ctx, const u64 *in, u64 *out, long long cnt, int end_bit, hipStream_t st) {
    size_t tb = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb, in, out, (int)cnt, 0, end_bit, st));
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(tmp(ctx, tb), tb, in, out, (int)cnt, 0, end_bit, st));
}

// stable: equal keys keep the order of their values' positions
void sort_pairs(jh_ctx *ctx, const u64 *kin, u64 *kout, const uint32_t *vin, uint32_t *vout, long long cnt, hipStream_t st) {
    size_t tb = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, kin, kout, vin, vout, (int)cnt, 0, 64, st));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp(ctx, tb), tb, kin, kout, vin, vout, (int)cnt, 0, 64, st));
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
