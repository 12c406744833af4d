// jh_prims.h -- the host and device odds and ends the workload checkers share:
// the op-type constants, the 16-byte row-pair load, the one-value device read,
// the event timer and the hipcub calls over a caller-named scratch slot. Everything is internal to the including file
// (anonymous namespace). jh_lin.hip does not use it: its hipcub sites size jointly.
#pragma once
#include "jh_internal.h"
#include <hipcub/hipcub.hpp>
#include <algorithm>

namespace {
constexpr int T_INVOKE = JH_TYPE_INVOKE, T_OK = JH_TYPE_OK, T_FAIL = JH_TYPE_FAIL, T_INFO = JH_TYPE_INFO;

// Row pairs: both rows in one 16-byte load when the columns are 16-byte
// aligned (vec; workspace and torch allocations are), two 8-byte loads
// otherwise; a trailing odd row is the last pair's first half
__device__ __forceinline__ longlong2 ld_pair(const int64_t *__restrict__ c, int64_t i, int64_t n, bool vec) {
    if (2 * i + 1 < n) return vec ? ((const longlong2 *)c)[i] : make_longlong2(c[2 * i], c[2 * i + 1]);
    return make_longlong2(c[2 * i], 0);
}

// one value from the device, after everything queued on st
template <class T>
T fetch(const T *dev, hipStream_t st) {
    T h;
    HIP_TRY(hipMemcpyAsync(&h, dev, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return h;
}

// device time of a check, over the context's first two events
struct DeviceTimer {
    jh_ctx *ctx;
    hipStream_t st;
    void start() { HIP_TRY(hipEventRecord(ctx->ev[0], st)); }
    float stop() {
        HIP_TRY(hipEventRecord(ctx->ev[1], st));
        HIP_TRY(hipEventSynchronize(ctx->ev[1]));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        return ms;
    }
};

// ---------------------------------------------------------------------------
// hipcub's two-call pattern. call(scratch, bytes) is the hipcub call with its
// first two arguments left open: once with a null scratch to size it, then
// over the grow-only workspace slot the caller names. Iterator and count types
// pass through unchanged (they select hipcub's kernels).
template <class F>
size_t cub_size(F call) {
    size_t tb = 0;
    HIP_TRY(call(nullptr, tb));
    return tb;
}
template <class F>
void cub_run(jh_ctx *ctx, int slot, F call) {
    size_t tb = cub_size(call);
    HIP_TRY(call(ctx->ws<char>(slot, tb), tb));
}
// hipcub names its kernels after the iterator types: a buffer read as `const T *`
// and as `T *` gives two kernels. as_input(p) is the read-only spelling.
template <class T>
const T *as_input(const T *p) { return p; }
#define JH_CUB(fn, ...) [&](void *d_tmp, size_t &tb) { return hipcub::fn(d_tmp, tb, __VA_ARGS__); }

template <class In, class Out, class N>
void excl_sum(jh_ctx *ctx, int slot, In in, Out out, N cnt, hipStream_t st) {
    cub_run(ctx, slot, JH_CUB(DeviceScan::ExclusiveSum, in, out, cnt, st));
}
template <class In, class Out, class N>
void incl_sum(jh_ctx *ctx, int slot, In in, Out out, N cnt, hipStream_t st) {
    cub_run(ctx, slot, JH_CUB(DeviceScan::InclusiveSum, in, out, cnt, st));
}
template <class In, class Out, class Op, class Init, class N>
void excl_scan(jh_ctx *ctx, int slot, In in, Out out, Op op, Init init, N cnt, hipStream_t st) {
    cub_run(ctx, slot, JH_CUB(DeviceScan::ExclusiveScan, in, out, op, init, cnt, st));
}
template <class In, class Out, class Op, class N>
void incl_scan(jh_ctx *ctx, int slot, In in, Out out, Op op, N cnt, hipStream_t st) {
    cub_run(ctx, slot, JH_CUB(DeviceScan::InclusiveScan, in, out, op, cnt, st));
}
// radix sorts on bits [0, end_bit); the pair sorts are stable
template <class K, class N>
void sort_keys(jh_ctx *ctx, int slot, const K *in, K *out, N cnt, int end_bit, hipStream_t st) {
    cub_run(ctx, slot, JH_CUB(DeviceRadixSort::SortKeys, in, out, cnt, 0, end_bit, st));
}
template <class K, class N>
void sort_keys(jh_ctx *ctx, int slot, hipcub::DoubleBuffer<K> &k, N cnt, int end_bit, hipStream_t st) {
    cub_run(ctx, slot, JH_CUB(DeviceRadixSort::SortKeys, k, cnt, 0, end_bit, st));
}
template <class K, class V, class N>
void sort_pairs(jh_ctx *ctx, int slot, const K *kin, K *kout, const V *vin, V *vout, N cnt, int end_bit, hipStream_t st) {
    cub_run(ctx, slot, JH_CUB(DeviceRadixSort::SortPairs, kin, kout, vin, vout, cnt, 0, end_bit, st));
}
template <class K, class V, class N>
void sort_pairs(jh_ctx *ctx, int slot, hipcub::DoubleBuffer<K> &k, hipcub::DoubleBuffer<V> &v, N cnt, int end_bit,
                hipStream_t st) {
    cub_run(ctx, slot, JH_CUB(DeviceRadixSort::SortPairs, k, v, cnt, 0, end_bit, st));
}
template <class K, class N, class Off>
void seg_sort_keys(jh_ctx *ctx, int slot, const K *in, K *out, N cnt, int n_seg, Off seg_begin, Off seg_end,
                   hipStream_t st) {
    cub_run(ctx, slot,
            JH_CUB(DeviceSegmentedRadixSort::SortKeys, in, out, cnt, n_seg, seg_begin, seg_end, 0, (int)sizeof(K) * 8, st));
}
template <class In, class Flag, class Out, class Num, class N>
void select_flagged(jh_ctx *ctx, int slot, In in, Flag flag, Out out, Num n_sel, N cnt, hipStream_t st) {
    cub_run(ctx, slot, JH_CUB(DeviceSelect::Flagged, in, flag, out, n_sel, cnt, st));
}
template <class In, class Out, class Num, class N, class Pred>
void select_if(jh_ctx *ctx, int slot, In in, Out out, Num n_sel, N cnt, Pred pred, hipStream_t st) {
    cub_run(ctx, slot, JH_CUB(DeviceSelect::If, in, out, n_sel, cnt, pred, st));
}
}  // namespace
