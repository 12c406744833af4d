// jh_internal.h -- shared internals of libjh.so (HIP, gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>
#include <string>
#include "../../include/jh.h"

#define JH_WAVE 64

// ---------------------------------------------------------------------------
// error plumbing: every entry point returns a JH_* code and fills err.
struct JhError {
    int code = JH_OK;
    std::string msg;
};

#define HIP_TRY(expr)                                                                 \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) {                                                       \
            throw_hip(_e, #expr, __FILE__, __LINE__);                                 \
        }                                                                             \
    } while (0)

struct JhException {
    int code;
    std::string msg;
};

[[noreturn]] inline void throw_hip(hipError_t e, const char *expr, const char *file, int line) {
    char buf[512];
    snprintf(buf, sizeof buf, "HIP error %s (%d) at %s:%d: %s", hipGetErrorString(e), (int)e,
             file, line, expr);
    throw JhException{e == hipErrorOutOfMemory ? JH_ENOMEM : JH_EDEVICE, buf};
}
[[noreturn]] inline void throw_jh(int code, const std::string &msg) { throw JhException{code, msg}; }

// ---------------------------------------------------------------------------
// Device workspace: named, grow-only buffers owned by the context. Entry
// points never allocate in the steady state (same-size calls reuse).
struct Buf {
    void *p = nullptr;
    size_t bytes = 0;
};

struct jh_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t aux = nullptr;     // second stream for racing searches (jh_lin.hip)
    hipStream_t aux2 = nullptr;    // third stream: windows wider than 64 (jh_lin.hip)
    hipStream_t aux3 = nullptr;    // fourth stream: phase-2 late helpers (jh_lin.hip)
    std::mutex mu;
    std::vector<Buf> bufs;
    hipEvent_t ev[24] = {};
    uint32_t gen_base = 0;        // memo generation tags (see jh_lin.hip)
    bool lds_attr = false;        // >64 KB dynamic-LDS attributes set for this device's kernels
    bool lds_attr_wg = false;
    int n_cu = 256;
    int share = 1;                // contexts of one jh_open_devices call on this device (fit_units divides by it)
    size_t hbm_total = 0;         // the device's HBM (hipMemGetInfo, once): bounds the resume buffers
    int32_t *hflag = nullptr;     // host-mapped flag: phase 1's queue drained (jh_lin.hip)
    int32_t *hflag_dev = nullptr;
    void *pinned = nullptr;       // small pinned staging for scalars
    size_t pinned_bytes = 0;
    std::vector<jh_ctx *> members;  // jh_open_multi: one context per device (jh_multi.hip); empty otherwise
    struct Ingest *ingest = nullptr;  // host-buffer staging: packing threads, pinned chunks (jh_ingest.hip)
    size_t mr_cap = 0;              // entries per multi-register memo table whose generation tags are live (jh_linmr.hip)

    template <class T>
    T *ws(int slot, size_t count, bool zero = false) {
        if ((int)bufs.size() <= slot) bufs.resize(slot + 1);
        size_t need = count * sizeof(T);
        if (need == 0) need = 16;
        Buf &b = bufs[slot];
        if (b.bytes < need) {
            if (b.p) HIP_TRY(hipFree(b.p));
            b.p = nullptr;
            size_t alloc = need + need / 8;
            HIP_TRY(hipMalloc(&b.p, alloc));
            b.bytes = alloc;
            if (zero) {
                HIP_TRY(hipMemsetAsync(b.p, 0, alloc, stream));
                HIP_TRY(hipStreamSynchronize(stream));   // callers may run on another stream
            }
        }
        return (T *)b.p;
    }
    bool ws_fresh(int slot) const { return (int)bufs.size() <= slot || bufs[slot].p == nullptr; }
};

// Round 6: contexts open on each device in this process (jh_open / jh_close):
// fit_units and the resume buffers divide a device by max(share, this), so a
// second context opened with its own jh_open does not size its tables as if
// it had the device to itself
int device_open_contexts(int device);

// workspace slot ids (one namespace for the whole library)
enum WsSlot {
    WS_COL_PROCESS = 0, WS_COL_TYPE, WS_COL_F, WS_COL_KEY, WS_COL_VALUE, WS_COL_VALUE2, WS_COL_AUX,
    WS_KEYS_A, WS_KEYS_B, WS_ROWS_A, WS_ROWS_B, WS_SORT_TMP, WS_SEG_OFF, WS_REC, WS_PAIR,
    WS_VIOL, WS_RANK, WS_MISC, WS_VERDICT, WS_QUEUE, WS_DEFER, WS_MEMO, WS_STACK, WS_SCRATCH,
    WS_MEMO_DEEP, WS_STACK_DEEP, WS_SCRATCH_DEEP, WS_SUMMARY, WS_STATS,
    WS_C_PAIR, WS_C_LAST, WS_C_LO, WS_C_HI, WS_C_OUT, WS_C_FLAG, WS_C_TMP, WS_C_IDX,
    WS_S_BITS, WS_S_RUNS, WS_S_TMP, WS_S_CNT,
    WS_BFS_SET, WS_BFS_Q, WS_BFS_META, WS_CLAIM, WS_SCRATCH_BFS, WS_DEBUG, WS_META, WS_ARENA, WS_DEFER_PROG, WS_LIST_W, WS_C_PT,
    WS_DEFER3, WS_MEMO_P3, WS_STACK_P3, WS_SCRATCH_P3,
    WS_LIST_X, WS_MEMO_X, WS_STACK_X, WS_SCRATCH_X, WS_C_OUT2, WS_C_TAB, WS_S_CODE,
    WS_SF_META, WS_SF_FLAG, WS_SF_LUT, WS_SF_TMP, WS_SF_ELEM, WS_SF_STATE, WS_SF_RFLAG, WS_SF_READS,
    WS_SF_BITS, WS_SF_OUT, WS_SF_FL, WS_SF_SEL, WS_SF_TIME, WS_SF_PART,
    WS_Q_META, WS_Q_PART, WS_Q_HIST, WS_Q_FLAG, WS_Q_ROWS, WS_Q_TMP, WS_Q_MULT, WS_Q_MFLAG, WS_Q_POS,
    WS_Q_OUT, WS_Q_KEYS, WS_Q_MULT2, WS_LCOST, WS_LSORT, WS_LTMP, WS_ACC_STATS, WS_WG_GSET, WS_WG_WORK, WS_WG_WTAB, WS_WG_PEND, WS_STATS_KEYS,
    WS_BFS_NODES, WS_BFS_LSTART, WS_BFS_HKEY, WS_BFS_HID, WS_BFS_LIVE, WS_BFS_VIS, WS_BFS_TMP,
    WS_WG_MEMO, WS_WG_STACK, WS_WG_SCR, WS_S_BYTES, WS_IV_U, WS_IV_IDX, WS_IV_KEY, WS_IV_RINIT, WS_IV_MAX, WS_IV_TMP,
    WS_HELP_START, WS_HELP_TAKEN, WS_DEFER_TIME, WS_BFS_TMPK,
    WS_DEFER64, WS_DEFER64_T, WS_MEMO_WIDE, WS_STACK_WIDE, WS_SCRATCH_WIDE,
    WS_CFG_SLOT, WS_CFG_OUT, WS_CFG_N, WS_CFG_ROWS, WS_CFG_KEYS,
    WS_S_RB_HIST, WS_S_RB_OUT, WS_TL, WS_RS_ARENA, WS_RS_OFF, WS_RS_LOG, WS_DEFER_INFO,
    WS_SPEC, WS_SPEC_RES, WS_DEBUG_WG, WS_HANDOFF, WS_RS_LOG2,
    WS_U_META, WS_U_PART, WS_U_LIST, WS_U_ALT, WS_U_ALT2, WS_U_BITS, WS_U_TMP, WS_U_FLAG, WS_U_RUNS, WS_U_PAIRS,
    WS_U_CNT, WS_U_IDX, WS_U_SEL, WS_U_OUT,
    WS_B_META, WS_B_WORDS, WS_B_TCNT, WS_B_TBASE, WS_B_TMP, WS_B_ROW, WS_B_START, WS_B_CNT, WS_B_OFF, WS_B_TOT,
    WS_B_BAD, WS_B_CLS, WS_B_FIRST, WS_B_PARTS, WS_B_ACC, WS_B_OUT, WS_B_TRI,
    WS_LF_META, WS_LF_WORDS, WS_LF_TCNT, WS_LF_TBASE, WS_LF_TMP, WS_LF_ROW, WS_LF_START, WS_LF_CNT, WS_LF_GRP, WS_LF_MASK,
    WS_LF_WKEY, WS_LF_WROW, WS_LF_FIRST, WS_LF_KEYS, WS_LF_IDX, WS_LF_RANK, WS_LF_SLOT, WS_LF_CTAB, WS_LF_VTAB, WS_LF_GBITS,
    WS_LF_FLAG, WS_LF_SKEY, WS_LF_SMASK, WS_LF_SROW, WS_LF_PC, WS_LF_OUT,
    WS_CR_META, WS_CR_WORDS, WS_CR_TCNT, WS_CR_TBASE, WS_CR_TMP, WS_CR_WKEY, WS_CR_WVAL, WS_CR_RKEY, WS_CR_RPERM, WS_CR_RROW,
    WS_CR_OFF, WS_CR_TIER, WS_CR_KV, WS_CR_EXP, WS_CR_MISS, WS_CR_SOFF, WS_CR_SCRATCH, WS_CR_OUT, WS_CR_SEG, WS_CR_MBUF,
    WS_CY_META, WS_CY_TMP, WS_CY_PKEY, WS_CY_PROW, WS_CY_COMP, WS_CY_REV, WS_CY_IP, WS_CY_ICOMP, WS_CY_CNT,
    WS_CY_TXN, WS_CY_REC, WS_CY_HASH, WS_CY_HIDX, WS_CY_RAW, WS_CY_EDGES, WS_CY_REACH, WS_CY_BS, WS_CY_REG, WS_CY_SEL,
    WS_CY_FWD, WS_CY_BWD, WS_CY_CSR, WS_CY_STATE, WS_CY_LABEL, WS_CY_SIZE, WS_CY_KEYS, WS_CY_VALS,
    WS_CY_AP_META, WS_CY_AP_ROWS, WS_CY_AP_RECS, WS_CY_AP_LONGEST,
    WS_CY_MO_META, WS_CY_MO_ROWS, WS_CY_MO_RECS,
    WS_BFS_TAKEN,
    WS_CM_META, WS_CM_WORDS, WS_CM_TCNT, WS_CM_TBASE, WS_CM_TMP, WS_CM_KEY, WS_CM_ROW, WS_CM_OFF, WS_CM_SUM, WS_CM_EV, WS_CM_OUT,
    WS_G2_META, WS_G2_CNT, WS_G2_WORDS, WS_G2_TCNT, WS_G2_TBASE, WS_G2_TMP, WS_G2_MIN, WS_G2_OUT,
    WS_PF_META, WS_PF_TIME, WS_PF_TMP, WS_PF_K64A, WS_PF_K64B, WS_PF_K64C, WS_PF_K64D, WS_PF_V32A, WS_PF_V32B,
    WS_PF_K32A, WS_PF_K32B, WS_PF_PAIR, WS_PF_RUN_U, WS_PF_RUN_C, WS_PF_RUN_S, WS_PF_NRUNS, WS_PF_OUT,
    WS_SI_KEYS, WS_SI_META, WS_SI_WORDS, WS_SI_TMP, WS_SI_BITS, WS_SI_OUT, WS_SI_RECS,
    WS_MR_META, WS_MR_TMP, WS_MR_NF, WS_MR_FLAG, WS_MR_ROLE, WS_MR_LINK, WS_MR_SRC, WS_MR_SKEY, WS_MR_SKEY2, WS_MR_ROWID,
    WS_MR_ROWS, WS_MR_OFF, WS_MR_INC, WS_MR_PK, WS_MR_PK2, WS_MR_RA, WS_MR_RB, WS_MR_KB, WS_MR_KB2, WS_MR_VIOL,
    WS_MR_KEYS, WS_MR_CNT, WS_MR_SCAN, WS_MR_OPIDX, WS_MR_OPS, WS_MR_OPRR, WS_MR_LAYERS, WS_MR_WND, WS_MR_COST,
    WS_MR_COST2, WS_MR_ORDER, WS_MR_ORDER2, WS_MR_MEMO, WS_MR_STACK, WS_MR_GEN, WS_MR_OUT, WS_MR_TABS,
    WS_COUNT
};

// row-level helpers shared by kernels
__device__ __forceinline__ uint64_t jh_mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33; return x;
}

// Block-wide reduction for 256-thread blocks (4 waves): one value per block,
// so a reduction kernel issues one global atomic per block, not per wave
// (per-wave atomics on a few addresses serialise in L2).
template <class T, class Op>
__device__ __forceinline__ T block_reduce256(T v, Op op, T *sh /* [4] shared */) {
    for (int o = 32; o > 0; o >>= 1) v = op(v, (T)__shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return op(op(sh[0], sh[1]), op(sh[2], sh[3]));
}
struct RedMin { template <class T> __device__ T operator()(T a, T b) const { return a < b ? a : b; } };
struct RedMax { template <class T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct RedSum { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };
struct RedOr { template <class T> __device__ T operator()(T a, T b) const { return a | b; } };

inline int grid_for(int64_t n, int block, int cap = 65536) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

// Copies a host jh_history to device workspace columns (or passes device
// pointers through). Returns a device-pointer view.
jh_history stage_history(jh_ctx *ctx, const jh_history *h, bool need_key, bool need_aux);
// jh_ingest.hip: packed, pipelined staging of large host histories (false: too small)
bool ingest_columns(jh_ctx *ctx, const int64_t *const src[7], int64_t *const dst[7], int64_t n, hipStream_t st);
void ingest_free(struct Ingest *g);

// linearizability (jh_lin.hip). cfg: a jh_lin_configs request (the frontier
// configurations of the listed keys, device buffers; null for a check)
struct LinCfgReq {
    const int64_t *keys_dev;      // n_q requested keys
    int32_t n_q, per_key;
    const int32_t *slot_dev;      // per key: its index in keys_dev, or -1
    jh_lin_config *out_dev;       // n_q * per_key
    int32_t *n_dev;               // n_q, -1 on entry
    int64_t *rows_dev;            // n_q * per_key * 64
};
// Bytes of the caller's jh_lin_opts / jh_summary the library may touch: the
// whole struct with JH_LIN_TAIL_FIELDS, else ABI 8's layout (jh.h)
inline size_t lin_opts_bytes(const jh_lin_opts *o) {
    return o && (o->flags & JH_LIN_TAIL_FIELDS) ? sizeof(jh_lin_opts) : offsetof(jh_lin_opts, bfs_stall_min);
}
inline size_t lin_summary_bytes(const jh_lin_opts *o) {
    return o && (o->flags & JH_LIN_TAIL_FIELDS) ? sizeof(jh_summary) : offsetof(jh_summary, bfs_stall_picks);
}
void lin_check_independent(jh_ctx *ctx, const jh_history *dh, const jh_lin_opts *opts,
                           bool keyed, jh_key_verdict *out_dev, jh_summary *sum,
                           hipStream_t stream, const LinCfgReq *cfg = nullptr);
// per-key row CSR of an independent history (jh_lin.hip)
void key_index(jh_ctx *ctx, const jh_history *dh, int64_t *key_off, int64_t *rows, hipStream_t stream);
// counter (jh_counter.hip)
void counter_check(jh_ctx *ctx, const jh_history *dh, int64_t *reads_out, int64_t reads_cap,
                   int64_t *n_reads, int64_t *n_errors, int64_t *first_err, int32_t *valid,
                   int32_t *cause, hipStream_t stream);
// set (jh_set.hip)
void set_check(jh_ctx *ctx, const jh_history *dh, jh_set_result *res, int64_t *runs[4],
               int64_t runs_cap, hipStream_t stream);
void set_check_bitmaps(jh_ctx *ctx, const jh_history *dh, jh_set_result *res, uint32_t *bits_out[4],
                       int64_t words_cap, int64_t *base, int64_t *n_words, hipStream_t stream);
// independent set (jh_setindep.hip); keys_out = max(n_keys, 1) host records (or null), bits_out = {ok, lost, unexpected, recovered}
void set_independent_check(jh_ctx *ctx, const jh_history *dh, const jh_set_indep_opts *opts, jh_set_indep_result *res,
                           jh_set_key *keys_out, uint32_t *bits_out[4], int64_t words_cap, hipStream_t stream);
// set-full (jh_setfull.hip); lists_out = {lost, never-read, stale}
void set_full_check(jh_ctx *ctx, const jh_history *dh, const int64_t *time_dev, bool linearizable, int64_t read_batch,
                    jh_set_full_result *res, int64_t *lists_out[3], int64_t list_cap, hipStream_t stream);
// queues (jh_queue.hip); outs = {lost, unexpected, duplicated, recovered}
void total_queue_check(jh_ctx *ctx, const jh_history *dh, jh_queue_result *res, int64_t *outs[4],
                       int64_t cap, hipStream_t stream);
void queue_check(jh_ctx *ctx, const jh_history *dh, jh_queue_result *res, int64_t *final_out, int64_t cap,
                 hipStream_t stream);
// unique-ids (jh_uids.hip); dup_out = (id, count) pairs
void unique_ids_check(jh_ctx *ctx, const jh_history *dh, const jh_unique_ids_opts *opts, jh_unique_ids_result *res,
                      int64_t *dup_out, int64_t dup_cap, hipStream_t stream);
// bank (jh_bank.hip); reads_out = [row, total, class] triples
void bank_check(jh_ctx *ctx, const jh_history *dh, const jh_bank_opts *opts, jh_bank_result *res,
                int64_t *reads_out, int64_t reads_cap, int64_t *n_reads, hipStream_t stream);
// long-fork (jh_longfork.hip); forks_out = [row_a, row_b] pairs
void long_fork_check(jh_ctx *ctx, const jh_history *dh, const jh_long_fork_opts *opts, jh_long_fork_result *res,
                     int64_t *forks_out, int64_t fork_cap, hipStream_t stream);
// causal-reverse (jh_causal.hip); errors_out = [row, key, expected_count, missing_count, missing_offset]
void causal_reverse_check(jh_ctx *ctx, const jh_history *dh, const jh_causal_reverse_opts *opts,
                          jh_causal_reverse_result *res, int32_t *key_valid, int64_t *errors_out, int64_t err_cap,
                          int64_t *missing_out, int64_t missing_cap, hipStream_t stream);
// causal (jh_causalreg.hip); keys_out = max(n_keys, 1) host records
void causal_check(jh_ctx *ctx, const jh_history *dh, jh_causal_result *res, jh_causal_key *keys_out, hipStream_t stream);
// adya g2 (jh_g2.hip); illegal_out = [key id, count] pairs
void g2_check(jh_ctx *ctx, const jh_history *dh, jh_g2_result *res, int64_t *illegal_out, int64_t illegal_cap,
              hipStream_t stream);
// multi-register linearizability (jh_linmr.hip); out = max(n_keys, 1) host verdicts, sum may be null
void multi_register_check(jh_ctx *ctx, const jh_history *dh, const jh_multi_register_opts *opts, jh_key_verdict *out,
                          jh_summary *sum, hipStream_t stream);
// perf (jh_perf.hip); dh's process / type / f and time_dev are device columns, the outputs host buffers (any may be null)
struct PerfOut {
    int64_t *pair, pair_cap, *pt_row, pt_cap, *series, series_cap, *groups, group_cap, *cells, cell_cap;
};
void perf_reduce(jh_ctx *ctx, const jh_history *dh, const int64_t *time_dev, const jh_perf_opts *opts,
                 jh_perf_result *res, const PerfOut &out, hipStream_t stream);
// cycle (jh_cycle.hip); src / dst are host edge lists, the outputs host buffers (any may be null)
struct CycleOut {
    int64_t *labels, *scc_off, *scc_rows, scc_cap, rows_cap, *edges, edge_cap;
};
void scc_check(jh_ctx *ctx, int64_t n, const int64_t *src, const int64_t *dst, int64_t n_edges,
               const jh_cycle_opts *opts, jh_cycle_result *res, const CycleOut &out, hipStream_t stream);
void cycle_check(jh_ctx *ctx, const jh_history *dh, const jh_cycle_opts *opts, jh_cycle_result *res,
                 const CycleOut &out, hipStream_t stream);
// appends-and-reads-graph (jh_cycle_append.hip). append_plan runs the verification passes and sizes the
// edge slots (cause != 0: res holds the cause's fields and nothing more is to be done); append_fill writes
// plan.slots packed words, holes included, and returns the number of link calls
struct AppendPlan {
    int cause = 0;
    long long reads = 0, appends = 0, rw = 0, slots = 0;
    alignas(8) unsigned char state[640] = {};   // the builder's device arrays between the two calls
};
AppendPlan append_plan(jh_ctx *ctx, const jh_history *dh, jh_cycle_result *res, hipStream_t stream);
long long append_fill(jh_ctx *ctx, const AppendPlan &plan, unsigned long long *raw, hipStream_t stream);
// monotonic-key-graph (jh_cycle_mono.hip). mono_plan validates, sorts the (k, v, row) records and places the
// edges (slots = their number, every one a real edge, decided from 64-bit counts; res->entries = the pairs
// scanned); mono_fill writes plan.slots packed words
struct MonoPlan {
    long long records = 0, slots = 0;
    const long long *eoff = nullptr;          // the builder's device arrays between the two calls
    const int32_t *dstart = nullptr, *srow = nullptr;
};
MonoPlan mono_plan(jh_ctx *ctx, const jh_history *dh, jh_cycle_result *res, hipStream_t stream);
void mono_fill(jh_ctx *ctx, const MonoPlan &plan, unsigned long long *raw, hipStream_t stream);
