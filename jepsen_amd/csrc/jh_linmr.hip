// jh_linmr.hip -- (independent/checker (checker/linearizable {:model
// (multi-register init)})) on MI355X: the multi-register model of
// yugabyte/src/yugabyte/multi_key_acid.clj:20-42 searched by WGL, every key of
// an independent history in one call (include/jh.h, jh_check_multi_register).
//
// A txn reduces, whatever the state, to (never, rmask, rval, wmask, wval) over a
// bit-packed state word: step(s) = (never or (s & rmask) != rval) ? inconsistent
// : (s & ~wmask) | wval. A model step is four ALU ops; there is no table.
//
//   k_mr_rows     flat, one thread per row: the row's sort key (its key, or K
//                 for a row no key owns), its txn compiled to the normal form,
//                 the refusals
//   (sort, k_mr_off)   the stable key partition: rows by key in history order
//   k_mr_pk, k_mr_kb, (two sorts), k_mr_pair
//                 the client rows that are not :info sorted by process, then
//                 stably by key: neighbours in a (key, process) run are an
//                 invocation and its completion; causes 3 and 4; each
//                 invocation classified ok / crashed with writes / dropped
//   k_mr_count    one wave per key over its rows in history order: ops, :ok
//                 returns, the windows' sizes; the early verdicts
//   (scans, sort) table offsets; the searched keys, widest window sum first
//   k_mr_fill     one wave per key: ops in call order, layers (the :ok returns
//                 in history order) and each layer's window
//   k_mr_search   persistent waves, one key per wave from an atomic queue: the
//                 WGL DFS of DESIGN section 3 over (t, mask, state), memo in
//                 HBM under generation tags
//
// The window of layer t is W(t) of DESIGN section 3 -- the kept ops called before
// the t-th :ok return and open there -- WITHOUT the returning op itself: that op
// is never linearized inside its own layer, so it needs no mask bit, and it is
// held apart (lane j = member j of the others, at most JH_MR_MAX_WINDOW = 64 of
// them). Candidates keep W(t)'s call order: the returning op stands at retpos.
#include "jh_prims.h"

namespace {

constexpr int MR_TBITS = 20;                         // layer bits of a memo tag; the rest is the generation
constexpr uint32_t MR_GEN_MAX = (1u << (32 - MR_TBITS)) - 1;
constexpr int64_t MR_OK_LIMIT = (1LL << MR_TBITS) - 1;   // searched :ok ops of one key
constexpr unsigned long long MR_NO_VIOL = ~0ULL;

enum : int { MR_BAD_KEY = 1, MR_UNSUP_KEY = 2, MR_BAD_RANGE = 4, MR_UNSUP_MOPS = 8, MR_BAD_F = 16, MR_BAD_REG = 32,
             MR_BAD_VAL = 64 };
enum : uint8_t { NF_NEVER = 1, NF_NIL = 2, NF_WRITES = 4 };     // a row's flags: never, a nil :value, a write micro-op
enum : uint8_t { ROLE_NONE = 0, ROLE_CALL = 1, ROLE_RET = 2 };  // a row in the search: a kept op's call, a kept :ok op's return

struct MrMeta {
    int flags;
    uint32_t n_inc;                  // client rows that are not :info (the pairing's rows)
    unsigned long long max_proc;
    uint32_t n_search;               // keys that need a search
    uint32_t head;                   // the search queue's head
    uint32_t max_ops;                // most ops of one searched key (the stack's depth)
};

struct MrKey {
    uint32_t n_ops, n_ok, max_w, searched;
    unsigned long long sum_w;
};

struct MrLayer {                     // the t-th :ok return of a key
    uint32_t wrel;                   // its window's first entry, relative to the key's
    uint32_t ret_row;
    uint32_t w_pos;                  // members of the window | the returning op's position in W(t) << 8
    uint32_t ret_op;                 // the returning op
};

struct MrTab {                       // a searched key's tables
    unsigned long long ooff, loff, woff;
};

__device__ __forceinline__ uint32_t field_mask(int reg, int bits) {
    return (uint32_t)(((1ULL << bits) - 1) << (reg * bits));
}

// One thread per row.
__global__ void __launch_bounds__(256) k_mr_rows(const int64_t *__restrict__ process, const int64_t *__restrict__ type,
                                                 const int64_t *__restrict__ key, const int64_t *__restrict__ val,
                                                 const int64_t *__restrict__ val2, const int64_t *__restrict__ aux,
                                                 int64_t n_aux, int64_t n, int64_t K, int keyed, int n_regs, int bits,
                                                 uint32_t *__restrict__ skey, uint32_t *__restrict__ rowid,
                                                 uint8_t *__restrict__ inc, uint4 *__restrict__ nf,
                                                 uint8_t *__restrict__ nflag, uint8_t *__restrict__ role, MrMeta *m) {
    const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (r >= n) return;
    int flags = 0;
    const int64_t p = process[r], ty = type[r];
    const bool client = p >= 0;
    int64_t k = keyed ? key[r] : 0;
    if (k >= K) { flags |= MR_BAD_KEY; k = -1; }
    if (client && k < 0) flags |= MR_UNSUP_KEY;
    const bool mine = client && k >= 0;
    skey[r] = mine ? (uint32_t)k : (uint32_t)K;
    rowid[r] = (uint32_t)r;
    role[r] = ROLE_NONE;
    inc[r] = mine && (ty == T_INVOKE || ty == T_OK || ty == T_FAIL);
    uint32_t rmask = 0, rval = 0, wmask = 0, wval = 0, wset = 0;
    uint8_t fl = 0;
    if (mine) {
        const int64_t off = val[r], cnt = val2[r];
        if (off == JH_NIL) fl |= NF_NIL;
        else if (cnt < 0 || off < 0 || off > n_aux / 3 || cnt > n_aux / 3 - off || (cnt > 0 && !aux)) flags |= MR_BAD_RANGE;
        else if (cnt > JH_CY_MAX_MOPS) flags |= MR_UNSUP_MOPS;
        else {
            for (int64_t j = 0; j < cnt; j++) {
                const int64_t f = aux[3 * (off + j)], reg = aux[3 * (off + j) + 1];
                int64_t v = aux[3 * (off + j) + 2];
                if (v == JH_NIL) v = 0;
                if (f != JH_F_READ && f != JH_F_WRITE) { if (ty != T_FAIL) flags |= MR_BAD_F; continue; }
                if (reg < 0 || reg >= n_regs) { flags |= MR_BAD_REG; continue; }
                if (v < 0 || v >= (1LL << bits)) { flags |= MR_BAD_VAL; continue; }
                const uint32_t fm = field_mask((int)reg, bits), vv = (uint32_t)((uint64_t)v << (reg * bits));
                if (f == JH_F_READ) {
                    if (v == 0) continue;                                   // a nil read is always legal
                    if ((wset >> reg) & 1) { if ((wval & fm) != vv) fl |= NF_NEVER; }
                    else if (rmask & fm) { if ((rval & fm) != vv) fl |= NF_NEVER; }
                    else { rmask |= fm; rval |= vv; }
                } else {
                    fl |= NF_WRITES;
                    wset |= 1u << reg; wmask |= fm; wval = (wval & ~fm) | vv;
                }
            }
        }
        if ((unsigned long long)p > *(volatile unsigned long long *)&m->max_proc) atomicMax(&m->max_proc, (unsigned long long)p);
    }
    nf[r] = make_uint4(rmask, rval, wmask, wval);
    nflag[r] = fl;
    if (flags) atomicOr(&m->flags, flags);
}

// off[k] = the first position of the sorted keys that is >= k, k in [0, K]
__global__ void k_mr_off(const uint32_t *__restrict__ sk, int64_t n, int64_t K, uint32_t *__restrict__ off) {
    const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (k > K) return;
    int64_t a = 0, b = n;
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (sk[mid] < (uint32_t)k) a = mid + 1; else b = mid;
    }
    off[k] = (uint32_t)a;
}

__global__ void k_mr_pk(const uint32_t *__restrict__ rows, int64_t n, const int64_t *__restrict__ process,
                        unsigned long long *__restrict__ pk) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) pk[i] = (unsigned long long)process[rows[i]];
}

__global__ void k_mr_kb(const uint32_t *__restrict__ rows, int64_t n, const uint32_t *__restrict__ skey,
                        uint32_t *__restrict__ kb) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i < n) kb[i] = skey[rows[i]];
}

__global__ void k_mr_viol_init(unsigned long long *viol, int64_t K) {
    const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (k < K) viol[k] = MR_NO_VIOL;
}

// rows[i]: the pairing's rows by (key, process), history order inside a run.
// Among the rows of a run that are not :info (none is here), an :invoke after an
// :invoke is a double invocation and a completion after anything else an orphan;
// an :invoke's completion is its successor. The invocation's thread classifies
// the op: link[call] = the completion row or -1, link[ret] = the call row,
// src[call] = the row whose txn the op takes.
__global__ void __launch_bounds__(256) k_mr_pair(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ kb,
                                                 int64_t n, const int64_t *__restrict__ process,
                                                 const int64_t *__restrict__ type, const uint4 *__restrict__ nf,
                                                 const uint8_t *__restrict__ nflag, unsigned long long *viol,
                                                 uint8_t *__restrict__ role, int32_t *__restrict__ link,
                                                 uint32_t *__restrict__ src) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = rows[i], k = kb[i];
    const int64_t p = process[r];
    const bool inv = type[r] == T_INVOKE;
    bool prev_inv = false;
    if (i > 0 && kb[i - 1] == k) {
        const uint32_t q = rows[i - 1];
        prev_inv = process[q] == p && type[q] == T_INVOKE;
    }
    if (inv ? prev_inv : !prev_inv)
        atomicMin(&viol[k], (unsigned long long)r * 8 + (inv ? JH_CAUSE_DOUBLE_INVOKE : JH_CAUSE_ORPHAN));
    if (!inv) return;
    int64_t c = -1;
    if (i + 1 < n && kb[i + 1] == k) {
        const uint32_t q = rows[i + 1];
        if (process[q] == p && type[q] != T_INVOKE) c = q;
    }
    uint32_t s = r;
    bool keep;
    if (c < 0) keep = nflag[r] & NF_WRITES;                              // crashed: only its writes matter
    else if (type[c] == T_FAIL) keep = false;
    else {
        if (!(nflag[c] & NF_NIL)) s = (uint32_t)c;                        // the completion's txn when it has one
        const uint4 f = nf[s];
        keep = (nflag[s] & (NF_NEVER | NF_WRITES)) || f.x != 0;           // the identity constrains nothing
    }
    if (!keep) return;
    role[r] = ROLE_CALL;
    link[r] = c >= 0 ? (int32_t)c : -1;
    src[r] = s;
    if (c >= 0) { role[c] = ROLE_RET; link[c] = (int32_t)r; }
}

// One wave per key over its rows in history order: the ops, the :ok returns and
// the windows' sizes (the kept ops called before return t and open there, the
// returning one left out). Decides every key that needs no search.
__global__ void __launch_bounds__(64) k_mr_count(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ off,
                                                 int64_t K, const uint8_t *__restrict__ role,
                                                 const unsigned long long *__restrict__ viol, MrKey *__restrict__ keys,
                                                 unsigned long long *__restrict__ cnt3, uint32_t *__restrict__ cost,
                                                 uint32_t *__restrict__ order, jh_key_verdict *__restrict__ out,
                                                 MrMeta *m) {
    const int lane = threadIdx.x;
    const unsigned long long lt = (1ULL << lane) - 1;
    for (int64_t k = blockIdx.x; k < K; k += gridDim.x) {
        const uint32_t r0 = off[k], r1 = off[k + 1];
        uint32_t n_ops = 0, n_ok = 0, max_w = 0, open = 0;
        unsigned long long sum_w = 0;
        for (uint32_t base = r0; base < r1; base += 64) {                 // (the same trip count for every lane)
            const uint32_t i = base + lane;
            const uint8_t ro = i < r1 ? role[rows[i]] : ROLE_NONE;
            const unsigned long long calls = __ballot(ro == ROLE_CALL), rets = __ballot(ro == ROLE_RET);
            uint32_t w = 0;
            if (ro == ROLE_RET) w = open + __popcll(calls & lt) - __popcll(rets & lt) - 1;
            uint32_t ws = w, wm = w;
            for (int o = 32; o > 0; o >>= 1) { ws += __shfl_xor(ws, o); wm = max(wm, (uint32_t)__shfl_xor(wm, o)); }
            sum_w += ws; max_w = max(max_w, wm);
            n_ops += __popcll(calls); n_ok += __popcll(rets);
            open += __popcll(calls) - __popcll(rets);
        }
        if (lane != 0) continue;
        jh_key_verdict v;
        memset(&v, 0, sizeof v);
        v.valid = JH_VALID; v.cause = JH_CAUSE_NONE; v.fail_entry = -1; v.explored = 0;
        v.previous_ok = -1; v.last_op = -1; v.analyzer = JH_ANALYZER_WGL;
        bool search = false;
        const unsigned long long vi = viol[k];
        if (r0 == r1) v.explored = -1;                                    // a key in no client row
        else if (vi != MR_NO_VIOL) { v.valid = JH_UNKNOWN; v.cause = (int32_t)(vi & 7); }
        else if (n_ok == 0) {}
        else if (max_w > JH_MR_MAX_WINDOW || n_ok >= MR_OK_LIMIT) { v.valid = JH_UNKNOWN; v.cause = JH_CAUSE_WINDOW; }
        else search = true;
        out[k] = v;
        MrKey kr;
        kr.n_ops = n_ops; kr.n_ok = n_ok; kr.max_w = max_w; kr.searched = search; kr.sum_w = sum_w;
        keys[k] = kr;
        cnt3[k] = search ? n_ops : 0;
        cnt3[(K + 1) + k] = search ? n_ok : 0;
        cnt3[2 * (K + 1) + k] = search ? sum_w : 0;
        // the queue's order: widest window sum first (a radix sort on the complement); the unsearched keys last
        cost[k] = search ? 0xFFFFFFFEu - (uint32_t)min(sum_w, 0xFFFFFFFEULL) : 0xFFFFFFFFu;
        order[k] = (uint32_t)k;
        if (search) { atomicAdd(&m->n_search, 1u); atomicMax(&m->max_ops, n_ops); }
    }
}

// One wave per searched key: its ops in call order, its layers and windows.
__global__ void __launch_bounds__(64) k_mr_fill(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ off,
                                                int64_t K, const uint8_t *__restrict__ role,
                                                const int32_t *__restrict__ link, const uint32_t *__restrict__ src,
                                                const uint4 *__restrict__ nf, const uint8_t *__restrict__ nflag,
                                                const MrKey *__restrict__ keys,
                                                const unsigned long long *__restrict__ scan3,
                                                uint32_t *__restrict__ opidx, uint4 *__restrict__ ops,
                                                int32_t *__restrict__ oprr, MrLayer *__restrict__ layers,
                                                uint32_t *__restrict__ wnd, MrTab *__restrict__ tabs) {
    const int lane = threadIdx.x;
    const unsigned long long lt = (1ULL << lane) - 1;
    for (int64_t k = blockIdx.x; k < K; k += gridDim.x) {
        if (!keys[k].searched) continue;                                  // (the same for every lane)
        const unsigned long long ooff = scan3[k], loff = scan3[(K + 1) + k], woff = scan3[2 * (K + 1) + k];
        if (lane == 0) { MrTab t; t.ooff = ooff; t.loff = loff; t.woff = woff; tabs[k] = t; }
        const uint32_t r0 = off[k], r1 = off[k + 1];
        // pass a: every call row's op, numbered in call order
        uint32_t n_ops = 0;
        for (uint32_t base = r0; base < r1; base += 64) {
            const uint32_t i = base + lane;
            const uint32_t r = i < r1 ? rows[i] : 0;
            const bool call = i < r1 && role[r] == ROLE_CALL;
            const unsigned long long calls = __ballot(call);
            if (call) {
                const uint32_t j = n_ops + __popcll(calls & lt);
                const uint32_t s = src[r];
                uint4 f = nf[s];
                if (nflag[s] & NF_NEVER) { f.x = 0; f.y = 1; }            // rval outside rmask: never consistent
                ops[ooff + j] = f;
                oprr[ooff + j] = -1;                                      // crashed until its return is met
                opidx[r] = j;
            }
            n_ops += __popcll(calls);
        }
        __threadfence();                                                  // pass b reads opidx and rewrites oprr
        // pass b: the events in history order. The open ops, in call order, sit in the lanes: position q in
        // act0 (q < 64) or act1 (q - 64). A searched key has at most 65 open at a return; where more are open
        // no return follows, and the positions past 127 are not kept.
        uint32_t act0 = 0, act1 = 0, na = 0, t = 0, used = 0;
        for (uint32_t base = r0; base < r1; base += 64) {
            const uint32_t i = base + lane;
            const uint32_t r = i < r1 ? rows[i] : 0;
            const uint8_t ro = i < r1 ? role[r] : ROLE_NONE;
            uint32_t j = 0;
            if (ro == ROLE_CALL) j = opidx[r];
            else if (ro == ROLE_RET) j = opidx[(uint32_t)link[r]];
            unsigned long long ev = __ballot(ro != ROLE_NONE);
            while (ev) {                                                  // (wave-uniform)
                const int e = __ffsll((long long)ev) - 1;
                ev &= ev - 1;
                const uint32_t ej = __shfl(j, e), er = __shfl(r, e);
                const bool is_call = __shfl((int)ro, e) == ROLE_CALL;
                if (is_call) {
                    if (na < 64) { if (lane == (int)na) act0 = ej; }
                    else if (na < 128) { if (lane == (int)na - 64) act1 = ej; }
                    na++;
                    continue;
                }
                const unsigned long long at0 = __ballot(lane < (int)na && act0 == ej);
                const unsigned long long at1 = __ballot(64 + lane < (int)na && act1 == ej);
                const int pos = at0 ? __ffsll((long long)at0) - 1 : 64 + __ffsll((long long)at1) - 1;
                if (lane < (int)na && lane != pos) wnd[woff + used + lane - (lane > pos)] = act0;
                if (64 + lane < (int)na && 64 + lane != pos) wnd[woff + used + 64 + lane - (64 + lane > pos)] = act1;
                if (lane == 0) {
                    MrLayer L;
                    L.wrel = used; L.ret_row = er; L.w_pos = (na - 1) | (uint32_t)pos << 8; L.ret_op = ej;
                    layers[loff + t] = L;
                    oprr[ooff + ej] = (int32_t)t;
                }
                used += na - 1; t++;
                // the returned op leaves the open list
                const uint32_t n0 = __shfl_down(act0, 1), n1 = __shfl_down(act1, 1), first1 = __shfl(act1, 0);
                if (pos < 64) {
                    if (lane >= pos) act0 = lane < 63 ? n0 : first1;
                    if (lane < 63) act1 = n1;
                } else if (lane >= pos - 64 && lane < 63) act1 = n1;
                na--;
            }
        }
    }
}

struct MrSearch {
    const uint32_t *order;
    uint32_t n_search;
    uint32_t *head;
    const MrKey *keys;
    const MrTab *tabs;
    const uint4 *ops;
    const int32_t *oprr;
    const MrLayer *layers;
    const uint32_t *wnd;
    unsigned long long *memo;        // waves * cap entries of two words: mask, (generation : layer) << 32 | state
    unsigned long long cap;
    unsigned long long *stack;       // waves * stack_cap frames of three words
    unsigned long long stack_cap;
    uint32_t *gen;                   // a table's last generation
    long long budget;
    uint32_t s0;
    jh_key_verdict *out;
};

__device__ __forceinline__ unsigned long long ld_l2(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_l2(unsigned long long *p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t bcast32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ unsigned long long bcast64(unsigned long long v) {
    return (unsigned long long)bcast32((uint32_t)(v >> 32)) << 32 | bcast32((uint32_t)v);
}

// Is (cm, tag) in the table? If not, slot = where it goes: the first slot of its probe sequence that does not
// hold this generation (at most half the table does).
__device__ __forceinline__ bool mr_absent(const unsigned long long *memo, unsigned long long cmask, uint32_t gen,
                                          unsigned long long cm, unsigned long long tag, unsigned long long &slot) {
    slot = jh_mix64(cm * 0x9E3779B97F4A7C15ULL ^ tag) & cmask;
    for (;;) {
        const unsigned long long w1 = ld_l2(&memo[2 * slot + 1]);
        if ((uint32_t)(w1 >> (32 + MR_TBITS)) != gen) return true;
        if (w1 == tag && ld_l2(&memo[2 * slot]) == cm) return false;
        slot = (slot + 1) & cmask;
    }
}

// The WGL search of one key by one wave: a configuration is
// (t, mask, state); candidates in call order; after a lift the scan restarts,
// after a pop it resumes behind the popped candidate; the child is inserted into
// the memo before descending. The lanes evaluate the window's candidates at once
// -- one step each, then the memo probes, the returning op's child on a lane that
// has no candidate -- and the first consistent candidate in call order whose
// child is absent is taken: the order of the sequential search. The memo and the
// stack are read and written past L1 (an entry's writer is another lane than its
// later readers).
__global__ void __launch_bounds__(64) k_mr_search(MrSearch A) {
    const int lane = threadIdx.x;
    const unsigned long long lt = (1ULL << lane) - 1;
    unsigned long long *memo = A.memo + 2 * A.cap * blockIdx.x;
    unsigned long long *stack = A.stack + 3 * A.stack_cap * blockIdx.x;
    const unsigned long long cmask = A.cap - 1;
    uint32_t gen = A.gen[blockIdx.x];
    for (;;) {
        uint32_t q = 0;
        if (lane == 0) q = atomicAdd(A.head, 1u);
        q = bcast32(q);
        if (q >= A.n_search) break;
        const uint32_t k = A.order[q];
        const MrTab tab = A.tabs[k];
        const uint32_t n_ok = A.keys[k].n_ok;
        if (++gen > MR_GEN_MAX) {                                         // the tags wrap: one clear
            for (unsigned long long i = lane; i < 2 * A.cap; i += 64) st_l2(&memo[i], 0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            gen = 1;
        }
        uint32_t t = 0, s = A.s0, start = 0, tmax = 0, loaded = ~0u;
        unsigned long long depth = 0, mask = 0;
        long long count = 0;
        int verdict = -1;
        // the layer: the window in the lanes, the returning op apart
        uint32_t w = 0, retpos = 0;
        uint4 f = make_uint4(0, 1, 0, 0), fr = f;
        int32_t rr = -1;
        while (verdict < 0) {
            if (loaded != t) {
                const MrLayer L = A.layers[tab.loff + t];
                w = L.w_pos & 255; retpos = L.w_pos >> 8;
                fr = A.ops[tab.ooff + L.ret_op];
                if (lane < (int)w) {
                    const uint32_t j = A.wnd[tab.woff + L.wrel + lane];
                    f = A.ops[tab.ooff + j];
                    rr = A.oprr[tab.ooff + j];
                }
                loaded = t;
            }
            const bool in = lane < (int)w, lin = in && ((mask >> lane) & 1);
            const uint32_t idx = lane + (lane >= (int)retpos);            // the member's place in W(t)'s call order
            const bool cand = in && idx >= start && !lin && (s & f.x) == f.y;
            const uint32_t s2 = (s & ~f.z) | f.w;
            const unsigned long long cm = mask | (1ULL << lane);
            // the returning op's child: t advances past every return already linearized, the mask is compacted
            // onto the new window (the members that stay open lead it, in order; the next returning op leaves)
            const bool retc = retpos >= start && (s & fr.x) == fr.y;      // (wave-uniform)
            uint32_t ru = t + 1;
            unsigned long long rm = 0;
            const uint32_t rs2 = (s & ~fr.z) | fr.w;
            if (retc) {
                while (ru < n_ok && __ballot(lin && rr == (int32_t)ru)) ru++;
                if (ru < n_ok) {
                    const bool keep = in && (rr < 0 || rr > (int32_t)ru);
                    const unsigned long long kp = __ballot(keep);
                    rm = keep && lin ? 1ULL << __popcll(kp & lt) : 0;
                    for (int o = 32; o > 0; o >>= 1) rm |= __shfl_xor(rm, o);
                }
            }
            const unsigned long long busy = __ballot(cand);
            const int rl = retc && ~busy ? __ffsll((long long)~busy) - 1 : -1;   // the lane that probes for the returning op
            const bool for_ret = lane == rl;
            const unsigned long long pm = for_ret ? rm : cm;
            const unsigned long long tag = ((unsigned long long)(gen << MR_TBITS | (for_ret ? ru : t)) << 32) | (for_ret ? rs2 : s2);
            bool absent = false;
            unsigned long long slot = 0;
            if (cand || for_ret) absent = mr_absent(memo, cmask, gen, pm, tag, slot);
            const unsigned long long ab = __ballot(absent && cand);
            bool rabs = __ballot(absent && for_ret) != 0;
            unsigned long long rslot = 0;
            const unsigned long long rtag = ((unsigned long long)(gen << MR_TBITS | ru) << 32) | rs2;
            if (retc && rl < 0) {                                         // every lane has a candidate: one more round
                if (lane == 0) rabs = mr_absent(memo, cmask, gen, rm, rtag, rslot);
                rabs = __ballot(rabs && lane == 0) != 0;
            }
            const unsigned long long below = retpos >= 64 ? ~0ULL : (1ULL << retpos) - 1;
            int take = -1;                                                // a lane, or 64: the returning op
            if (ab & below) take = __ffsll((long long)(ab & below)) - 1;
            else if (rabs) take = 64;
            else if (ab) take = __ffsll((long long)ab) - 1;
            if (take < 0) {                                               // nothing to take here: pop
                if (depth == 0) { verdict = JH_INVALID; break; }
                depth--;
                unsigned long long a = 0, b = 0, c = 0;
                if (lane == 0) {
                    a = ld_l2(&stack[3 * depth]); b = ld_l2(&stack[3 * depth + 1]); c = ld_l2(&stack[3 * depth + 2]);
                }
                mask = bcast64(a); b = bcast64(b); c = bcast64(c);
                t = (uint32_t)(b >> 32); start = (uint32_t)b + 1; s = (uint32_t)c;
                continue;
            }
            if (count >= A.budget) { verdict = JH_UNKNOWN; break; }
            if (take == 64) {
                if (rl >= 0) { if (for_ret) { st_l2(&memo[2 * slot], rm); st_l2(&memo[2 * slot + 1], rtag); } }
                else if (lane == 0) { st_l2(&memo[2 * rslot], rm); st_l2(&memo[2 * rslot + 1], rtag); }
            } else if (lane == take) { st_l2(&memo[2 * slot], cm); st_l2(&memo[2 * slot + 1], tag); }
            const uint32_t tidx = take == 64 ? retpos : (uint32_t)take + ((uint32_t)take >= retpos);
            if (lane == 0) {
                st_l2(&stack[3 * depth], mask);
                st_l2(&stack[3 * depth + 1], (unsigned long long)t << 32 | tidx);
                st_l2(&stack[3 * depth + 2], s);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the entry is in L2 before the next probes
            count++; depth++;
            if (take == 64) { t = ru; s = rs2; mask = rm; }
            else { s = bcast32(__shfl(s2, take)); mask = bcast64(__shfl(cm, take)); }
            start = 0;
            if (t > tmax) tmax = t;
            if (t == n_ok) verdict = JH_VALID;
        }
        if (lane == 0) {
            jh_key_verdict v;
            memset(&v, 0, sizeof v);
            v.valid = verdict; v.cause = verdict == JH_UNKNOWN ? JH_CAUSE_BUDGET : JH_CAUSE_NONE;
            v.fail_entry = verdict == JH_INVALID ? (int64_t)A.layers[tab.loff + tmax].ret_row : -1;
            v.explored = count; v.previous_ok = -1; v.last_op = -1; v.analyzer = JH_ANALYZER_WGL;
            A.out[k] = v;
        }
    }
    if (lane == 0) A.gen[blockIdx.x] = gen;
}

int bits_of(unsigned long long v) {
    int b = 1;
    while (b < 64 && (v >> b)) b++;
    return b;
}
}  // namespace

void multi_register_check(jh_ctx *ctx, const jh_history *dh, const jh_multi_register_opts *opts, jh_key_verdict *out,
                          jh_summary *sum, hipStream_t st) {
    if (sum) { memset(sum, 0, offsetof(jh_summary, bfs_stall_picks)); sum->first_fail_entry = -1; }   // ABI 8's layout
    const int64_t n = dh->n;
    const bool keyed = dh->key != nullptr && dh->n_keys > 0;
    const int64_t K = keyed ? dh->n_keys : 1;
    const int n_regs = opts->n_regs, bits = opts->bits;
    if (n_regs < 0 || bits < 0) throw_jh(JH_EINVAL, "multi-register: negative n_regs or bits");
    if ((int64_t)n_regs * bits > 32 || n_regs > 32)
        throw_jh(JH_EUNSUPPORTED, "multi-register: the packed state exceeds 32 bits, or more than 32 registers");
    if (K >= (1LL << 31) - 2) throw_jh(JH_EUNSUPPORTED, "multi-register: more than 2^31 - 3 keys");
    if (n >= (1LL << 31)) throw_jh(JH_EUNSUPPORTED, "multi-register: 2^31 rows or more");
    uint32_t s0 = 0;
    for (int r = 0; r < n_regs && opts->init; r++) {
        int64_t v = opts->init[r];
        if (v == JH_NIL) v = 0;
        if (v < 0 || v >= (1LL << bits)) throw_jh(JH_EINVAL, "multi-register: an initial value id outside [0, 2^bits)");
        s0 |= (uint32_t)((uint64_t)v << (r * bits));
    }
    const long long budget = opts->budget > 0 ? opts->budget : JH_DEFAULT_BUDGET;
    if (budget > (1LL << 36)) throw_jh(JH_EINVAL, "multi-register: budget above 2^36");
    for (int64_t k = 0; k < K; k++) {
        memset(&out[k], 0, sizeof(jh_key_verdict));
        out[k].valid = JH_VALID; out[k].fail_entry = out[k].previous_ok = out[k].last_op = -1;
        out[k].explored = -1; out[k].analyzer = JH_ANALYZER_WGL;
    }
    if (n == 0) return;                                                   // no key is in any row
    DeviceTimer timer{ctx, st};
    timer.start();

    // 1. rows: sort keys, normal forms, refusals
    MrMeta *m = ctx->ws<MrMeta>(WS_MR_META, 1);
    HIP_TRY(hipMemsetAsync(m, 0, sizeof(MrMeta), st));
    uint32_t *skey = ctx->ws<uint32_t>(WS_MR_SKEY, n), *skey2 = ctx->ws<uint32_t>(WS_MR_SKEY2, n);
    uint32_t *rowid = ctx->ws<uint32_t>(WS_MR_ROWID, n), *rows = ctx->ws<uint32_t>(WS_MR_ROWS, n);
    uint8_t *inc = ctx->ws<uint8_t>(WS_MR_INC, n), *nflag = ctx->ws<uint8_t>(WS_MR_FLAG, n);
    uint8_t *role = ctx->ws<uint8_t>(WS_MR_ROLE, n);
    uint4 *nf = ctx->ws<uint4>(WS_MR_NF, n);
    int32_t *link = ctx->ws<int32_t>(WS_MR_LINK, n);
    uint32_t *src = ctx->ws<uint32_t>(WS_MR_SRC, n), *opidx = ctx->ws<uint32_t>(WS_MR_OPIDX, n);
    k_mr_rows<<<grid_for(n, 256, 1 << 23), 256, 0, st>>>(dh->process, dh->type, dh->key, dh->value, dh->value2, dh->aux,
                                                         dh->n_aux, n, K, keyed ? 1 : 0, n_regs, bits, skey, rowid, inc,
                                                         nf, nflag, role, m);
    // 2. the stable key partition, and the pairing's rows
    sort_pairs(ctx, WS_MR_TMP, as_input(skey), skey2, as_input(rowid), rows, (int)n, bits_of((unsigned long long)K), st);
    uint32_t *off = ctx->ws<uint32_t>(WS_MR_OFF, K + 1);
    k_mr_off<<<grid_for(K + 1, 256, 1 << 23), 256, 0, st>>>(skey2, n, K, off);
    uint32_t *ra = ctx->ws<uint32_t>(WS_MR_RA, n), *rb = ctx->ws<uint32_t>(WS_MR_RB, n);
    select_flagged(ctx, WS_MR_TMP, as_input(rowid), as_input(inc), ra, &m->n_inc, (int)n, st);
    const MrMeta mh = fetch(m, st);
    if (mh.flags & MR_BAD_KEY) throw_jh(JH_EINVAL, "multi-register: a key outside [0, n_keys)");
    if (mh.flags & MR_BAD_RANGE) throw_jh(JH_EINVAL, "multi-register: a txn's triples leave aux or have a negative count");
    if (mh.flags & MR_BAD_REG) throw_jh(JH_EINVAL, "multi-register: a register outside [0, n_regs)");
    if (mh.flags & MR_BAD_VAL) throw_jh(JH_EINVAL, "multi-register: a value id outside [0, 2^bits)");
    if (mh.flags & MR_BAD_F) throw_jh(JH_EINVAL, "multi-register: a micro-op that is neither a read nor a write");
    if (mh.flags & MR_UNSUP_KEY) throw_jh(JH_EUNSUPPORTED, "multi-register: a client row without a key in a keyed history");
    if (mh.flags & MR_UNSUP_MOPS) throw_jh(JH_EUNSUPPORTED, "multi-register: a txn of more than JH_CY_MAX_MOPS micro-ops");
    unsigned long long *viol = ctx->ws<unsigned long long>(WS_MR_VIOL, K);
    k_mr_viol_init<<<grid_for(K, 256, 1 << 23), 256, 0, st>>>(viol, K);
    const int64_t ni = mh.n_inc;
    if (ni > 0) {
        unsigned long long *pk = ctx->ws<unsigned long long>(WS_MR_PK, ni), *pk2 = ctx->ws<unsigned long long>(WS_MR_PK2, ni);
        uint32_t *kb = ctx->ws<uint32_t>(WS_MR_KB, ni), *kb2 = ctx->ws<uint32_t>(WS_MR_KB2, ni);
        const int g = grid_for(ni, 256, 1 << 23);
        k_mr_pk<<<g, 256, 0, st>>>(ra, ni, dh->process, pk);
        sort_pairs(ctx, WS_MR_TMP, as_input(pk), pk2, as_input(ra), rb, (int)ni, bits_of(mh.max_proc), st);
        k_mr_kb<<<g, 256, 0, st>>>(rb, ni, skey, kb);
        sort_pairs(ctx, WS_MR_TMP, as_input(kb), kb2, as_input(rb), ra, (int)ni, bits_of((unsigned long long)K), st);
        k_mr_pair<<<g, 256, 0, st>>>(ra, kb2, ni, dh->process, dh->type, nf, nflag, viol, role, link, src);
    }

    // 3. per key: sizes and the early verdicts
    MrKey *keys = ctx->ws<MrKey>(WS_MR_KEYS, K);
    unsigned long long *cnt3 = ctx->ws<unsigned long long>(WS_MR_CNT, 3 * (K + 1));
    unsigned long long *scan3 = ctx->ws<unsigned long long>(WS_MR_SCAN, 3 * (K + 1));
    uint32_t *cost = ctx->ws<uint32_t>(WS_MR_COST, K), *cost2 = ctx->ws<uint32_t>(WS_MR_COST2, K);
    uint32_t *order = ctx->ws<uint32_t>(WS_MR_ORDER, K), *order2 = ctx->ws<uint32_t>(WS_MR_ORDER2, K);
    jh_key_verdict *dv = ctx->ws<jh_key_verdict>(WS_MR_OUT, K);
    HIP_TRY(hipMemsetAsync(cnt3, 0, sizeof(unsigned long long) * 3 * (K + 1), st));
    const int gk = grid_for(K, 1, 1 << 16);
    k_mr_count<<<gk, 64, 0, st>>>(rows, off, K, role, viol, keys, cnt3, cost, order, dv, m);
    for (int a = 0; a < 3; a++)
        excl_sum(ctx, WS_MR_TMP, as_input(cnt3 + a * (K + 1)), scan3 + a * (K + 1), (int)(K + 1), st);
    sort_pairs(ctx, WS_MR_TMP, as_input(cost), cost2, as_input(order), order2, (int)K, 32, st);
    unsigned long long tot[3];
    for (int a = 0; a < 3; a++)
        HIP_TRY(hipMemcpyAsync(&tot[a], scan3 + a * (K + 1) + K, sizeof tot[a], hipMemcpyDeviceToHost, st));
    const MrMeta mk = fetch(m, st);

    // 4. the searched keys' tables and the search
    int waves = 0;
    if (mk.n_search > 0) {
        uint4 *ops = ctx->ws<uint4>(WS_MR_OPS, tot[0]);
        int32_t *oprr = ctx->ws<int32_t>(WS_MR_OPRR, tot[0]);
        MrLayer *layers = ctx->ws<MrLayer>(WS_MR_LAYERS, tot[1]);
        uint32_t *wnd = ctx->ws<uint32_t>(WS_MR_WND, tot[2]);
        MrTab *tabs = ctx->ws<MrTab>(WS_MR_TABS, K);
        k_mr_fill<<<gk, 64, 0, st>>>(rows, off, K, role, link, src, nf, nflag, keys, scan3, opidx, ops, oprr, layers, wnd,
                                     tabs);
        // one memo table and one stack per wave; a table holds at least twice the budget
        unsigned long long cap = 64;
        while (cap < 2ULL * (unsigned long long)budget) cap <<= 1;
        const unsigned long long stack_cap = (unsigned long long)mk.max_ops + 1;
        const size_t per_wave = (size_t)cap * 16 + (size_t)stack_cap * 24;
        const int max_waves = 4 * std::max(ctx->n_cu, 1);
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const size_t held = ctx->ws_fresh(WS_MR_MEMO) ? 0 : ctx->bufs[WS_MR_MEMO].bytes;   // ours already
        const size_t fit = (free_b / 4 + held) / (per_wave + per_wave / 8 + 1);
        if (fit < 1) throw_jh(JH_ENOMEM, "multi-register: no room for one memo table of 2 x budget entries");
        waves = (int)std::min<size_t>({(size_t)mk.n_search, (size_t)max_waves, fit});
        if (opts->waves > 0) waves = std::min(waves, opts->waves);
        // the tags of an earlier call mean something only in the same allocation under the same table size:
        // decided before ws() grows a slot (a larger buffer may come back at the address of the freed one)
        const size_t memo_need = sizeof(unsigned long long) * (size_t)waves * cap * 2;
        const bool fresh = ctx->ws_fresh(WS_MR_MEMO) || ctx->bufs[WS_MR_MEMO].bytes < memo_need ||
                           ctx->ws_fresh(WS_MR_GEN) || ctx->bufs[WS_MR_GEN].bytes < sizeof(uint32_t) * max_waves ||
                           ctx->mr_cap != cap;
        ctx->mr_cap = 0;                                                  // (a call that fails below leaves no live tags)
        unsigned long long *memo = ctx->ws<unsigned long long>(WS_MR_MEMO, (size_t)waves * cap * 2);
        unsigned long long *stack = ctx->ws<unsigned long long>(WS_MR_STACK, (size_t)waves * stack_cap * 3);
        uint32_t *gen = ctx->ws<uint32_t>(WS_MR_GEN, max_waves);
        if (fresh || (opts->flags & JH_MR_GEN_JUMP)) {
            HIP_TRY(hipMemsetAsync(memo, 0, ctx->bufs[WS_MR_MEMO].bytes, st));
            HIP_TRY(hipMemsetAsync(gen, 0, sizeof(uint32_t) * max_waves, st));
        }
        ctx->mr_cap = cap;
        // the hook starts every table (all clear) just below the wrap
        if (opts->flags & JH_MR_GEN_JUMP) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)gen, (int)(MR_GEN_MAX - 1), max_waves, st));
        MrSearch A;
        A.order = order2; A.n_search = mk.n_search; A.head = &m->head; A.keys = keys; A.tabs = tabs; A.ops = ops;
        A.oprr = oprr; A.layers = layers; A.wnd = wnd; A.memo = memo; A.cap = cap; A.stack = stack; A.stack_cap = stack_cap;
        A.gen = gen; A.budget = budget; A.s0 = s0; A.out = dv;
        k_mr_search<<<waves, 64, 0, st>>>(A);
    }
    HIP_TRY(hipMemcpyAsync(out, dv, sizeof(jh_key_verdict) * K, hipMemcpyDeviceToHost, st));
    const float ms = timer.stop();                                        // (the stream is drained here)
    if (!sum) return;
    sum->valid = JH_VALID; sum->device_ms = ms; sum->waves[0] = waves;
    for (int64_t k = 0; k < K; k++) {
        const jh_key_verdict &v = out[k];
        if (v.explored < 0) continue;
        sum->n_keys++; sum->explored += v.explored;
        if (v.valid == JH_INVALID) {
            sum->n_invalid++;
            if (sum->first_fail_entry < 0 || v.fail_entry < sum->first_fail_entry) sum->first_fail_entry = v.fail_entry;
        } else if (v.valid == JH_UNKNOWN) sum->n_unknown++;
    }
    sum->valid = sum->n_invalid ? JH_INVALID : sum->n_unknown ? JH_UNKNOWN : JH_VALID;
}
