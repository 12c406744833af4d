/*
 * jh.h -- C ABI of libjh.so, the MI355X-native Jepsen history checker.
 *
 * This is the drop-in boundary for the verification phase of Jepsen
 * (reference: jepsen "0.1.14-SNAPSHOT", /root/reference/jepsen/project.clj:1).
 * Each entry point replaces one `jepsen.checker/Checker` reify on the JVM
 * side; a JNA shim encodes the history once into the
 * columnar layout below and calls:
 *
 *   jh_check_cas_independent  <- (independent/checker (checker/linearizable
 *                                   {:model (model/cas-register v0)}))
 *                                 jepsen/src/jepsen/independent.clj:247-298
 *                                 jepsen/src/jepsen/checker.clj:127-158
 *   jh_check_cas              <- (checker/linearizable {:model (model/cas-register)})
 *                                 jepsen/src/jepsen/checker.clj:127-158
 *   jh_check_counter          <- (checker/counter)  jepsen/src/jepsen/checker.clj:679-734
 *   jh_check_set              <- (checker/set)      jepsen/src/jepsen/checker.clj:182-233
 *   jh_check_set_full         <- (checker/set-full {:linearizable? b})
 *                                                   jepsen/src/jepsen/checker.clj:236-534
 *   jh_check_total_queue      <- (checker/total-queue) jepsen/src/jepsen/checker.clj:536-628
 *   jh_check_queue            <- (checker/queue (model/unordered-queue))
 *                                                   jepsen/src/jepsen/checker.clj:160-180
 *   jh_check_unique_ids       <- (checker/unique-ids) jepsen/src/jepsen/checker.clj:631-676
 *   jh_check_bank             <- (jepsen.tests.bank/checker opts)
 *                                                   jepsen/src/jepsen/tests/bank.clj:46-121
 *   jh_check_long_fork        <- (jepsen.tests.long-fork/checker n)
 *                                                   jepsen/src/jepsen/tests/long_fork.clj:158-324
 *   jh_check_causal_reverse   <- (independent/checker (jepsen.tests.causal-reverse/checker))
 *                                                   jepsen/src/jepsen/tests/causal_reverse.clj:21-84
 *   jh_check_set_independent  <- (independent/checker (checker/set))
 *                                                   jepsen/src/jepsen/independent.clj:247-298
 *                                                   jepsen/src/jepsen/checker.clj:182-233
 *   jh_check_causal           <- (independent/checker (jepsen.tests.causal/check (causal-register)))
 *                                                   jepsen/src/jepsen/tests/causal.clj:33-110
 *   jh_check_g2               <- (jepsen.tests.adya/g2-checker)
 *                                                   jepsen/src/jepsen/tests/adya.clj:62-88
 *   jh_check_cycle            <- (jepsen.tests.cycle/checker (cycle/combine ...))
 *                                                   jepsen/src/jepsen/tests/cycle.clj:202-216,911-934
 *   jh_scc                    <- cycle/tarjan       jepsen/src/jepsen/tests/cycle.clj:150-160
 *   jh_perf                   <- (checker/perf), (checker/latency-graph), (checker/rate-graph):
 *                                 the reduction behind the three plots
 *                                                   jepsen/src/jepsen/checker.clj:736-768
 *                                                   jepsen/src/jepsen/checker/perf.clj
 *   jh_check_multi_register   <- (independent/checker (checker/linearizable {:model (multi-register {})}))
 *                                                   yugabyte/src/yugabyte/multi_key_acid.clj:20-42,112-127
 *
 * Plain pointers and sizes only. The caller owns every buffer; the library
 * never retains a caller pointer after returning. All entry points are
 * reentrant: one jh_ctx serialises its device work with a mutex.
 *
 * History encoding (one row per history map, in history order; the row
 * number IS knossos' :index, jepsen/src/jepsen/core.clj:441):
 *   process  >= 0 for an integer client process; < 0 for anything else
 *            (:nemesis is -1, other non-integers are interned to -2, -3, ...)
 *   type     JH_TYPE_INVOKE / OK / FAIL / INFO
 *   f        JH_F_READ / WRITE / CAS / ADD, anything else interned >= 16
 *   key      (key v) when :value is an independent tuple (a MapEntry,
 *            jepsen/src/jepsen/independent.clj:21-29), interned to
 *            [0, n_keys); -1 when :value is not a tuple.  May be NULL (= all -1).
 *   value    scalar :value (after unwrapping a tuple); for :cas the `cur`
 *            element of [cur new]; JH_NIL for nil / absent :value.
 *            For a set :read, the offset of its elements in `aux`.
 *   value2   for :cas the `new` element; for a set :read the element count;
 *            JH_NIL otherwise.
 *
 * Bank reads (jh_check_bank only; every other entry point keeps the layout
 * above): an :ok :read whose :value is a map {account balance} has
 *   value    the index of the read's first PAIR, value2 its number of pairs;
 *            pair j of the read is aux[2*(value+j)] (the account code) and
 *            aux[2*(value+j)+1] (the balance, JH_NIL = nil), in the order
 *            (seq (:value op)) yields them; n_aux is even.
 *   A nil :value is value = JH_NIL, value2 = 0 (the empty map).
 *   Account codes: the caller interns accounts; code i is the i-th distinct
 *   element of (:accounts test), any other key gets a code >= n_accounts in
 *   first-appearance order, so "unexpected" is code < 0 || code >= n_accounts.
 *   Ranges need not be contiguous or ordered in aux. Rows of any other f
 *   (:transfer, nemesis) carry value = value2 = JH_NIL and are never read.
 *
 * Long-fork txns (jh_check_long_fork only), in the bank pair layout. f is set
 * from the SHAPE of :value, never from the op's :f:
 *   read txn   (every micro-op [:r k v]; nil and [] included): f = JH_F_READ,
 *            value = the index of its first pair, value2 = its number of
 *            pairs; pair j is aux[2*(value+j)] (the key, a signed int64) and
 *            aux[2*(value+j)+1] (the value, JH_NIL = nil), in micro-op order.
 *            A nil :value is value = JH_NIL, value2 = 0; an empty txn has
 *            value2 = 0. Only :ok rows' ranges are read; ranges need not be
 *            contiguous or ordered in aux.
 *   write txn  (exactly one micro-op, a [:w k v]): f = JH_F_WRITE, value = k,
 *            value2 = v.
 *   any other row (a mixed txn, nemesis): an interned f >= 16 and value =
 *            value2 = JH_NIL.
 *   Keys that are not integers, and values that are not integers or nil, have
 *   no encoding.
 *
 * Causal-reverse (jh_check_causal_reverse only): the standard columns. A
 * :write has f = JH_F_WRITE and value = the written integer (never JH_NIL); an
 * :ok :read has f = JH_F_READ, value = the offset of its elements in aux and
 * value2 = their number (the set-read layout; a nil or empty :value has
 * value2 = 0, and then value is not looked at). `key` as in
 * jh_check_cas_independent; key == NULL or n_keys == 0 is one un-keyed history.
 *
 * Cycle txns (jh_check_cycle with JH_CY_WR only): an :ok txn row has value = the
 * index of its first micro-op and value2 = its number of micro-ops; micro-op j
 * is the triple aux[3*(value+j) .. +3) = [f, k, v] with f = JH_F_READ /
 * JH_F_WRITE, k an int64 the caller interned and v an int64 or JH_NIL; n_aux is
 * a multiple of 3. A nil :value is value = JH_NIL, value2 = 0. Rows of other
 * types are not read.
 *
 * Append txns (jh_check_cycle with JH_CY_APPEND): every non-nemesis row of every
 * type carries its txn: value = the aux word index of its first micro-op and
 * value2 = its number of micro-ops (a nil :value is JH_NIL, 0). Micro-op j is
 * the four words aux[value + 4j .. +4) = [f, k, a, b]. f = JH_F_READ: a = the aux
 * word index of the read's first element and b = its number of elements (nil
 * and [] are b = 0, and then a is not looked at). f = JH_F_APPEND: a = the
 * element, b = 0. Elements are int64 and never JH_NIL; k is dense,
 * 0 <= k < n_keys.
 *
 * Causal ops (jh_check_causal only): f = JH_F_READ / JH_F_WRITE /
 * JH_F_READ_INIT or an interned id >= 16, value = :value (JH_NIL for nil),
 * value2 unused (0); aux holds 2 n words, aux[2 i] = row i's :position and
 * aux[2 i + 1] = its :link, nil as JH_NIL and :init as JH_CAUSAL_INIT. Values,
 * positions and links are longs in (INT64_MIN + 1, INT64_MAX]; only :ok rows are
 * read. `key` as in jh_check_cas_independent.
 *
 * G2 ops (jh_check_g2 only): f = JH_F_INSERT for :insert, anything else
 * otherwise; key = the interned (key (:value op)). Only type, f and key are read.
 */
#ifndef JH_H
#define JH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JH_ABI_VERSION 8

/* Return codes. Anything non-zero also writes a NUL-terminated message into
 * the caller's err buffer; the JNA shim throws ex-info and check-safe turns
 * it into {:valid? :unknown :error ...} (jepsen/src/jepsen/checker.clj:77-88). */
#define JH_OK            0
#define JH_EINVAL        1   /* malformed arguments or history */
#define JH_EUNSUPPORTED  2   /* input the device path does not handle: shim falls back */
#define JH_EDEVICE       3   /* HIP error, or no device */
#define JH_ENOMEM        4   /* device allocation failed */

/* :type */
#define JH_TYPE_INVOKE 0
#define JH_TYPE_OK     1
#define JH_TYPE_FAIL   2
#define JH_TYPE_INFO   3

/* :f */
#define JH_F_READ  0
#define JH_F_WRITE 1
#define JH_F_CAS   2
#define JH_F_ADD   3
#define JH_F_ENQUEUE 4
#define JH_F_DEQUEUE 5
#define JH_F_DRAIN   6  /* an :ok :drain's :value collection is a CSR range in aux, like a set read */

#define JH_NIL INT64_MIN

/* Verdict codes, ordered like jepsen.checker/valid-priorities
 * (jepsen/src/jepsen/checker.clj:26-31): true 0 < :unknown 0.5 < false 1. */
#define JH_VALID    0
#define JH_UNKNOWN  1
#define JH_INVALID  2

/* Per-key causes. */
#define JH_CAUSE_NONE         0
#define JH_CAUSE_BUDGET       1  /* memo-insert budget exhausted -> :unknown */
#define JH_CAUSE_WINDOW       2  /* more than JH_MAX_WINDOW concurrent ops   */
#define JH_CAUSE_DOUBLE_INVOKE 3 /* knossos.history/complete would throw     */
#define JH_CAUSE_ORPHAN       4  /* :ok/:fail with no open invocation        */
#define JH_CAUSE_BAD_F        5  /* op :f the cas-register model does not know */
#define JH_CAUSE_NIL_VALUE    6  /* nil where the checker does arithmetic     */
#define JH_CAUSE_OVERFLOW     7  /* long overflow (Clojure + throws)          */
#define JH_CAUSE_STATES       8  /* more than 65532 distinct values in one key */
#define JH_CAUSE_DEFERRED     9  /* JH_LIN_PHASE1_ONLY: past the quick budget, not searched further;
                                    explored = the key's rank for the heavy-key pass, heaviest first:
                                    2^31 - 1 - its estimated inserts (the quick search's inserts over
                                    its progress, deepest layer / layers; round 5) */
#define JH_CAUSE_MULTIPLE_WRITES 10 /* long-fork: a key written by two :invoke write txns */
#define JH_CAUSE_ILLEGAL_HISTORY 11 /* long-fork: the reference throws :illegal-history   */

#define JH_MAX_WINDOW 256
/* Per-key limits, each pinned at N and N + 1 by tests/test_gpu_lin_edges.py:
 *  - a widest window of 257 members or more: JH_UNKNOWN / JH_CAUSE_WINDOW;
 *  - 2^20 - 1 or more :ok ops that the search keeps (not failed, not a read of
 *    nil): JH_UNKNOWN / JH_CAUSE_WINDOW for that key alone, explored = 0
 *    (2^20 - 2 are searched);
 *  - more than 65532 distinct values in one key, the initial value included:
 *    JH_UNKNOWN / JH_CAUSE_STATES for that key alone, explored = 0.
 * The value range is taken over the whole call: vmax - vmin over every client
 * read / write / cas value and the initial value. One outlying value in one
 * key therefore decides for every key whether states fit 8 bits (vmax - vmin
 * <= 254: the LDS memo of windows up to 40), whether the reachable-set engine
 * applies (vmax - vmin <= 4093; with JH_ALGO_LINEAR the analyzer is
 * JH_ANALYZER_LINEAR exactly for the searched keys of at most 32 window members
 * then, and fewer than 2^20 - 2 ok ops), and whether values are numbered per
 * key (vmax - vmin >= 65531, or a difference that overflows int64; the two
 * conditions above then read "the largest key's distinct values" + 1 for
 * vmax - vmin + 2). Verdicts, causes, rows and explored do not depend on it. */

typedef struct jh_history {
    int64_t n;                 /* entries */
    const int64_t *process;
    const int64_t *type;
    const int64_t *f;
    const int64_t *key;        /* may be NULL */
    const int64_t *value;
    const int64_t *value2;
    int64_t n_keys;            /* keys are 0..n_keys-1 */
    const int64_t *aux;        /* set-read elements, CSR via value/value2; may be NULL */
    int64_t n_aux;
    int32_t on_device;         /* 1: every pointer above is a device (HBM) pointer */
    int32_t reserved;
} jh_history;

/* :algorithm of (checker/linearizable {:model m :algorithm a}), checker.clj:141-145.
 * Every algorithm decides the same :valid? (all are complete decision
 * procedures); the choice selects which analysis is reported (:analyzer) and,
 * for an invalid key, which search's frontier :configs come from. */
#define JH_ALGO_COMPETITION 0       /* knossos.competition (the default): :wgl and :linear race */
#define JH_ALGO_WGL         1       /* knossos.wgl */
#define JH_ALGO_LINEAR      2       /* knossos.linear (JIT-linearization configuration sets) */

/* jh_lin_opts.flags: test hooks, 0 in production */
#define JH_LIN_BFS_ONLY        1    /* heavy keys: the reachable-set BFS alone (no DFS race) */
#define JH_LIN_GEN_JUMP        2    /* start at the top of the memo generation range (wrap test) */
#define JH_LIN_INTERN_PER_KEY  4    /* intern values per key even when one global range fits */
#define JH_LIN_NO_HELPERS      8    /* no late helper workgroups in phase 2 */
#define JH_LIN_HELPERS_NOW    16    /* late helpers take a key at once (helper_late_us = 0) */
/* Two-stage checking for rebalancing heavy keys across devices (jh_multi,
 * jepsen_amd/shard.py): stage 1 settles every key it can under the quick
 * budget and returns the others as JH_UNKNOWN / JH_CAUSE_DEFERRED; stage 2
 * sends every key that needs a search straight to the heavy-key engines. */
#define JH_LIN_PHASE1_ONLY    32
#define JH_LIN_SKIP_PHASE1    64
/* Phase 1 keeps every key it started until the quick budget (no hand-over of
 * long searches to the heavy-key pass once its queue is empty). */
#define JH_LIN_NO_HANDOVER   128
/* The streaming heavy-key pass: its engines consume phase 1's deferrals as
 * they are made instead of starting after phase 1. Same verdicts; measured
 * slower on C3 (the heavy keys' searches share CUs with phase
 * 1 and start without helpers), so it is off by default. */
#define JH_LIN_STREAM        256
/* Round 5: phase 1 saves each deferred search (stack + memo) and the heavy-key
 * pass continues it; this flag restarts deferred keys from scratch instead
 * (round 4's behaviour; same verdicts and counts, for A/B and the tests). */
#define JH_LIN_NO_RESUME     512
/* Round 5: WGL's exact cache size for every key. Without it, a valid key the
 * reachable-set engine settles (a terminal configuration reachable and at
 * most `budget` configurations reachable: WGL's cache is a subset of them,
 * so WGL could not have run out) is emitted at once with explored =
 * JH_EXPLORED_UNCOUNTED instead of after the count pass -- the reference's
 * map has no :explored (doc/tutorial/04-checker.md:126-138); the parity
 * tests set this flag. */
#define JH_LIN_EXACT_COUNT  1024
#define JH_EXPLORED_UNCOUNTED (-3)
/* Round 6: late helpers with no key of their own enumerate dead-subtree
 * candidates posted by the helpers that run a key's exact search, which merge
 * the dead ones (same verdicts and counts); this flag turns that off (A/B and
 * the tests). */
#define JH_LIN_NO_SPEC      2048
/* Round 6: late helpers serve posted spec jobs before taking keys of their
 * own (scheduling only: same verdicts and counts). */
#define JH_LIN_SPEC_FIRST   4096
/* Round 6: late helpers pick the keys whose sequential search has gone
 * longest without reaching a deeper layer (stuck in a big dead subtree)
 * instead of the ones running longest (scheduling only). */
#define JH_LIN_HELP_STALL   8192
/* Round 6, the takeover (opt-in): a late helper that takes a key phase 2's
 * sequential search is running continues that search's saved state instead
 * of restarting it (JH_LIN_TAKEOVER); JH_LIN_NO_TAKEOVER forces it off. */
#define JH_LIN_NO_TAKEOVER  16384
#define JH_LIN_TAKEOVER     32768
/* Round 8, not a test hook: the caller's jh_lin_opts and jh_summary have the
 * fields added after ABI 8's layout (jh_lin_opts.bfs_stall_min,
 * jh_summary.bfs_stall_picks). Additive to ABI 8: a caller built against the
 * earlier layout never sets it, and the library then reads and writes nothing
 * past that layout (the defaults apply). */
#define JH_LIN_TAIL_FIELDS  65536

typedef struct jh_lin_opts {
    int64_t init_value;        /* (model/cas-register init); JH_NIL = (cas-register) */
    int64_t budget;            /* max memo inserts per key before :unknown; <=0: default */
    int64_t stream;            /* hipStream_t to run on (0 = the ctx stream) */
    int32_t algorithm;         /* JH_ALGO_*; 0 = competition, the reference's default */
    int32_t flags;             /* JH_LIN_* test hooks */
    int64_t quick_budget;      /* phase-1 inserts before a key is deferred; <=0: 8192 */
    int64_t phase2_budget;     /* phase-2 inserts before a key restarts in phase 3; <=0: 65536 */
    /* scheduling of the heavy-key pass (every value decides the same verdicts;
     * the parity tests run the less common paths through these): */
    int32_t helpers;           /* phase-2 late helper workgroups; <=0: 64 (a quarter of the CUs), at most half the CUs (JH_LIN_NO_HELPERS: none) */
    int32_t helper_late_us;    /* > 0: a helper takes the key running longest, once past this run time
                                  (JH_LIN_HELPERS_NOW: at once; JH_LIN_HELP_STALL: 250); <=0: the pick
                                  by stall, helper_stall_min */
    int32_t xw_waves;          /* waves of the 65-256-member search; <=0: one per key, up to 4 per CU */
    int32_t p2_waves_per_cu;   /* 1: phase 2 at one wave per CU with the 128 KB LDS memo; else 4
                                  when WIDE keys share the grid. LEAN keys alone: 3 (32 KB memo,
                                  16 KB Bloom filter, round 5) or 6 (16 KB memo, 8 KB filter,
                                  round 7); <=0: the default, DESIGN.md section 5 */
    int32_t lean_waves;        /* at most this many phase-2 waves for LEAN keys; <=0: no cap */
    int32_t wide_waves;        /* at most this many waves for WIDE keys; <=0: no cap */
    int32_t handover_min;      /* phase 1: once its queue is empty, searches past this many
                                  inserts go to the heavy-key pass (checked every 1024
                                  inserts: 1024 hands over at 2047); 0: default (1024 when
                                  the deferred searches resume, round 5; else off), <0: never */
    int32_t p1_waves_per_cu;   /* phase-1 waves per CU (<= 26, the LDS limit); <=0: 26 */
    int32_t bfs_wgs;           /* ABI 7: phase-2 reachable-set BFS workgroups (one per CU); <=0: default */
    int32_t helper_stall_min;  /* round 7 (the former reserved slot): a late helper takes a key once its
                                  sequential search has made this many inserts without reaching a
                                  deeper layer (published every 1024 inserts), the smallest such
                                  stall first; <=0: 4096. Not used when helper_late_us > 0 or
                                  JH_LIN_HELPERS_NOW / JH_LIN_HELP_STALL is set: those keep the
                                  time-based pick */
    /* round 8, read only with JH_LIN_TAIL_FIELDS set in flags: */
    int32_t bfs_stall_min;     /* the default race's reachable-set BFS takes the key whose sequential
                                  search has the largest such stall, from this stall on, instead of
                                  keys in list order (scheduling only); <=0: 4096 */
    int32_t reserved;
} jh_lin_opts;

#define JH_DEFAULT_BUDGET (1 << 20)

typedef struct jh_key_verdict {
    int32_t valid;             /* JH_VALID / JH_UNKNOWN / JH_INVALID */
    int32_t cause;             /* JH_CAUSE_* */
    int64_t fail_entry;        /* invalid: history row of the ok completion of the
                                  first op no linearization can get past; else -1 */
    int64_t explored;          /* memo inserts (WGL cache size) for this key, the same
                                  on every run; -1 for a key in no tuple */
    /* invalid keys, from the search frontier (knossos' :previous-ok / :last-op;
     * knossos is not vendored, so these definitions are this library's and
     * PARITY-UNPINNED against knossos: oracle and device agree with each other):
     * last_op     = history row of the :ok completion of the last op the
     *               furthest configuration got past (RET[tmax-1]), -1 if none;
     * previous_ok = history row of the last client :ok in the key's
     *               subhistory before fail_entry, -1 if none.
     * Both -1 for keys that are not invalid. */
    int64_t previous_ok;
    int64_t last_op;
    /* ABI 4: the analysis that decided the key (knossos' :analyzer):
     * JH_ANALYZER_WGL (explored = WGL's cache size) or JH_ANALYZER_LINEAR
     * (explored = configurations the JIT-linearization analysis visited) */
    int32_t analyzer;
    int32_t reserved;
} jh_key_verdict;

#define JH_ANALYZER_WGL    0
#define JH_ANALYZER_LINEAR 1

typedef struct jh_summary {
    int64_t valid;             /* merge-valid over keys (checker.clj:33-47) */
    int64_t n_invalid;         /* == (count :failures) (independent.clj:289-295) */
    int64_t n_unknown;
    int64_t first_fail_entry;  /* min fail_entry over invalid keys, or -1 */
    int64_t n_keys;            /* keys checked (keys present in the history) */
    int64_t explored;          /* sum of memo inserts */
    int64_t memo_probes;       /* memo slots read by the phase-1 search kernel k_lin_dfs (roofline bytes) */
    double  device_ms;         /* device time of the check (HIP events) */
    double  dfs_ms;            /* of which the phase-1 search kernel k_lin_dfs (all keys, quick budget) */
    /* phase 2 (keys over the quick budget), for the roofline of its kernels */
    double  seq_ms;            /* the sequential search of the deferred keys (k_lin_seq / k_lin_wg) */
    double  bfs_ms;            /* the reachable-set BFS racing it (k_lin_bfs; 0 if not run) */
    int64_t n_deferred;        /* keys the phase-1 search handed on */
    int64_t deferred_entries;  /* history entries of those keys */
    int64_t seq_probes;        /* HBM memo probes of the phase-2 sequential search (LEAN keys) */
    /* ABI 4: per-phase accounting. Each search kernel has its own probe counter
     * and its own HIP events (on the stream it runs on), so each phase's
     * roofline is (56 B x its keys' entries + 16 B x its probes) / its time. */
    double  p3_ms;             /* phase 3, LEAN keys (restarted past phase2_budget) */
    double  wide_ms;           /* WIDE keys (window 41-64 or >= 256 states), phases 2 + 3 */
    double  xw_ms;             /* windows of 65-256 members (k_lin_xw) */
    int64_t p3_probes;
    int64_t wide_probes;
    int64_t xw_probes;
    int64_t helper_probes;     /* phase-2 late helper workgroups */
    int64_t n_deferred_wide;   /* WIDE keys among n_deferred */
    int64_t n_phase3;          /* LEAN keys restarted in phase 3 */
    int64_t n_phase3_wide;     /* WIDE keys restarted in phase 3 */
    int64_t n_xw;              /* keys searched by k_lin_xw */
    int64_t lean_entries;      /* entries of the deferred LEAN keys */
    int64_t wide_entries;      /* entries of the deferred WIDE keys */
    int64_t xw_entries;        /* entries of the k_lin_xw keys */
    int64_t waves[4];          /* launched waves: phase-2 LEAN, WIDE, phase-3 LEAN, xw */
    /* ABI 5 (round 4): the streaming heavy-key pass (JH_LIN_STREAM turns it
     * on). When streamed, seq_ms / bfs_ms / xw_ms are the engines' own spans
     * (first key taken to last wave end), p3_ms runs from the end of phase 2. */
    int64_t streamed;          /* 1: heavy keys started while phase 1 still ran */
    int64_t p3_entries;        /* entries of the LEAN keys restarted in phase 3 */
    double  p2_start_ms;       /* heavy-key pass start (streamed: its first key taken), ms after phase 1 began (-1: none) */
    double  p1_span_ms;        /* phase 1's first wave to its last wave's end (streamed) */
    /* ABI 6 (round 5): deferred searches phase 1 saved and the heavy-key pass
     * continued (JH_LIN_NO_RESUME: 0), and the bytes of their records */
    int64_t resumed;
    int64_t resume_bytes;
    /* ABI 7 (round 6): speculative dead-subtree enumerations by idle late
     * helpers (JH_LIN_NO_SPEC: 0): jobs run, of which dead, dead results the
     * searches merged and the nodes those merges added to their counts */
    int64_t spec_jobs;
    int64_t spec_dead;
    int64_t spec_merges;
    int64_t spec_nodes;
    /* round 6: keys a late helper took over from the sequential search with
     * its saved state (the takeover; JH_LIN_NO_TAKEOVER: 0) */
    int64_t takeovers;
    /* round 8, written only with JH_LIN_TAIL_FIELDS set in the call's flags:
     * keys the reachable-set BFS took by their stall (0 on the paths that keep
     * list order: JH_LIN_BFS_ONLY, JH_ALGO_LINEAR, JH_LIN_STREAM, a
     * configurations request, no sequential LEAN wave) */
    int64_t bfs_stall_picks;
} jh_summary;

typedef struct jh_ctx jh_ctx;

int  jh_version(void);
/* Opens a context on HIP device `device`. */
int  jh_open(int device, jh_ctx **out);
/* Opens one context over devices 0..n_gpus-1 (n_gpus <= 0: every visible
 * device; SURVEY 8(b) "jh_open(n_gpus)"). jh_check_cas_independent on it
 * splits the keys over the devices by the jh_key_costs estimate (heaviest
 * first to the least-loaded device), checks every part concurrently, one host
 * thread per device, and merges the verdicts and the summary on the host:
 * same result as one device, bit for bit. The other checkers run on device 0.
 * Host columns only (on_device = 0). jh_close closes every device. */
int  jh_open_multi(int n_gpus, jh_ctx **out);
/* The same over an explicit device list; a device may appear more than once
 * (several contexts share it, each with its own streams and workspace). */
int  jh_open_devices(const int32_t *devices, int n, jh_ctx **out);
int  jh_n_devices(const jh_ctx *ctx);
void jh_close(jh_ctx *ctx);

/* Per-key search-cost estimate used to split keys between devices: the key's
 * entries plus its window sum (for every client op, the :ok returns inside its
 * window; a crashed op's window runs to the end). Host columns; no device. */
int  jh_key_costs(const jh_history *h, int64_t *cost /*[n_keys]*/, char *err, size_t errlen);

/* (independent/checker (checker/linearizable {:model (model/cas-register init)})).
 * out[k] receives the verdict of key k for k in [0, h->n_keys); keys that
 * occur in no tuple get valid = JH_VALID, explored = -1 (they have no
 * :results entry, independent.clj:222-232). */
int jh_check_cas_independent(jh_ctx *ctx, const jh_history *h,
                             const jh_lin_opts *opts,
                             jh_key_verdict *out, jh_summary *sum,
                             char *err, size_t errlen);

/* The per-key row index of an independent history, from the device's stable
 * key partition: rows[key_off[k] .. key_off[k+1]) are key k's rows in history
 * order, and rows[key_off[n_keys] .. n) the rows in no tuple (nemesis ops).
 * Key k's subhistory (independent.clj:234-245) is the merge of its rows with
 * the un-keyed rows, so the shim writes every key's history.edn
 * (independent.clj:277-284) in one O(N) pass. Only the key column is read.
 * key_off: n_keys+1 entries; rows: n entries (host buffers). */
int jh_key_index(jh_ctx *ctx, const jh_history *h, int64_t *key_off, int64_t *rows,
                 char *err, size_t errlen);

/* Round 6: the columns of a host history exactly as the device sees them
 * after staging (the packed host-buffer path for >= 2 M rows, plain copies
 * below): process, type, f, key, value, value2 -- n int64 each, in that
 * order, into out (6 * n; the key block is left as is without a key column).
 * Checks nothing: a maintainer's (and the tests') view of the staging. */
int jh_stage_history(jh_ctx *ctx, const jh_history *h, int64_t *out, char *err, size_t errlen);

/* knossos' :configs (checker.clj:146-158 passes the analysis through and
 * keeps (take 10 ...) of them), from the JIT-linearization analysis
 * (:algorithm :linear; doc/tutorial/04-checker.md:126-138 prints one).
 *  - An invalid key: its frontier -- the configurations of the last layer
 *    its search reaches, the ways of linearizing the ops before the failing
 *    :ok op from which that op cannot be.
 *  - A valid key (ABI 6): its final configurations -- the configurations the
 *    analysis holds after the key's last :ok completion: every way the
 *    crashed ops may stand once every :ok op is linearized (the register
 *    value, and which crashed ops were linearized).
 * For each requested key, up to per_key (<= 16) configurations in a
 * canonical order: register value (nil first, then ascending), then the
 * linearized members as a bit mask in call order (a JH_MAX_WINDOW-bit
 * number). n_out[i] = the count for keys[i], or -1 (no search was needed, a
 * window over JH_MAX_WINDOW members, more than budget configurations
 * reachable, or a valid key the reachable-set engine cannot hold: WGL
 * decides those, and a WGL analysis carries no configurations).
 * Windows up to 32 members with < 4096 states come from the reachable-set
 * engine, wider invalid ones (round 4) from the 65-256-member search's table.
 * out[i * per_key + j] describes configuration j of keys[i]; its rows are
 * rows_out[rows_off .. rows_off + n_linearized + n_pending): the invocation
 * rows of the linearized ops, then of the pending ones (knossos' :pending),
 * each in call order -- for a frontier the members of the window, for final
 * configurations the crashed ops (their :info completion or none) the search
 * keeps; rows_cap >= n_keys_q * per_key * JH_MAX_WINDOW. Round 6: the reads
 * the search drops (crashed reads, :ok reads of nil -- they constrain
 * nothing) are listed too: each configuration is the one knossos holds in
 * which such a read is linearized exactly when its own completion forces it,
 * so a read invoked before the configuration's point and not completed there
 * is pending (call order, at most JH_MAX_WINDOW rows in all). last_row (ABI 6)
 * is the configuration's :last-op as knossos' analysis prints it: the row of
 * the key's last client :ok completion before the configurations' point (the
 * failing op's completion for a frontier, the end of the history for final
 * configurations; a read of nil completing later than a final
 * configuration's own last op is its :last-op), -1 if there is none.
 * knossos is not vendored: this order,
 * the cut and the layer are this library's definitions (parity unpinned; the
 * oracle restates them). */
typedef struct jh_lin_config {
    int64_t key;
    int64_t model_value;       /* the register's value in this configuration (JH_NIL: nil) */
    int32_t n_linearized;
    int32_t n_pending;
    int64_t rows_off;
    int64_t last_row;          /* ABI 6: the :ok completion that is this configuration's :last-op, or -1 */
} jh_lin_config;

int jh_lin_configs(jh_ctx *ctx, const jh_history *h, const jh_lin_opts *opts,
                   const int64_t *keys, int64_t n_keys_q, int32_t per_key,
                   jh_lin_config *out, int32_t *n_out, int64_t *rows_out, int64_t rows_cap,
                   char *err, size_t errlen);

/* (checker/linearizable {:model (model/cas-register init)}) on a history
 * whose values are not tuples (key column ignored). */
int jh_check_cas(jh_ctx *ctx, const jh_history *h, const jh_lin_opts *opts,
                 jh_key_verdict *out, char *err, size_t errlen);

/* Device-resident variant for benchmarking and for callers that keep the
 * encoded history in HBM: h->on_device must be 1; out_dev is a device array
 * of n_keys verdicts; sum is host. Runs on opts->stream, synchronises it. */
int jh_check_cas_independent_device(jh_ctx *ctx, const jh_history *h,
                                    const jh_lin_opts *opts,
                                    jh_key_verdict *out_dev, jh_summary *sum,
                                    char *err, size_t errlen);

/* (checker/counter). reads_out receives 3*n_reads int64 [lower value upper]
 * triples in history order (the :reads vector); at most reads_cap triples
 * are written, *n_reads is always the full count. *valid is JH_VALID /
 * JH_INVALID / JH_UNKNOWN (cause in *cause). *first_err_entry = history row
 * of the :ok read behind (first errors), or -1. */
int jh_check_counter(jh_ctx *ctx, const jh_history *h,
                     int64_t *reads_out, int64_t reads_cap,
                     int64_t *n_reads, int64_t *n_errors,
                     int64_t *first_err_entry, int32_t *valid, int32_t *cause,
                     char *err, size_t errlen);

typedef struct jh_set_result {
    int32_t valid;             /* JH_VALID / JH_INVALID / JH_UNKNOWN ("Set was never read") */
    int32_t cause;
    int64_t attempt_count, acknowledged_count, ok_count,
            lost_count, recovered_count, unexpected_count;
    int64_t first_fail_entry;  /* min row of an :ok :add whose element is lost;
                                  else the final read's row if unexpected; else -1 */
    int64_t final_read_entry;
    /* Run-length form of the four result sets (util.clj:536-575): run r of
     * set s is [runs[s][2r], runs[s][2r+1]] inclusive. Sets: 0 ok, 1 lost,
     * 2 unexpected, 3 recovered. Caller provides runs_cap pairs per set. */
    int64_t n_runs[4];
} jh_set_result;

int jh_check_set(jh_ctx *ctx, const jh_history *h, jh_set_result *res,
                 int64_t *runs_ok, int64_t *runs_lost, int64_t *runs_unexpected,
                 int64_t *runs_recovered, int64_t runs_cap,
                 char *err, size_t errlen);

/* (checker/set) with the four result sets as bitmaps instead of runs: bit i
 * of word w of a set is element *base + 32 w + i, for w < *n_words (at most
 * words_cap words are written per set; *n_words is always the full count).
 * Same counts, first_fail_entry and n_runs as jh_check_set. The D2H is 4
 * bytes per 32 elements of span, whatever the run structure; the shim
 * formats integer-interval-set-str (util.clj:536-575) from the bits. */
int jh_check_set_bitmaps(jh_ctx *ctx, const jh_history *h, jh_set_result *res,
                         uint32_t *ok, uint32_t *lost, uint32_t *unexpected, uint32_t *recovered,
                         int64_t words_cap, int64_t *base, int64_t *n_words,
                         char *err, size_t errlen);

/* Page-locked host memory for result buffers a caller keeps across calls
 * (jh_check_counter's triples, jh_check_set_bitmaps' bitmaps): their D2H then
 * runs at PCIe speed instead of through the runtime's pageable staging
 * copies. Not in the reference's interface (a JVM has no such thing): the
 * JNA shim allocates one per checker instance and reuses it. */
int jh_host_alloc(size_t bytes, void **out, char *err, size_t errlen);
int jh_host_free(void *p);

/* (checker/set-full {:linearizable? linearizable}), checker.clj:236-534.
 * Elements are the :value of every :invoke :add by an integer process; a
 * set :read's :value is its CSR range in aux (value = offset, value2 =
 * count; a nil :value reads as the empty set). `time` is the :time column
 * (nanoseconds), indexed by row like the others (host or device pointer
 * following h->on_device). Per element (set-full-element-results,
 * checker.clj:289-345): known = the first :ok :add or :ok :read containing
 * it, last-present / last-absent = the read INVOCATION of greatest index
 * whose :ok read did / did not contain it; all counted from the element's
 * last :invoke :add on (a re-invoke resets its state, checker.clj:483-487).
 * A read counts as the set of its elements: their order, repeated elements,
 * JH_NIL entries and values that no integer process ever added (below,
 * above or between the elements) do not matter.
 * The lost / never-read / stale element lists come back sorted; with fewer
 * than count entries of room (list_cap) each is the sorted list's prefix,
 * and the counts, quantiles and worst_stale are always those of the whole
 * result. worst_stale holds the (take 8 (reverse (sort-by :stable-latency
 * stale))) entries: among equal latencies the larger element first. */
#define JH_SF_QUANTILES 5          /* points [0 0.5 0.95 0.99 1], checker.clj:412 */
#define JH_SF_WORST 8

typedef struct jh_set_full_elem {
    int64_t element;
    int64_t stable_latency;        /* ms */
    int64_t known_entry;           /* row of the :known op: an :ok :add or an :ok :read */
    int64_t last_absent_entry;     /* row of the :last-absent read invocation, or -1 */
} jh_set_full_elem;

typedef struct jh_set_full_result {
    int32_t valid;                 /* JH_VALID / JH_INVALID / JH_UNKNOWN (no stable element) */
    int32_t cause;
    int64_t attempt_count, stable_count, lost_count, never_read_count, stale_count;
    int32_t has_stable_latencies, has_lost_latencies;
    int64_t stable_latencies[JH_SF_QUANTILES];   /* ms at the points above */
    int64_t lost_latencies[JH_SF_QUANTILES];
    int64_t n_worst;
    jh_set_full_elem worst_stale[JH_SF_WORST];
    int64_t n_reads;               /* :ok :reads by integer processes */
    int64_t read_elements;         /* sum of their element counts (aux entries scanned) */
    double  device_ms;             /* device time of the check (HIP events) */
} jh_set_full_result;

int jh_check_set_full(jh_ctx *ctx, const jh_history *h, const int64_t *time,
                      int32_t linearizable, jh_set_full_result *res,
                      int64_t *lost, int64_t *never_read, int64_t *stale, int64_t list_cap,
                      char *err, size_t errlen);

/* jh_check_set_full with options (zero-initialise; the call above is this
 * with only `linearizable` set). */
typedef struct jh_set_full_opts {
    int32_t linearizable;      /* {:linearizable? true}: stale elements make the result invalid */
    int32_t pad;
    int64_t read_batch;        /* :ok reads per bitmap batch, 0 = automatic (<= 2 GiB of bitmap,
                                  <= 65535 reads); tests use 1 and 3 to cross batch edges */
    int64_t reserved[4];
} jh_set_full_opts;
int jh_check_set_full_opts(jh_ctx *ctx, const jh_history *h, const int64_t *time,
                           const jh_set_full_opts *opts, jh_set_full_result *res,
                           int64_t *lost, int64_t *never_read, int64_t *stale, int64_t list_cap,
                           char *err, size_t errlen);

/* Queues. Values are the :value of :enqueue / :dequeue ops and the elements
 * of :ok :drain ops (integers, or ids the shim interned; JH_NIL = nil).
 * Multisets come back as (value, multiplicity) int64 pairs in ascending
 * order of value, with nil's pair (value JH_NIL) last, after every integer --
 * not first, where its INT64_MIN encoding would sort. At most pairs_cap
 * pairs are written per multiset, a prefix in that order (n_pairs is always
 * complete), so a multiset cut short loses nil's pair first. */
typedef struct jh_queue_result {
    int32_t valid;             /* JH_VALID / JH_INVALID */
    int32_t cause;
    int64_t attempt_count, acknowledged_count, ok_count, unexpected_count,
            duplicated_count, lost_count, recovered_count;
    int64_t n_pairs[4];        /* total-queue: lost, unexpected, duplicated, recovered;
                                  queue: [0] = the final queue */
    int64_t fail_entry;        /* queue: row of the first :ok :dequeue the model cannot
                                  supply ("can't dequeue v"), else -1 */
    int64_t fail_value;
    double  device_ms;
} jh_queue_result;

/* (checker/total-queue), checker.clj:570-628, after expand-queue-drain-ops
 * (:536-568; a crashed :drain is JH_EINVAL, as the reference throws). */
int jh_check_total_queue(jh_ctx *ctx, const jh_history *h, jh_queue_result *res,
                         int64_t *lost, int64_t *unexpected, int64_t *duplicated,
                         int64_t *recovered, int64_t pairs_cap, char *err, size_t errlen);

/* (checker/queue (model/unordered-queue)), checker.clj:160-180: the model
 * reduced over :invoke :enqueue and :ok :dequeue ops in history order.
 * final_queue receives the remaining multiset when valid. */
int jh_check_queue(jh_ctx *ctx, const jh_history *h, jh_queue_result *res,
                   int64_t *final_queue, int64_t pairs_cap, char *err, size_t errlen);

/* (checker/unique-ids), checker.clj:631-676 (ABI 8), over the whole history:
 * attempted = :invoke :generate rows; the acknowledged ids are the :value of
 * every :ok :generate row (JH_NIL, a nil :value, is an id like any other);
 * duplicated = the ids acknowledged more than once. :generate has no JH_F_*
 * code of its own: it is an interned f (>= 16) like every other name, and the
 * caller passes the code its encoder gave it in opts->f_generate.
 *
 * Ids are compared as signed int64, and JH_NIL (INT64_MIN) sorts first, which
 * is where `compare` puts nil. A caller whose ids are not integers interns
 * them; the counts and the duplicates need only equality, but range_lo /
 * range_hi (:range) are the smallest and largest CODE, so such a caller has
 * to intern in `compare` order if it wants :range.
 *
 * duplicated receives (id, count) int64 pairs: the min(duplicated_count,
 * dup_cap) entries that (->> dups (sort-by val) reverse (take dup_cap)) keeps
 * -- the largest counts, ties in count towards the larger id -- written in
 * ascending id (nil first). duplicated_count is always complete.
 * More than 2^31 - 1 acknowledged ids: JH_EUNSUPPORTED. */
typedef struct jh_unique_ids_opts {
    int64_t f_generate;   /* the f code the caller's encoder gave :generate (>= 0) */
    int32_t path;         /* 0 auto, 1 dense bitmap, 2 sorted (tests force both); dense over a
                             span above 2^35 ids (a 4 GiB bitmap) is JH_EINVAL */
    int32_t pad;
    int64_t reserved[4];
} jh_unique_ids_opts;

typedef struct jh_unique_ids_result {
    int32_t valid;            /* JH_VALID / JH_INVALID */
    int32_t path;             /* the path taken (1 / 2; 0: no acks). With only nil acks nothing
                                 is marked or sorted: the forced path, or 1 */
    int64_t attempted_count, acknowledged_count, duplicated_count;
    int64_t range_lo, range_hi;   /* JH_NIL = nil */
    int64_t nil_count;        /* acks whose id is nil */
    double  device_ms;
} jh_unique_ids_result;

int jh_check_unique_ids(jh_ctx *ctx, const jh_history *h, const jh_unique_ids_opts *opts,
                        jh_unique_ids_result *res, int64_t *duplicated, int64_t dup_cap,
                        char *err, size_t errlen);

/* (jepsen.tests.bank/checker checker-opts), tests/bank.clj:46-121 (additive to
 * ABI 8: new structs and one new symbol), over the :ok :read rows of any
 * process, their :value maps encoded as pair ranges (top of this file). Per
 * read, check-op's cond gives the FIRST matching error: unexpected-key (a code
 * outside [0, n_accounts)), nil-balance, wrong-total (the sum of the balances
 * is not total_amount), negative-value (only when negative_balances is 0).
 * A read without pairs sums to 0.
 *
 * errors[t]: per type in cond order, the number of such reads and the rows of
 * the first, the last and the worst one. worst_badness is err-badness as an
 * integer -- the number of unexpected keys, the number of nils, |total -
 * total_amount| (read it as UNSIGNED 64-bit: it can reach 2^64 - 1), -(sum of
 * the negative balances) -- and ties go to the smaller row, as util/max-by
 * keeps the earlier element. The reference orders wrong-totals by
 * (float (/ diff total-amount)); this result is in exact |diff| order, which
 * is the same order while worst_badness < 2^22 (above that distinct diffs can
 * share a float; a caller that wants the reference's tie there re-ranks the
 * triples). lowest_row / highest_row: the wrong-total with the smallest /
 * largest total, ties to the smaller row.
 *
 * reads_out (may be NULL) receives 3 * min(n_reads, reads_cap) int64:
 * [row, total, class] per :ok :read in history order -- total is the sum of
 * the read's non-nil balances (what bank/points plots), class 0 for no error
 * and 1..4 for the error types, + 8 when some prefix of that sum, in pair
 * order, overflows int64 (total is then JH_NIL). *n_reads is always complete.
 * The reference's (reduce + balances) throws on such a prefix for a read
 * that reaches the sum, so an overflowing read without an unexpected key or a
 * nil (class 8) makes the call valid = JH_UNKNOWN, cause = JH_CAUSE_OVERFLOW;
 * in a read of class 1 or 2 (9, 10) the overflow is not an error.
 *
 * JH_EINVAL: a pair range that leaves [0, n_aux / 2), a negative count, an
 * odd n_aux. JH_EUNSUPPORTED: a read of more than 2^31 - 1 pairs, more than
 * 2^31 - 2 reads. Balances that are not integers have no encoding: the shim
 * falls back to the JVM checker. */
typedef struct jh_bank_opts {
    int64_t total_amount;        /* (:total-amount test) */
    int64_t n_accounts;          /* distinct elements of (:accounts test) */
    int32_t negative_balances;   /* (:negative-balances? checker-opts) */
    int32_t pad;
    int64_t reserved[4];
} jh_bank_opts;

typedef struct jh_bank_err {        /* one per type, in cond order: 0 unexpected-key, 1 nil-balance,
                                       2 wrong-total, 3 negative-value */
    int64_t count, first_row, last_row, worst_row, worst_badness,
            lowest_row, highest_row; /* rows -1 when count == 0; lowest/highest: wrong-total only */
} jh_bank_err;

typedef struct jh_bank_result {
    int32_t valid, cause;
    int64_t read_count, error_count, first_error_row,
            entries;                 /* pairs scanned */
    jh_bank_err errors[4];
    double device_ms;
} jh_bank_result;

int jh_check_bank(jh_ctx *ctx, const jh_history *h, const jh_bank_opts *opts, jh_bank_result *res,
                  int64_t *reads_out, int64_t reads_cap, int64_t *n_reads, char *err, size_t errlen);

/* (jepsen.tests.long-fork/checker n), tests/long_fork.clj:158-324 (additive to
 * ABI 8: new structs, two cause codes and one new symbol), over txns encoded
 * as at the top of this file.
 *
 * reads = the :ok read-txn rows; early = those without a non-nil value, late =
 * those without a nil value (a read without pairs is both). The three counts
 * are always filled.
 *
 * Multiple writes: over the :invoke write-txn rows in history order, the first
 * row whose key an earlier such row wrote -> valid = JH_UNKNOWN, cause =
 * JH_CAUSE_MULTIPLE_WRITES, multiple_key / multiple_row; nothing below is
 * reached then.
 *
 * Otherwise an :ok read whose number of pairs is not n -> valid = JH_UNKNOWN,
 * cause = JH_CAUSE_ILLEGAL_HISTORY, illegal_kind = 1, illegal_row = the
 * smallest such row. Reads are grouped by key set; a group that holds two
 * distinct non-nil values for one key -> illegal_kind = 2, illegal_row = the
 * smallest row of a read holding a value for such a key. Otherwise two reads
 * of a group fork when each has a non-nil value where the other has nil:
 * fork_count pairs in fork_groups groups, valid = JH_INVALID when there is one.
 *
 * forks_out (may be NULL) receives min(fork_count, fork_cap) [row_a, row_b]
 * int64 pairs, row_a < row_b, ordered by group (ascending lowest key), then
 * row_a, then row_b: the first fork_cap pairs in that order. fork_count and
 * fork_groups are always complete.
 *
 * JH_EINVAL: a pair range that leaves [0, n_aux / 2), a negative count, an odd
 * n_aux, n < 1, a forced dense path whose tables would pass 2^28 entries.
 * JH_EUNSUPPORTED (the shim falls back): n > 64; an :ok read of exactly n pairs
 * whose keys are not the aligned range [l, l + n), l = k - (mod k n) (group-for,
 * the only shape the reference's generator emits), or that names one key
 * twice (the duplicate-key test applies only to reads of exactly n pairs);
 * more than 2^31 - 2 reads or :invoke writes. */
typedef struct jh_long_fork_opts {
    int64_t n;            /* the group size, 1..64 */
    int32_t path;         /* 0 auto, 1 dense tables (indexed by key - min / group - min group),
                             2 sparse (radix sorts); tests force both */
    int32_t pad;
    int64_t reserved[4];
} jh_long_fork_opts;

typedef struct jh_long_fork_result {
    int32_t valid, cause;          /* JH_VALID / JH_INVALID / JH_UNKNOWN (cause 10 or 11) */
    int32_t path;                  /* the path of the group slots (1 / 2; 0: the call ended before them) */
    int32_t illegal_kind;          /* 0 none, 1 group size, 2 distinct values */
    int64_t reads_count, early_count, late_count;
    int64_t multiple_key, multiple_row;   /* JH_NIL / -1 when there is none */
    int64_t illegal_row;           /* -1 when illegal_kind == 0 */
    int64_t fork_groups, fork_count;
    int64_t entries;               /* pairs of the :ok reads */
    double device_ms;
} jh_long_fork_result;

int jh_check_long_fork(jh_ctx *ctx, const jh_history *h, const jh_long_fork_opts *opts, jh_long_fork_result *res,
                       int64_t *forks_out, int64_t fork_cap, char *err, size_t errlen);

/* (independent/checker (jepsen.tests.causal-reverse/checker)),
 * tests/causal_reverse.clj:21-84 (additive to ABI 8: new structs and one new
 * symbol), batched over the keys of an independent history.
 *
 * Per key: the rows with f = JH_F_WRITE of type :invoke / :ok (any process)
 * build the precedence graph; every :ok JH_F_READ row is then judged, wherever
 * it stands. With last_inv[v] the row of the last :invoke of v and first_ok[v]
 * the row of the first :ok of v (invoked or not), a read that saw the set S has
 * M = max last_inv[w] over the invoked w in S (none: -1), expects
 * E = {v : first_ok[v] < M} and is an error when E - S is not empty:
 * expected_count = |E|, missing = E - S. S is the SET of the read's elements:
 * repeated elements change nothing. (The reference's behaviour on a vector
 * :value, clojure.set/difference testing indices, is not reproduced here; the
 * shim keeps such reads on the host unless asked otherwise.)
 *
 * key_valid (may be NULL) receives max(n_keys, 1) int32: JH_VALID / JH_INVALID.
 * errors_out (may be NULL) receives the first min(error_count, err_cap) failing
 * reads in row order as 5 int64 each: [row, key, expected_count, missing_count,
 * missing_offset] (key 0 for an un-keyed history; missing_offset = the sum of
 * the missing_count of the failing reads before it). missing_out (may be NULL)
 * receives the first min(missing_total, missing_cap) values of the failing
 * reads' missing sets, each ascending, concatenated in that same order. Every
 * result field is complete whatever the caps are.
 *
 * Two tiers. A key with at most JH_CR_LDS_VALUES distinct written values is
 * judged by one workgroup that keeps the key's value table in LDS; any other
 * key runs the same kernel with its table in device memory. The scratch of the
 * global tier is bounded by JH_CR_SCRATCH_MAX bytes: beyond it JH_ENOMEM.
 *
 * JH_EINVAL: an :ok read's range that leaves [0, n_aux), a negative count, a
 * key >= n_keys, path 1 forced with a key of more than JH_CR_LDS_VALUES
 * distinct values. JH_EUNSUPPORTED (the shim falls back): in a keyed history
 * an :invoke / :ok write row or an :ok read row without a key (it would belong
 * to every key); a write of JH_NIL; more than 2^31 - 2 reads or writes. */
#define JH_CR_LDS_VALUES 1024            /* distinct values per key of the on-chip tier */
#define JH_CR_SCRATCH_MAX (1LL << 32)    /* bytes of value tables and bitmaps of the global tier */

typedef struct jh_causal_reverse_opts {
    int32_t path;         /* 0 auto, 1 on-chip per-key tier, 2 global tier; tests force both */
    int32_t pad;
    int64_t reserved[4];
} jh_causal_reverse_opts;

typedef struct jh_causal_reverse_result {
    int32_t valid, cause;          /* JH_VALID / JH_INVALID; cause is JH_CAUSE_NONE */
    int32_t path;                  /* 1: every key on chip, 2: some key in the global tier, 0: no key was judged */
    int32_t pad;
    int64_t read_count;            /* :ok reads */
    int64_t error_count;           /* failing reads */
    int64_t invalid_keys;
    int64_t first_error_row;       /* -1 when there is none */
    int64_t missing_total;         /* sum of missing_count over the failing reads */
    int64_t entries;               /* elements of the :ok reads */
    double device_ms;
} jh_causal_reverse_result;

int jh_check_causal_reverse(jh_ctx *ctx, const jh_history *h, const jh_causal_reverse_opts *opts,
                            jh_causal_reverse_result *res, int32_t *key_valid, int64_t *errors_out, int64_t err_cap,
                            int64_t *missing_out, int64_t missing_cap, char *err, size_t errlen);

/* (independent/checker (checker/set)), independent.clj:247-298 over
 * checker.clj:182-233 (additive to ABI 8: new structs and one new symbol),
 * batched over the keys of an independent history: every key is judged as
 * jh_check_set_bitmaps judges its sub-history, in one call.
 *
 * The standard columns, with `key` as in jh_check_cas_independent and set reads
 * in aux through value / value2. Key k's sub-history is its own rows plus the
 * un-keyed rows (independent.clj:234-245); the call takes a keyed history only
 * when no un-keyed row can matter (below). Per key: attempts = the elements of
 * its :invoke :add rows, adds = those of its :ok :add rows (any process), the
 * final read R = the elements of its LAST :ok :read row (repeated elements
 * count once; an empty read is a read). No such row, or a nil :value there, is
 * JH_UNKNOWN / JH_CAUSE_NIL_VALUE ("Set was never read"). ok = R n attempts,
 * unexpected = R - attempts, lost = adds - R, recovered = ok - adds; valid iff
 * lost and unexpected are empty. Adds after the final read count.
 * first_fail_entry is the smallest row of an :ok :add of the key whose element
 * is lost, else the key's final-read row if anything is unexpected, else -1.
 *
 * keys_out (may be NULL) receives max(n_keys, 1) records. A key's four result
 * sets are bitmaps over [base, base + 32 n_words), base = the smallest element
 * of its add rows and its final read (0 when it has none), at words
 * [word_off, word_off + n_words) of ok / lost / unexpected / recovered: each
 * key owns a whole number of words, no two keys share one, and word_off is the
 * running sum of n_words in key order. A JH_UNKNOWN key and a key in no row
 * (rows == 0: it has no :results entry, independent.clj:222-232) have
 * n_words == 0. The four bitmaps (any may be NULL) receive the first
 * min(total_words, words_cap) words; the records and the result are complete
 * whatever the cap is. key == NULL or n_keys == 0 is one un-keyed history judged
 * as key 0: its record and bits equal jh_check_set_bitmaps' on the same columns.
 *
 * Two tiers. A key whose elements span at most JH_SI_LDS_SPAN is judged by one
 * workgroup that keeps its three bitmaps in LDS and writes each output word
 * once; any other key marks concatenated bitmaps in device memory. The three
 * working and four output bitmaps take 28 bytes per word: at most
 * 28 * JH_SI_WORDS_MAX = 7 GiB.
 *
 * JH_EUNSUPPORTED (the shim falls back to one jh_check_set_bitmaps per key): in
 * a keyed history an :invoke / :ok :add row or an :ok :read row without a key
 * (it would belong to every key); an :add element of JH_NIL; a key whose span
 * exceeds 2^34; total_words above JH_SI_WORDS_MAX; 2^31 rows or more.
 * JH_EINVAL: a key >= n_keys; a final read's range that leaves [0, n_aux) or
 * has a negative count; path 1 forced with a key wider than JH_SI_LDS_SPAN. */
#define JH_SI_LDS_SPAN  (1 << 17)        /* elements per key of the on-chip tier: three 16 KiB bitmaps in LDS */
#define JH_SI_WORDS_MAX (1LL << 28)      /* bitmap words over all keys: 7 GiB of device bitmaps, 4 GiB of output */

typedef struct jh_set_indep_opts {
    int32_t path;         /* 0 auto, 1 on-chip tier, 2 global tier; tests force both */
    int32_t pad;
    int64_t reserved[4];
} jh_set_indep_opts;

typedef struct jh_set_key {        /* one per key */
    int32_t valid, cause;          /* JH_VALID / JH_INVALID / JH_UNKNOWN (JH_CAUSE_NIL_VALUE) */
    int64_t rows;                  /* rows carrying this key; 0: the key is in no row, the shim gives it no result */
    int64_t attempt_count, acknowledged_count, ok_count, lost_count, recovered_count, unexpected_count;
    int64_t first_fail_entry, final_read_entry;   /* history rows, -1: none */
    int64_t base, word_off, n_words;              /* bit i of word word_off + w of a set is element base + 32 w + i */
} jh_set_key;

typedef struct jh_set_indep_result {
    int32_t valid, cause;          /* merge-valid over the keys that have rows */
    int32_t path, pad;             /* 1: every key on chip, 2: some key in the global tier, 0: no key judged */
    int64_t keys_valid, keys_invalid, keys_unknown;
    int64_t first_fail_entry;      /* min over keys, -1 */
    int64_t total_words;           /* sum of n_words: always the full count */
    int64_t entries;               /* rows + final-read elements consumed */
    double device_ms;
} jh_set_indep_result;

int jh_check_set_independent(jh_ctx *ctx, const jh_history *h, const jh_set_indep_opts *opts, jh_set_indep_result *res,
                             jh_set_key *keys_out, uint32_t *ok, uint32_t *lost, uint32_t *unexpected,
                             uint32_t *recovered, int64_t words_cap, char *err, size_t errlen);

/* (jepsen.tests.cycle/checker (cycle/combine ...)), tests/cycle.clj:202-216,
 * 911-934, and cycle/tarjan, cycle.clj:150-160 (additive to ABI 8: new structs,
 * one cause code and two symbols). Vertices are history rows (jh_scc: 0..n-1);
 * only completion rows ever carry edges. Rows with process == -1 (:nemesis) are
 * skipped by every builder: they are never an invoke, an :ok source or a txn,
 * which gives what the reference's removing them first gives (cycle.clj:919)
 * while the vertices stay history rows; other non-integer processes stay.
 *
 * Analyzers (opts->analyzers, a mask; at least one, or n_extra > 0):
 *  JH_CY_PROCESS   process-graph, cycle.clj:271-300: over the :ok rows, each row
 *                  links to the next :ok row of the same process.
 *  JH_CY_REALTIME  realtime-graph, cycle.clj:315-377, in closed form. Every
 *                  invoke is paired with the next completion of its process
 *                  (knossos' pair-index). For an :ok completion at row c let
 *                  R(c) be the smallest completion row over the ops invoked
 *                  after c whose completion is :ok (none: the end of the
 *                  history); the reference's `oks` buffer holds c exactly during
 *                  (c, R(c)), so c links to the completion, of any type, of
 *                  every invoke whose row lies in (c, R(c)).
 *                  A double invoke, or an :ok / :fail with no open invoke (an
 *                  :info without one is left unpaired, as pair-index leaves it)
 *                  -> valid = JH_UNKNOWN, cause JH_CAUSE_DOUBLE_INVOKE /
 *                  JH_CAUSE_ORPHAN, unknown_row = the smallest such row
 *                  (pair-index is not vendored: parity-unpinned). An invoke
 *                  without a completion that stands after the first :ok row ->
 *                  JH_UNKNOWN / JH_CAUSE_UNMATCHED_INVOKE, unknown_row = the
 *                  smallest such row (link's assert, cycle.clj:99-104, throws
 *                  there and check-safe makes it :unknown).
 *  JH_CY_WR        wr-graph, cycle.clj:703-779 with txn/src/jepsen/txn.clj:5-28,
 *                  over the :ok rows of any process, txns encoded as below. The
 *                  external read of k is the value of the txn's first micro-op
 *                  on k when that is not a write; the external write of k is the
 *                  value of its last write to k. For every externally read
 *                  (k, v), nil being a value like any other: no :ok writer of
 *                  k = v: no edge; one: an edge from the writer to every reader
 *                  (a txn reading its own (k, v) gives a self-loop, kept in
 *                  edges_out, and changing nothing); two or more: valid =
 *                  JH_UNKNOWN, cause JH_CAUSE_MULTIPLE_WRITES, unknown_row = the
 *                  smallest reader row with such a pair, unknown_key /
 *                  unknown_value = that row's first such pair in micro-op order,
 *                  unknown_rows = its two smallest writer rows. A (k, v) written
 *                  twice and never read externally is not an error.
 *  JH_CY_APPEND    appends-and-reads-graph, cycle.clj:381-699, txns encoded as
 *                  "Append txn encoding" below; not together with JH_CY_WR
 *                  (JH_EINVAL: the two read the txn columns differently and share
 *                  edge_count[2]). A position is (row, micro-op index); "first"
 *                  is the smallest position, the order of the reference's
 *                  reduce-mops. The checks run in this order and the first that
 *                  fires is the result:
 *                  unique appends (:invoke rows): the first [:append k v] whose
 *                  (k, v) an earlier :invoke micro-op appended (one of the same
 *                  txn included) -> JH_CAUSE_DUPLICATE_APPENDS.
 *                  no dups (rows of every type): the first read that holds an
 *                  element twice -> JH_CAUSE_DUPLICATE_ELEMENTS.
 *                  From here on only :ok and :info rows count. total order:
 *                  every read of k must be a prefix of L_k, k's longest read
 *                  (the first one of that length); nil and [] are both the
 *                  empty read. A key with a read that is not -> JH_CAUSE_NO_
 *                  TOTAL_ORDER. The writer of (k, v) is the last :ok / :info
 *                  row appending it. Edges, for every micro-op of every :ok /
 *                  :info row r, never from a row to itself:
 *                   wr  [:r k v], v not empty: writer(k, last v) -> r.
 *                   ww  [:append k v], v at position i > 0 of L_k:
 *                       writer(k, L_k[i-1]) -> r.
 *                   rw  the same append, i >= 0: q -> r for every read micro-op
 *                       of k of length i on an :ok / :info row q (once per such
 *                       micro-op: repeats are counted in edge_count[2]).
 *                  An append whose value stands in no read gives nothing. A wr
 *                  or ww writer that does not exist (the element came from a
 *                  :fail op, or from nothing) -> JH_CAUSE_NO_WRITER at the first
 *                  such micro-op (the reference's assert).
 *                  cause                 valid       unknown_row  unknown_rows[0]  unknown_key  unknown_value
 *                  13 DUPLICATE_APPENDS  JH_UNKNOWN  row          micro-op index   k            v
 *                  14 DUPLICATE_ELEMENTS JH_INVALID  row          micro-op index   k            the read's first element, in
 *                                                    list order, that equals an earlier one
 *                  15 NO_TOTAL_ORDER     JH_INVALID  the smallest row with a read of unknown_key that is no prefix of
 *                                                    its L_k; unknown_rows[0] = the number of bad keys, unknown_key =
 *                                                    the smallest bad key, unknown_value = JH_NIL
 *                  16 NO_WRITER          JH_UNKNOWN  row          micro-op index   k            the element nobody appended
 *                  unknown_rows[1] is -1 in all four. JH_INVALID with cause == 0
 *                  keeps meaning "SCCs".
 *  JH_CY_MONOTONIC monotonic-key-graph, cycle.clj:218-267, over the :ok rows of
 *                  any process, each row's :value a map {key value} encoded as
 *                  "Map reads encoding" below; not together with JH_CY_WR or
 *                  JH_CY_APPEND (JH_EINVAL: they read aux differently and share
 *                  edge_count[2]). For every key separately the rows that hold
 *                  it are grouped by their value of it and the groups ordered by
 *                  value as signed int64 (JH_NIL = INT64_MIN comes first, where
 *                  the reference's compare puts nil); every row of a group links
 *                  to every row of the key's next group. Values need not be
 *                  adjacent ({0, 1, 4}: 0 -> 1 and 1 -> 4); a key with a single
 *                  group gives nothing; a row is in one group per key, so there
 *                  are no self-loops; two rows linked through two keys count
 *                  twice. Rows of other types are not read.
 *  extra edges     opts->extra_src / extra_dst / n_extra: host int64 history rows,
 *                  for edges of analyzers the caller builds itself.
 * With several causes the first of: double invoke, orphan, unmatched invoke,
 * multiple writes, then 13, 14, 15, 16 is reported; edges and SCCs are not
 * computed then (scc_count = 0, labels_out all -1).
 *
 * Txn encoding (JH_CY_WR only): an :ok txn row has value = the index of its
 * first micro-op and value2 = its number of micro-ops; micro-op j is the triple
 * aux[3*(value+j) .. +3) = [f, k, v], f = JH_F_READ / JH_F_WRITE, k an int64 the
 * caller interned, v an int64 or JH_NIL; n_aux is a multiple of 3. A nil :value
 * is value = JH_NIL, value2 = 0. Rows of other types are not read.
 *
 * Append txn encoding (JH_CY_APPEND only): see "Append txns" at the top. With
 * it edge_count[2] = the number of link calls of the reference (repeats are
 * counted, pairs of a row with itself are not) and entries = micro-ops scanned
 * plus read elements scanned.
 *
 * Map reads encoding (JH_CY_MONOTONIC only; the pair layout of the bank and
 * long-fork reads): an :ok row has value = the index of its first pair and
 * value2 = its number of pairs; pair j is aux[2*(value+j)] (the key, an int64
 * the caller interned) and aux[2*(value+j)+1] (the value, an int64 or JH_NIL);
 * n_aux is even. A nil or empty map is value2 = 0, and value is then not looked
 * at. Ranges need not be contiguous or ordered in aux. With it edge_count[2] =
 * the number of link calls (the sum over keys and successive groups of
 * |A| * |B|) and entries = pairs scanned. The edge count is decided from 64-bit
 * counts before any edge buffer is sized.
 *
 * SCCs. An edge with dst < src is a back edge; every cycle holds one, and the
 * row intervals [dst, src] of the back edges, merged where they overlap, are
 * the regions: every SCC of more than one vertex lies inside one region. Each
 * region of two or more vertices is searched by one workgroup (worklist
 * trimming, then pivots with backward / forward reach), its per-vertex state in
 * LDS when it has at most JH_CY_LDS_VERTICES vertices and in device memory
 * otherwise. Work cap: a region of V vertices and E edges (both CSRs count E
 * once) may visit at most JH_CY_WORK_MULT * (V + E) edges; past that the call
 * returns JH_EUNSUPPORTED.
 *
 * Outputs (any may be NULL; every count is complete whatever the caps):
 *  labels_out[n]  for each row the smallest row of its SCC, -1 when in none.
 *  scc_off / scc_rows  the SCCs ordered by (size, smallest row): scc_off gets
 *                 min(scc_count, scc_cap) + 1 offsets and scc_rows the member
 *                 rows, ascending within an SCC, of those SCCs, as far as
 *                 rows_cap reaches (offsets past rows_cap are still exact).
 *  edges_out      min(total edges, edge_cap) [src_row, dst_row] pairs, order
 *                 unspecified, repeats across analyzers allowed.
 *
 * JH_EUNSUPPORTED (the shim falls back): a micro-op f other than read / write; a
 * txn of more than JH_CY_MAX_MOPS micro-ops; more than 2^31 - 2 vertices or
 * edges; a region past the work cap; with JH_CY_APPEND also an f other than
 * read / append, more than 2^31 - 2 records, and a read that needs the direct
 * duplicate check (it stands on an :invoke / :fail row, or is no prefix of its
 * L_k) and is longer than JH_CY_AP_DIRECT_READ elements. JH_EINVAL with
 * JH_CY_APPEND: a micro-op or element range leaving [0, n_aux), a negative
 * count, a key outside [0, n_keys), an element equal to JH_NIL, JH_CY_APPEND |
 * JH_CY_WR. With JH_CY_MONOTONIC: JH_EUNSUPPORTED for a row of more than
 * JH_CY_MAX_MOPS pairs and for more than 2^31 - 2 records; JH_EINVAL for a pair
 * range leaving [0, n_aux / 2), a negative count, an odd n_aux, a row that names
 * one key twice, JH_CY_MONOTONIC | JH_CY_WR and JH_CY_MONOTONIC | JH_CY_APPEND.
 * JH_EINVAL otherwise: a txn range leaving
 * [0, n_aux / 3), a negative count, n_aux % 3 != 0, an edge endpoint outside
 * [0, n), analyzers == 0 with no extra edges, a :type outside 0..3, path 1
 * forced with a region of more than JH_CY_LDS_VERTICES vertices. */
#define JH_CAUSE_UNMATCHED_INVOKE 12     /* cycle: an invoke without completion after the first :ok */
#define JH_CY_PROCESS  1
#define JH_CY_REALTIME 2
#define JH_CY_WR       4
#define JH_CY_APPEND   16                /* (8 is not an analyzer) */
#define JH_CY_MONOTONIC 32
#define JH_F_APPEND    7                 /* micro-op f of an append txn */
#define JH_CY_AP_DIRECT_READ 4096        /* elements of a read the direct duplicate check takes (a cap on a slow path) */
#define JH_CAUSE_DUPLICATE_APPENDS  13   /* cycle, JH_CY_APPEND: see the table above */
#define JH_CAUSE_DUPLICATE_ELEMENTS 14
#define JH_CAUSE_NO_TOTAL_ORDER     15
#define JH_CAUSE_NO_WRITER          16
#define JH_CY_LDS_VERTICES 2048          /* vertices of a region of the on-chip tier (16 B each) */
#define JH_CY_MAX_MOPS 64                /* micro-ops per txn; pairs per map (JH_CY_MONOTONIC) */
#define JH_CY_WORK_MULT 64               /* work cap of a region: this * (vertices + edges) edge visits */

typedef struct jh_cycle_opts {
    int32_t analyzers;    /* mask of JH_CY_*; ignored by jh_scc */
    int32_t path;         /* 0 auto, 1 on-chip tier, 2 global tier; tests force both */
    const int64_t *extra_src, *extra_dst;   /* host pointers; ignored by jh_scc */
    int64_t n_extra;
    int64_t reserved[4];
} jh_cycle_opts;

typedef struct jh_cycle_result {
    int32_t valid, cause;          /* JH_VALID iff scc_count == 0; JH_UNKNOWN with a cause above */
    int32_t path;                  /* 1: every region on chip, 2: some region in the global tier, 0: no region */
    int32_t pad;
    int64_t scc_count, scc_vertices;
    int64_t edge_count[4];         /* process, realtime, wr / append / monotonic, extra (jh_scc: all in [3]); self-loops and repeats counted */
    int64_t back_edges;
    int64_t regions, max_region, global_regions;   /* regions of >= 2 vertices; the largest one's vertices */
    int64_t unknown_row, unknown_key, unknown_value, unknown_rows[2];   /* -1 / JH_NIL / JH_NIL / -1 when unused */
    int64_t entries;               /* micro-ops scanned (JH_CY_APPEND: plus read elements scanned; JH_CY_MONOTONIC: pairs scanned) */
    double device_ms;
} jh_cycle_result;

int jh_scc(jh_ctx *ctx, int64_t n_vertices, const int64_t *src, const int64_t *dst, int64_t n_edges,
           const jh_cycle_opts *opts, jh_cycle_result *res, int64_t *labels_out, int64_t *scc_off, int64_t *scc_rows,
           int64_t scc_cap, int64_t rows_cap, char *err, size_t errlen);
int jh_check_cycle(jh_ctx *ctx, const jh_history *h, const jh_cycle_opts *opts, jh_cycle_result *res,
                   int64_t *labels_out, int64_t *scc_off, int64_t *scc_rows, int64_t scc_cap, int64_t rows_cap,
                   int64_t *edges_out, int64_t edge_cap, char *err, size_t errlen);

/* (independent/checker (jepsen.tests.causal/check (causal-register))),
 * tests/causal.clj:33-110 (additive to ABI 8: new structs, two f codes, one
 * sentinel and one symbol), batched over the keys of an independent history.
 *
 * Causal ops (jh_check_causal only): the standard columns, key = the interned
 * independent key. f = JH_F_READ, JH_F_WRITE, JH_F_READ_INIT or an interned id
 * >= 16; value = :value (JH_NIL = nil); value2 is not read (0). aux holds 2 n
 * words: aux[2 i] = row i's :position and aux[2 i + 1] = its :link, JH_NIL for
 * nil / absent, JH_CAUSAL_INIT for the keyword :init. Values, positions and
 * links are longs in (INT64_MIN + 1, INT64_MAX]; anything else has no encoding
 * (the shim then checks on the host). Only :ok rows are read.
 *
 * Per key, over its :ok rows in history order, the register (value, counter,
 * last-pos) starts at (0, 0, nil). In a valid prefix value = counter = the
 * number of :ok writes so far and last-pos = the :position of the key's
 * previous :ok row, so every row is judged on its own from w = the key's :ok
 * writes before it and p = the position of the key's previous :ok row (JH_NIL
 * for the first). A row is an EVENT of
 *   kind 1  link != JH_CAUSAL_INIT and link != p (nil = nil passes);
 *   kind 2  a write of value != w + 1 (nil included);
 *   kind 3  a read-init with w = 0 and value != 0 (nil included), or with a
 *           value that is neither nil nor w;
 *   kind 4  a read of a value that is neither nil nor w;
 *   kind 5  any other f (the reference's condp throws; the link check comes
 *           first, so a bad link makes it kind 1).
 * The key's first event decides: kinds 1-4 JH_INVALID, kind 5 JH_UNKNOWN, no
 * event JH_VALID with the final model (counter, counter, last_pos).
 *
 * keys_out (may be NULL) receives max(n_keys, 1) jh_causal_key. An un-keyed
 * history (key == NULL or n_keys == 0) is one key 0. A key without :ok rows is
 * valid with counter 0 and last_pos JH_NIL.
 *
 * JH_EINVAL: n_aux != 2 n, an :ok row's key >= n_keys. JH_EUNSUPPORTED (the
 * shim falls back): in a keyed history an :ok row of a process >= 0 without a
 * key (it would belong to every key; such a row of a process < 0 is skipped,
 * the shim does not send one); more than 2^31 - 2 :ok rows, 2^32 - 1 rows or
 * 2^30 keys. */
#define JH_F_INSERT    8                 /* adya g2: :insert */
#define JH_F_READ_INIT 9                 /* causal: :read-init */
#define JH_CAUSAL_INIT (INT64_MIN + 1)   /* a :link of :init */

typedef struct jh_causal_opts {
    int64_t reserved[4];
} jh_causal_opts;

typedef struct jh_causal_key {   /* one per key */
    int32_t valid;               /* JH_VALID / JH_INVALID / JH_UNKNOWN */
    int32_t kind;                /* 0 none, 1 link, 2 write, 3 read-init, 4 read, 5 unknown f */
    int64_t row;                 /* the event row; -1 when valid */
    int64_t counter;             /* :ok writes of the key before `row`; all of them when valid */
    int64_t last_pos;            /* position of the key's previous :ok row (valid: of its last); JH_NIL: nil / none */
} jh_causal_key;

typedef struct jh_causal_result {
    int32_t valid, cause;          /* invalid outranks unknown outranks valid; JH_CAUSE_BAD_F when some key is unknown */
    int64_t ok_count;              /* :ok rows judged */
    int64_t invalid_keys, unknown_keys;
    int64_t first_event_row;       /* the smallest event row of any key; -1 when there is none */
    double device_ms;
} jh_causal_result;

int jh_check_causal(jh_ctx *ctx, const jh_history *h, const jh_causal_opts *opts, jh_causal_result *res,
                    jh_causal_key *keys_out, char *err, size_t errlen);

/* (jepsen.tests.adya/g2-checker), tests/adya.clj:62-88 (additive to ABI 8: new
 * structs and one symbol): at most one :insert completes :ok for any key.
 *
 * G2 ops (jh_check_g2 only): the standard columns. f = JH_F_INSERT for :insert,
 * anything else otherwise; key = the interned (key (:value op)). Only type, f
 * and key are read. Every insert row, of any type and any process, makes its
 * key present; an :ok insert adds one to the key's count.
 *   key_count      keys present
 *   illegal_count  keys with a count > 1
 *   legal_count    keys with a count > 0, less illegal_count
 * illegal_out (may be NULL) receives the first min(illegal_count, illegal_cap)
 * pairs [key id, count] in ascending key id. first_illegal_row = the smallest
 * row that is an :ok insert of an illegal key and not that key's first :ok
 * insert, or -1. Every result field is exact whatever the cap is.
 *
 * JH_EINVAL: an insert row's key >= n_keys. JH_EUNSUPPORTED: an insert row
 * without a key (the reference throws); more than 2^31 - 2 rows. */
typedef struct jh_g2_opts {
    int64_t reserved[4];
} jh_g2_opts;

typedef struct jh_g2_result {
    int32_t valid, cause;          /* JH_VALID / JH_INVALID; cause is JH_CAUSE_NONE */
    int64_t key_count, legal_count, illegal_count;
    int64_t insert_rows;
    int64_t first_illegal_row;     /* -1 when there is none */
    double device_ms;
} jh_g2_result;

int jh_check_g2(jh_ctx *ctx, const jh_history *h, const jh_g2_opts *opts, jh_g2_result *res,
                int64_t *illegal_out, int64_t illegal_cap, char *err, size_t errlen);

/* (checker/latency-graph), (checker/rate-graph) and (checker/perf),
 * checker.clj:736-768 over checker/perf.clj and util.clj:606-640 (additive to
 * ABI 8: new structs and one symbol). The product of these checkers is the plot,
 * not :valid?; jh_perf is the reduction over the history that the three plots
 * need, all of it in integers. The caller turns the outputs into the series of
 * perf/plot!.
 *
 * Only process, type and f of the history are read, and `time`, the :time
 * column (nanoseconds, indexed by row, host or device like the history).
 *
 * Pairing (util/history->latencies): rows are put in per-process order, a
 * stable sort by process (every value a key of its own, negative ones included).
 * A non-invoke row pairs with the row just before it in that order exactly when
 * that row is an invoke; every other row is unpaired. The latency of a pair is
 * time[completion] - time[invoke], signed.
 *   pair     [n] the partner row of each row, or -1
 *   t_max    max(0, every row's time)
 * Raw points (perf/point-graph!): the paired invokes, stably partitioned by
 * (f ascending; completion type in the order :ok :info :fail; row ascending).
 *   pt_row   [n_paired] the invoke rows in that order
 *   series   [n_series][3] = f, completion type, count: the non-empty series
 * Quantile groups (perf/quantiles-graph!), only when n_unpaired_invokes == 0
 * (has_quantiles; the reference throws otherwise): every invoke by (f, bucket of
 * the invoke's time with dt_quantiles).
 *   groups   [n_groups][7] = f, bucket, count, and the latency (ns) at 0.5, 0.95,
 *            0.99 and 1: sorted[min(count - 1, (int64)floor((double)count * q))];
 *            in (f, bucket) order
 * Rate cells (perf/rate-graph!): the non-invoke rows with process >= 0.
 *   cells    [n_cells][4] = f, type, bucket with dt_rate, count; in (f, type
 *            code, bucket) order
 * The bucket of a time t is (int64)(((double)t / 1e9) / (double)dt): the
 * reference's two double divisions, then truncation.
 *
 * Any output pointer may be NULL. A list with fewer than its count entries of
 * room (its cap) receives the prefix; the counts are those of the whole result.
 * n = 0 is JH_OK with every count 0. The pairing counts are filled when
 * JH_PERF_PAIR, _POINTS or _QUANTILES is wanted; t_max always.
 *
 * JH_EUNSUPPORTED (the shim falls back): a JH_NIL or negative time; an f code
 * outside [0, f_count); f_count above 2^20; more than 2^31 - 2 rows.
 * JH_EINVAL: f_count < 1, a negative dt, a want bit that is not defined. */
#define JH_PERF_PAIR      1
#define JH_PERF_POINTS    2
#define JH_PERF_QUANTILES 4
#define JH_PERF_RATE      8
#define JH_PERF_ALL       15

typedef struct jh_perf_opts {
    int64_t f_count;             /* f codes lie in [0, f_count): 16 + the interned f */
    int64_t dt_quantiles;        /* seconds; 0 = 30 */
    int64_t dt_rate;             /* seconds; 0 = 10 */
    int32_t want, pad;           /* JH_PERF_* bits; 0 = JH_PERF_ALL */
    int64_t reserved[4];
} jh_perf_opts;

typedef struct jh_perf_result {
    int64_t n_invokes, n_paired, n_unpaired_invokes;
    int64_t first_unpaired_invoke;   /* a row, or -1 */
    int64_t t_max;
    int64_t n_series, n_groups, n_cells;
    int32_t has_quantiles, pad;      /* 1: the groups were produced */
    double device_ms;
} jh_perf_result;

int jh_perf(jh_ctx *ctx, const jh_history *h, const int64_t *time, const jh_perf_opts *opts, jh_perf_result *res,
            int64_t *pair, int64_t pair_cap, int64_t *pt_row, int64_t pt_cap, int64_t *series, int64_t series_cap,
            int64_t *groups, int64_t group_cap, int64_t *cells, int64_t cell_cap, char *err, size_t errlen);

/* (independent/checker (checker/linearizable {:model (multi-register init)})),
 * yugabyte/src/yugabyte/multi_key_acid.clj:20-42,112-127 (additive to ABI 8).
 * The model's state is a map register -> value; an op is a txn [[f k v] ...] of
 * reads and writes applied left to right; a read of nil is always legal.
 *
 * Multi-register txns (this entry point only): EVERY client row (:invoke, :ok,
 * :fail, :info) carries its txn in the "Cycle txns" layout: value = the index
 * of its first micro-op, value2 = its number of micro-ops, micro-op j the triple
 * aux[3*(value+j) .. +3) = [f, reg, val] with f = JH_F_READ / JH_F_WRITE; a nil
 * :value is value = JH_NIL (value2 not read). The caller interns registers to
 * 0 .. n_regs-1 (registers that stand only in the initial map count) and values
 * to dense ids 1 .. V; nil is JH_NIL or id 0. The state is one 32-bit word,
 * `bits` = ceil(log2(V + 1)) bits per register, register r at bit r * bits.
 * `key` as in jh_check_cas_independent; key == NULL or n_keys == 0 is one
 * un-keyed history (out has one entry).
 *
 * A txn reduces, whatever the state, to (never, rmask, rval, wmask, wval):
 *   step(s) = (never or (s & rmask) != rval) ? inconsistent : (s & ~wmask) | wval
 * (a nil read adds nothing; a non-nil read of a register the txn wrote or read
 * before is compared with that value, a mismatch sets never; a write, nil
 * included, sets wmask / wval, a later one overwrites).
 *
 * Per key: invoke and completion are paired per process (an :info row never
 * completes: the op is crashed); a double invoke / an orphan completion make
 * the key JH_UNKNOWN with JH_CAUSE_DOUBLE_INVOKE / JH_CAUSE_ORPHAN (the
 * smallest such row decides). An :ok op's txn is its completion's when that
 * row's value is not JH_NIL, else its invocation's; a crashed op keeps its
 * invocation's (PARITY-UNPINNED: knossos is not vendored). Dropped: rows of a
 * process < 0, failed ops, crashed ops without a write, :ok ops whose normal
 * form is the identity. The rest is searched by WGL exactly as the cas path
 * (same order, explored = the cache size, budget as jh_lin_opts.budget):
 *   valid / cause / fail_entry / explored as in jh_key_verdict; previous_ok =
 *   last_op = -1; analyzer = JH_ANALYZER_WGL. A key in no client row: JH_VALID,
 *   explored = -1. More than JH_MR_MAX_WINDOW searched ops open at an :ok
 *   return besides the returning one, or 2^20 - 1 or more searched :ok ops:
 *   JH_UNKNOWN / JH_CAUSE_WINDOW for that key alone, explored = 0.
 * sum (may be NULL) receives valid, n_invalid, n_unknown, first_fail_entry,
 * n_keys, explored, device_ms and waves[0] (the search waves launched); every
 * other field of ABI 8's layout is 0.
 *
 * JH_EUNSUPPORTED (the shim falls back to its host checker): n_regs * bits > 32;
 * a txn of more than JH_CY_MAX_MOPS micro-ops; in a keyed history a client row
 * without a key; 2^31 rows or more. JH_EINVAL: a triple range leaving aux or a
 * negative count; reg outside [0, n_regs); a value id outside [0, 2^bits) (and
 * not JH_NIL), in a txn or in init; an f other than read / write on a client
 * row that is not :fail; a key >= n_keys. */
#define JH_MR_MAX_WINDOW 64
#define JH_MR_GEN_JUMP   1          /* flags, test hook: every memo table is cleared and its generations start just below their wrap */

typedef struct jh_multi_register_opts {
    int64_t budget;            /* max memo inserts per key before :unknown; <= 0: JH_DEFAULT_BUDGET */
    int32_t n_regs, bits;
    const int64_t *init;       /* n_regs value ids (host; 0 or JH_NIL = nil); NULL: every register nil */
    int32_t waves;             /* search waves; <= 0: min(keys, 4 per CU, what a quarter of free memory holds) */
    int32_t flags;             /* JH_MR_*; 0 in production */
    int64_t reserved[4];
} jh_multi_register_opts;

int jh_check_multi_register(jh_ctx *ctx, const jh_history *h, const jh_multi_register_opts *opts,
                            jh_key_verdict *out /*[max(n_keys, 1)]*/, jh_summary *sum, char *err, size_t errlen);

#ifdef __cplusplus
}
#endif
#endif /* JH_H */
