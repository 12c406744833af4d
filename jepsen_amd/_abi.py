"""ctypes mirror of include/jh.h (the C ABI of libjh.so).

Kept in one place so the product binding (`_native.py`), the test oracle
wrapper (`oracle/oracle.py`) and the generator wrapper (`synth.py`) agree on
every struct layout.
"""
import ctypes as C

JH_ABI_VERSION = 8

JH_OK, JH_EINVAL, JH_EUNSUPPORTED, JH_EDEVICE, JH_ENOMEM = 0, 1, 2, 3, 4
TYPE_INVOKE, TYPE_OK, TYPE_FAIL, TYPE_INFO = 0, 1, 2, 3
F_READ, F_WRITE, F_CAS, F_ADD = 0, 1, 2, 3
F_ENQUEUE, F_DEQUEUE, F_DRAIN = 4, 5, 6
F_FIRST_INTERNED = 16
NIL = -(1 << 63)

VALID, UNKNOWN, INVALID = 0, 1, 2

CAUSES = {
    0: None,
    1: "budget",
    2: "window",
    3: "double-invoke",
    4: "orphan-completion",
    5: "unsupported-f",
    6: "nil-value",
    7: "overflow",
    8: "states",
    9: "deferred",
    10: "multiple-writes",
    11: "illegal-history",
}

MAX_WINDOW = 256
DEFAULT_BUDGET = 1 << 20

_p64 = C.POINTER(C.c_int64)


class JhHistory(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("process", _p64),
        ("type", _p64),
        ("f", _p64),
        ("key", _p64),
        ("value", _p64),
        ("value2", _p64),
        ("n_keys", C.c_int64),
        ("aux", _p64),
        ("n_aux", C.c_int64),
        ("on_device", C.c_int32),
        ("reserved", C.c_int32),
    ]


ALGO_COMPETITION, ALGO_WGL, ALGO_LINEAR = 0, 1, 2
ALGORITHMS = {"competition": ALGO_COMPETITION, "wgl": ALGO_WGL, "linear": ALGO_LINEAR}
# jh_lin_opts.flags (test hooks)
LIN_BFS_ONLY, LIN_GEN_JUMP, LIN_INTERN_PER_KEY, LIN_NO_HELPERS, LIN_HELPERS_NOW = 1, 2, 4, 8, 16
LIN_PHASE1_ONLY, LIN_SKIP_PHASE1 = 32, 64
LIN_NO_HANDOVER = 128
LIN_STREAM = 256
LIN_NO_RESUME = 512           # round 5: restart deferred keys instead of continuing them
LIN_EXACT_COUNT = 1024        # round 5: WGL's exact count for every key (the parity tests)
EXPLORED_UNCOUNTED = -3       # a valid key settled without the count pass
LIN_NO_SPEC = 2048            # round 6: no speculative dead-subtree enumerations by idle helpers
LIN_SPEC_FIRST = 4096         # round 6: helpers serve posted spec jobs before taking keys
LIN_HELP_STALL = 8192         # round 6: helpers pick the keys stuck longest (no deeper layer)
LIN_NO_TAKEOVER = 16384       # round 6: forces the takeover off
LIN_TAKEOVER = 32768          # round 6 (opt-in): a helper continues the sequential search's saved state
LIN_TAIL_FIELDS = 65536       # round 8: these structs carry bfs_stall_min / bfs_stall_picks (always set by _native)
CAUSE_DEFERRED = 9


class JhLinOpts(C.Structure):
    _fields_ = [("init_value", C.c_int64), ("budget", C.c_int64), ("stream", C.c_int64),
                ("algorithm", C.c_int32), ("flags", C.c_int32),
                ("quick_budget", C.c_int64), ("phase2_budget", C.c_int64),
                ("helpers", C.c_int32), ("helper_late_us", C.c_int32),
                ("xw_waves", C.c_int32), ("p2_waves_per_cu", C.c_int32),
                ("lean_waves", C.c_int32), ("wide_waves", C.c_int32),
                ("handover_min", C.c_int32), ("p1_waves_per_cu", C.c_int32),
                ("bfs_wgs", C.c_int32), ("helper_stall_min", C.c_int32),       # ABI 7 (round 7: its reserved slot)
                ("bfs_stall_min", C.c_int32), ("reserved", C.c_int32)]         # round 8: read with LIN_TAIL_FIELDS


# every field of jh_key_verdict: the parity tests compare all of them
VERDICT_FIELDS = ("valid", "cause", "fail_entry", "explored", "previous_ok", "last_op", "analyzer")
ANALYZER_WGL, ANALYZER_LINEAR = 0, 1
ANALYZERS = {ANALYZER_WGL: "wgl", ANALYZER_LINEAR: "linear"}


class JhKeyVerdict(C.Structure):
    _fields_ = [("valid", C.c_int32), ("cause", C.c_int32),
                ("fail_entry", C.c_int64), ("explored", C.c_int64),
                ("previous_ok", C.c_int64), ("last_op", C.c_int64),
                ("analyzer", C.c_int32), ("reserved", C.c_int32)]


class JhSummary(C.Structure):
    _fields_ = [("valid", C.c_int64), ("n_invalid", C.c_int64), ("n_unknown", C.c_int64),
                ("first_fail_entry", C.c_int64), ("n_keys", C.c_int64),
                ("explored", C.c_int64), ("memo_probes", C.c_int64),
                ("device_ms", C.c_double), ("dfs_ms", C.c_double),
                ("seq_ms", C.c_double), ("bfs_ms", C.c_double), ("n_deferred", C.c_int64),
                ("deferred_entries", C.c_int64), ("seq_probes", C.c_int64),
                # ABI 4: per-phase accounting
                ("p3_ms", C.c_double), ("wide_ms", C.c_double), ("xw_ms", C.c_double),
                ("p3_probes", C.c_int64), ("wide_probes", C.c_int64), ("xw_probes", C.c_int64),
                ("helper_probes", C.c_int64), ("n_deferred_wide", C.c_int64), ("n_phase3", C.c_int64),
                ("n_phase3_wide", C.c_int64), ("n_xw", C.c_int64), ("lean_entries", C.c_int64),
                ("wide_entries", C.c_int64), ("xw_entries", C.c_int64), ("waves", C.c_int64 * 4),
                # ABI 5: the streaming heavy-key pass
                ("streamed", C.c_int64), ("p3_entries", C.c_int64), ("p2_start_ms", C.c_double),
                ("p1_span_ms", C.c_double),
                # ABI 6: deferred searches resumed by the heavy-key pass
                ("resumed", C.c_int64), ("resume_bytes", C.c_int64),
                # ABI 7: speculative dead-subtree enumerations (round 6)
                ("spec_jobs", C.c_int64), ("spec_dead", C.c_int64), ("spec_merges", C.c_int64),
                ("spec_nodes", C.c_int64), ("takeovers", C.c_int64),
                ("bfs_stall_picks", C.c_int64)]                               # round 8: written with LIN_TAIL_FIELDS


class JhLinConfig(C.Structure):
    _fields_ = [("key", C.c_int64), ("model_value", C.c_int64), ("n_linearized", C.c_int32),
                ("n_pending", C.c_int32), ("rows_off", C.c_int64),
                ("last_row", C.c_int64)]            # ABI 6: the :ok completion that is :last-op


CONFIGS_PER_KEY = 10          # checker.clj:146-158: (take 10 ...) of :configs and :final-paths


class JhSetResult(C.Structure):
    _fields_ = [("valid", C.c_int32), ("cause", C.c_int32),
                ("attempt_count", C.c_int64), ("acknowledged_count", C.c_int64),
                ("ok_count", C.c_int64), ("lost_count", C.c_int64),
                ("recovered_count", C.c_int64), ("unexpected_count", C.c_int64),
                ("first_fail_entry", C.c_int64), ("final_read_entry", C.c_int64),
                ("n_runs", C.c_int64 * 4)]


SF_QUANTILES = 5
SF_WORST = 8
SF_POINTS = (0, 0.5, 0.95, 0.99, 1)       # checker.clj:412


class JhSetFullElem(C.Structure):
    _fields_ = [("element", C.c_int64), ("stable_latency", C.c_int64),
                ("known_entry", C.c_int64), ("last_absent_entry", C.c_int64)]


class JhSetFullResult(C.Structure):
    _fields_ = [("valid", C.c_int32), ("cause", C.c_int32),
                ("attempt_count", C.c_int64), ("stable_count", C.c_int64),
                ("lost_count", C.c_int64), ("never_read_count", C.c_int64),
                ("stale_count", C.c_int64),
                ("has_stable_latencies", C.c_int32), ("has_lost_latencies", C.c_int32),
                ("stable_latencies", C.c_int64 * SF_QUANTILES),
                ("lost_latencies", C.c_int64 * SF_QUANTILES),
                ("n_worst", C.c_int64), ("worst_stale", JhSetFullElem * SF_WORST),
                ("n_reads", C.c_int64), ("read_elements", C.c_int64),
                ("device_ms", C.c_double)]


class JhSetFullOpts(C.Structure):
    _fields_ = [("linearizable", C.c_int32), ("pad", C.c_int32), ("read_batch", C.c_int64),
                ("reserved", C.c_int64 * 4)]


class JhIngestOpts(C.Structure):
    """include/jh_io.h jh_ingest_opts."""
    _fields_ = [("threads", C.c_int32), ("debug", C.c_int32), ("min_chunk", C.c_int64),
                ("reserved", C.c_int64 * 4)]


class JhQueueResult(C.Structure):
    _fields_ = [("valid", C.c_int32), ("cause", C.c_int32),
                ("attempt_count", C.c_int64), ("acknowledged_count", C.c_int64),
                ("ok_count", C.c_int64), ("unexpected_count", C.c_int64),
                ("duplicated_count", C.c_int64), ("lost_count", C.c_int64),
                ("recovered_count", C.c_int64), ("n_pairs", C.c_int64 * 4),
                ("fail_entry", C.c_int64), ("fail_value", C.c_int64), ("device_ms", C.c_double)]


UID_PATH_AUTO, UID_PATH_DENSE, UID_PATH_SORTED = 0, 1, 2
UID_DUP_CAP = 48              # checker.clj:674: (take 48) of :duplicated


class JhUniqueIdsOpts(C.Structure):
    _fields_ = [("f_generate", C.c_int64), ("path", C.c_int32), ("pad", C.c_int32),
                ("reserved", C.c_int64 * 4)]


class JhUniqueIdsResult(C.Structure):
    _fields_ = [("valid", C.c_int32), ("path", C.c_int32),
                ("attempted_count", C.c_int64), ("acknowledged_count", C.c_int64),
                ("duplicated_count", C.c_int64), ("range_lo", C.c_int64), ("range_hi", C.c_int64),
                ("nil_count", C.c_int64), ("device_ms", C.c_double)]


BANK_TYPES = ("unexpected-key", "nil-balance", "wrong-total", "negative-value")   # check-op's cond order
BANK_OVERFLOW = 8             # reads_out class bit: a prefix of the read's sum overflows
BANK_FLOAT_EXACT = 1 << 22    # below this |diff| the float badness orders like the integer


class JhBankOpts(C.Structure):
    _fields_ = [("total_amount", C.c_int64), ("n_accounts", C.c_int64),
                ("negative_balances", C.c_int32), ("pad", C.c_int32), ("reserved", C.c_int64 * 4)]


class JhBankErr(C.Structure):
    _fields_ = [("count", C.c_int64), ("first_row", C.c_int64), ("last_row", C.c_int64),
                ("worst_row", C.c_int64), ("worst_badness", C.c_int64),
                ("lowest_row", C.c_int64), ("highest_row", C.c_int64)]


class JhBankResult(C.Structure):
    _fields_ = [("valid", C.c_int32), ("cause", C.c_int32),
                ("read_count", C.c_int64), ("error_count", C.c_int64), ("first_error_row", C.c_int64),
                ("entries", C.c_int64), ("errors", JhBankErr * 4), ("device_ms", C.c_double)]


LF_PATH_AUTO, LF_PATH_DENSE, LF_PATH_SPARSE = 0, 1, 2
LF_TILE = 4096                # rows per tile of jh_longfork.hip's scan (the tests straddle its edges)
LF_MAX_N = 64                 # keys per group the device handles (one mask word)
LF_DENSE_MAX = 1 << 28        # table entries above which a forced dense path is JH_EINVAL
CAUSE_MULTIPLE_WRITES, CAUSE_ILLEGAL_HISTORY = 10, 11
LF_ILLEGAL_GROUP_SIZE, LF_ILLEGAL_DISTINCT_VALUES = 1, 2


class JhLongForkOpts(C.Structure):
    _fields_ = [("n", C.c_int64), ("path", C.c_int32), ("pad", C.c_int32), ("reserved", C.c_int64 * 4)]


class JhLongForkResult(C.Structure):
    _fields_ = [("valid", C.c_int32), ("cause", C.c_int32), ("path", C.c_int32), ("illegal_kind", C.c_int32),
                ("reads_count", C.c_int64), ("early_count", C.c_int64), ("late_count", C.c_int64),
                ("multiple_key", C.c_int64), ("multiple_row", C.c_int64), ("illegal_row", C.c_int64),
                ("fork_groups", C.c_int64), ("fork_count", C.c_int64), ("entries", C.c_int64),
                ("device_ms", C.c_double)]


CR_PATH_AUTO, CR_PATH_LDS, CR_PATH_GLOBAL = 0, 1, 2
CR_LDS_VALUES = 1024          # JH_CR_LDS_VALUES: distinct values per key of the on-chip tier
CR_TILE = 2048                # rows per tile of jh_causal.hip's scan (the tests straddle its edges)


class JhCausalReverseOpts(C.Structure):
    _fields_ = [("path", C.c_int32), ("pad", C.c_int32), ("reserved", C.c_int64 * 4)]


class JhCausalReverseResult(C.Structure):
    _fields_ = [("valid", C.c_int32), ("cause", C.c_int32), ("path", C.c_int32), ("pad", C.c_int32),
                ("read_count", C.c_int64), ("error_count", C.c_int64), ("invalid_keys", C.c_int64),
                ("first_error_row", C.c_int64), ("missing_total", C.c_int64), ("entries", C.c_int64),
                ("device_ms", C.c_double)]


# (independent/checker (checker/set)), jh_check_set_independent (additive to ABI 8)
SI_PATH_AUTO, SI_PATH_LDS, SI_PATH_GLOBAL = 0, 1, 2
SI_LDS_SPAN = 1 << 17         # JH_SI_LDS_SPAN: elements per key of the on-chip tier
SI_WORDS_MAX = 1 << 28        # JH_SI_WORDS_MAX: bitmap words over all keys
SI_SPAN_MAX = 1 << 34         # elements a key may span
SET_KEY_FIELDS = ("rows", "attempt_count", "acknowledged_count", "ok_count", "lost_count", "recovered_count",
                  "unexpected_count", "first_fail_entry", "final_read_entry", "base", "word_off", "n_words")


class JhSetIndepOpts(C.Structure):
    _fields_ = [("path", C.c_int32), ("pad", C.c_int32), ("reserved", C.c_int64 * 4)]


# (independent/checker (checker/linearizable {:model (multi-register init)})), jh_check_multi_register (additive to ABI 8)
MR_MAX_WINDOW = 64
MR_MAX_MOPS = 64              # JH_CY_MAX_MOPS
MR_GEN_JUMP = 1


class JhMultiRegisterOpts(C.Structure):
    _fields_ = [("budget", C.c_int64), ("n_regs", C.c_int32), ("bits", C.c_int32), ("init", _p64),
                ("waves", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int64 * 4)]


class JhSetKey(C.Structure):
    _fields_ = [("valid", C.c_int32), ("cause", C.c_int32)] + [(f, C.c_int64) for f in SET_KEY_FIELDS]


class JhSetIndepResult(C.Structure):
    _fields_ = [("valid", C.c_int32), ("cause", C.c_int32), ("path", C.c_int32), ("pad", C.c_int32),
                ("keys_valid", C.c_int64), ("keys_invalid", C.c_int64), ("keys_unknown", C.c_int64),
                ("first_fail_entry", C.c_int64), ("total_words", C.c_int64), ("entries", C.c_int64),
                ("device_ms", C.c_double)]


CY_PROCESS, CY_REALTIME, CY_WR = 1, 2, 4
CY_PATH_AUTO, CY_PATH_LDS, CY_PATH_GLOBAL = 0, 1, 2
CY_LDS_VERTICES = 2048        # JH_CY_LDS_VERTICES: vertices of a region of the on-chip tier
CY_MAX_MOPS = 64              # JH_CY_MAX_MOPS: micro-ops per txn
CY_WORK_MULT = 64             # JH_CY_WORK_MULT: a region's work cap is this * (vertices + edges)
CY_SCC_CAP = 8                # cycle.clj:926: (take 8) of the sorted SCCs
CAUSE_DOUBLE_INVOKE, CAUSE_ORPHAN, CAUSE_UNMATCHED_INVOKE = 3, 4, 12
CAUSES[12] = "unmatched-invoke"
# appends-and-reads-graph (additive to ABI 8)
CY_APPEND = 16                # JH_CY_APPEND (8 is not an analyzer)
CY_MONOTONIC = 32             # JH_CY_MONOTONIC: monotonic-key-graph over map reads
F_APPEND = 7                  # JH_F_APPEND: micro-op f of an append txn
CY_AP_DIRECT_READ = 4096      # JH_CY_AP_DIRECT_READ: elements of a read the direct duplicate check takes
CAUSE_DUPLICATE_APPENDS, CAUSE_DUPLICATE_ELEMENTS, CAUSE_NO_TOTAL_ORDER, CAUSE_NO_WRITER = 13, 14, 15, 16
CAUSES.update({13: "duplicate-appends", 14: "duplicate-elements", 15: "no-total-state-order", 16: "no-writer"})


# jepsen.tests.causal and adya/g2-checker (additive to ABI 8)
F_INSERT, F_READ_INIT = 8, 9  # JH_F_INSERT, JH_F_READ_INIT
CAUSAL_INIT = NIL + 1         # JH_CAUSAL_INIT: a :link of :init
CAUSE_BAD_F = 5
CM_TILE = 1024                # sorted slots per tile of jh_causalreg.hip's judge kernel (the tests straddle its edges)
CM_FLAG_TILE = 2048           # rows per tile of its flag pass
G2_TILE = 2048                # keys per tile of jh_g2.hip's key pass
CM_KINDS = {0: None, 1: "link", 2: "write", 3: "read-init", 4: "read", 5: "unknown-f"}


class JhCausalOpts(C.Structure):
    _fields_ = [("reserved", C.c_int64 * 4)]


class JhCausalKey(C.Structure):
    _fields_ = [("valid", C.c_int32), ("kind", C.c_int32), ("row", C.c_int64), ("counter", C.c_int64),
                ("last_pos", C.c_int64)]


class JhCausalResult(C.Structure):
    _fields_ = [("valid", C.c_int32), ("cause", C.c_int32), ("ok_count", C.c_int64), ("invalid_keys", C.c_int64),
                ("unknown_keys", C.c_int64), ("first_event_row", C.c_int64), ("device_ms", C.c_double)]


class JhG2Opts(C.Structure):
    _fields_ = [("reserved", C.c_int64 * 4)]


class JhG2Result(C.Structure):
    _fields_ = [("valid", C.c_int32), ("cause", C.c_int32), ("key_count", C.c_int64), ("legal_count", C.c_int64),
                ("illegal_count", C.c_int64), ("insert_rows", C.c_int64), ("first_illegal_row", C.c_int64),
                ("device_ms", C.c_double)]


# checker/perf: jh_perf (additive to ABI 8)
PERF_PAIR, PERF_POINTS, PERF_QUANTILES, PERF_RATE, PERF_ALL = 1, 2, 4, 8, 15   # JH_PERF_*
PERF_TILE = 1024              # sorted slots per tile of jh_perf.hip's pairing kernel (the tests straddle its edges)
PERF_DT_QUANTILES, PERF_DT_RATE = 30, 10      # perf.clj:505, :549
PERF_QS = (0.5, 0.95, 0.99, 1.0)              # the picks of a jh_perf group record, words 3..6
PERF_TYPE_ORDER = (TYPE_OK, TYPE_INFO, TYPE_FAIL)   # perf.clj:173-175


class JhPerfOpts(C.Structure):
    _fields_ = [("f_count", C.c_int64), ("dt_quantiles", C.c_int64), ("dt_rate", C.c_int64),
                ("want", C.c_int32), ("pad", C.c_int32), ("reserved", C.c_int64 * 4)]


class JhPerfResult(C.Structure):
    _fields_ = [("n_invokes", C.c_int64), ("n_paired", C.c_int64), ("n_unpaired_invokes", C.c_int64),
                ("first_unpaired_invoke", C.c_int64), ("t_max", C.c_int64),
                ("n_series", C.c_int64), ("n_groups", C.c_int64), ("n_cells", C.c_int64),
                ("has_quantiles", C.c_int32), ("pad", C.c_int32), ("device_ms", C.c_double)]


class JhCycleOpts(C.Structure):
    _fields_ = [("analyzers", C.c_int32), ("path", C.c_int32), ("extra_src", _p64), ("extra_dst", _p64),
                ("n_extra", C.c_int64), ("reserved", C.c_int64 * 4)]


class JhCycleResult(C.Structure):
    _fields_ = [("valid", C.c_int32), ("cause", C.c_int32), ("path", C.c_int32), ("pad", C.c_int32),
                ("scc_count", C.c_int64), ("scc_vertices", C.c_int64), ("edge_count", C.c_int64 * 4),
                ("back_edges", C.c_int64), ("regions", C.c_int64), ("max_region", C.c_int64),
                ("global_regions", C.c_int64), ("unknown_row", C.c_int64), ("unknown_key", C.c_int64),
                ("unknown_value", C.c_int64), ("unknown_rows", C.c_int64 * 2), ("entries", C.c_int64),
                ("device_ms", C.c_double)]


# numpy structured dtype with the same layout as jh_key_verdict
try:
    import numpy as _np
    VERDICT_DTYPE = _np.dtype([("valid", _np.int32), ("cause", _np.int32),
                               ("fail_entry", _np.int64), ("explored", _np.int64),
                               ("previous_ok", _np.int64), ("last_op", _np.int64),
                               ("analyzer", _np.int32), ("reserved", _np.int32)])
    # ... and as jh_causal_key
    CAUSAL_KEY_DTYPE = _np.dtype([("valid", _np.int32), ("kind", _np.int32), ("row", _np.int64),
                                  ("counter", _np.int64), ("last_pos", _np.int64)])
    # ... and as jh_set_key
    SET_KEY_DTYPE = _np.dtype([("valid", _np.int32), ("cause", _np.int32)] + [(f, _np.int64) for f in SET_KEY_FIELDS])
except Exception:  # pragma: no cover
    VERDICT_DTYPE = None
    CAUSAL_KEY_DTYPE = None
    SET_KEY_DTYPE = None


def ptr64(a):
    """int64* for a C-contiguous numpy int64 array (or None)."""
    if a is None:
        return None
    return a.ctypes.data_as(_p64)


def make_history(cols, on_device=False):
    """Build a JhHistory from an object with numpy (or device-pointer) columns.

    `cols` must have attributes n, process, type, f, key, value, value2,
    n_keys, aux (may be None)."""
    h = JhHistory()
    h.n = int(cols.n)
    if on_device:
        def dp(x):
            return C.cast(C.c_void_p(int(x)), _p64) if x else None
        h.process, h.type, h.f = dp(cols.process), dp(cols.type), dp(cols.f)
        h.key, h.value, h.value2 = dp(cols.key), dp(cols.value), dp(cols.value2)
        h.aux = dp(getattr(cols, "aux", 0))
        h.on_device = 1
    else:
        h.process, h.type, h.f = ptr64(cols.process), ptr64(cols.type), ptr64(cols.f)
        h.key, h.value, h.value2 = ptr64(cols.key), ptr64(cols.value), ptr64(cols.value2)
        h.aux = ptr64(cols.aux) if getattr(cols, "aux", None) is not None else None
        h.on_device = 0
    h.n_keys = int(cols.n_keys)
    aux = getattr(cols, "aux", None)
    h.n_aux = int(len(aux)) if (aux is not None and not on_device) else int(getattr(cols, "n_aux", 0))
    return h
