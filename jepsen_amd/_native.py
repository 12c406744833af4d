"""ctypes binding of libjh.so (include/jh.h). The product path: there is no
CPU fallback. If the library or a GPU is missing, every call raises.
"""
import ctypes as C
import os
import threading

import numpy as np

from . import _abi as A

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JH_LIB") or os.path.join(_HERE, "libjh.so")   # JH_LIB: A/B builds (tools/)
_lib = None
_lock = threading.Lock()


class JhError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libjh error {code}: {msg}")
        self.code = code
        self.msg = msg


def lib():
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(f"{LIB_PATH} is missing: run `python -m jepsen_amd.build` "
                                   "(the HIP extension is required; there is no CPU fallback)")
            L = C.CDLL(LIB_PATH)
            H = C.POINTER(A.JhHistory)
            L.jh_version.restype = C.c_int
            L.jh_open.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
            L.jh_open_multi.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
            L.jh_open_devices.argtypes = [C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_void_p)]
            L.jh_n_devices.argtypes = [C.c_void_p]
            L.jh_key_index.argtypes = [C.c_void_p, H, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                       C.c_char_p, C.c_size_t]
            L.jh_key_costs.argtypes = [C.POINTER(A.JhHistory), C.POINTER(C.c_int64), C.c_char_p, C.c_size_t]
            L.jh_stage_history.argtypes = [C.c_void_p, H, C.POINTER(C.c_int64), C.c_char_p, C.c_size_t]
            L.jh_close.argtypes = [C.c_void_p]
            L.jh_close.restype = None
            L.jh_check_cas_independent.argtypes = [C.c_void_p, H, C.POINTER(A.JhLinOpts),
                                                   C.POINTER(A.JhKeyVerdict), C.POINTER(A.JhSummary),
                                                   C.c_char_p, C.c_size_t]
            L.jh_check_cas_independent_device.argtypes = L.jh_check_cas_independent.argtypes
            L.jh_lin_configs.argtypes = [C.c_void_p, H, C.POINTER(A.JhLinOpts), C.POINTER(C.c_int64), C.c_int64,
                                         C.c_int32, C.POINTER(A.JhLinConfig), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int64), C.c_int64, C.c_char_p, C.c_size_t]
            L.jh_check_cas.argtypes = [C.c_void_p, H, C.POINTER(A.JhLinOpts),
                                       C.POINTER(A.JhKeyVerdict), C.c_char_p, C.c_size_t]
            p64 = C.POINTER(C.c_int64)
            L.jh_check_counter.argtypes = [C.c_void_p, H, p64, C.c_int64, p64, p64, p64,
                                           C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                           C.c_char_p, C.c_size_t]
            L.jh_check_set.argtypes = [C.c_void_p, H, C.POINTER(A.JhSetResult), p64, p64, p64, p64,
                                       C.c_int64, C.c_char_p, C.c_size_t]
            p32 = C.POINTER(C.c_uint32)
            L.jh_check_set_bitmaps.argtypes = [C.c_void_p, H, C.POINTER(A.JhSetResult), p32, p32, p32, p32,
                                               C.c_int64, p64, p64, C.c_char_p, C.c_size_t]
            L.jh_check_set_full.argtypes = [C.c_void_p, H, p64, C.c_int32, C.POINTER(A.JhSetFullResult),
                                            p64, p64, p64, C.c_int64, C.c_char_p, C.c_size_t]
            L.jh_check_set_full_opts.argtypes = [C.c_void_p, H, p64, C.POINTER(A.JhSetFullOpts),
                                                 C.POINTER(A.JhSetFullResult), p64, p64, p64, C.c_int64,
                                                 C.c_char_p, C.c_size_t]
            L.jh_check_total_queue.argtypes = [C.c_void_p, H, C.POINTER(A.JhQueueResult), p64, p64, p64, p64,
                                               C.c_int64, C.c_char_p, C.c_size_t]
            L.jh_check_queue.argtypes = [C.c_void_p, H, C.POINTER(A.JhQueueResult), p64, C.c_int64,
                                         C.c_char_p, C.c_size_t]
            L.jh_check_unique_ids.argtypes = [C.c_void_p, H, C.POINTER(A.JhUniqueIdsOpts),
                                              C.POINTER(A.JhUniqueIdsResult), p64, C.c_int64, C.c_char_p, C.c_size_t]
            L.jh_check_bank.argtypes = [C.c_void_p, H, C.POINTER(A.JhBankOpts), C.POINTER(A.JhBankResult), p64,
                                        C.c_int64, p64, C.c_char_p, C.c_size_t]
            L.jh_check_long_fork.argtypes = [C.c_void_p, H, C.POINTER(A.JhLongForkOpts),
                                             C.POINTER(A.JhLongForkResult), p64, C.c_int64, C.c_char_p, C.c_size_t]
            L.jh_check_causal_reverse.argtypes = [C.c_void_p, H, C.POINTER(A.JhCausalReverseOpts),
                                                  C.POINTER(A.JhCausalReverseResult), C.POINTER(C.c_int32), p64,
                                                  C.c_int64, p64, C.c_int64, C.c_char_p, C.c_size_t]
            L.jh_check_set_independent.argtypes = [C.c_void_p, H, C.POINTER(A.JhSetIndepOpts),
                                                   C.POINTER(A.JhSetIndepResult), C.POINTER(A.JhSetKey),
                                                   p32, p32, p32, p32, C.c_int64, C.c_char_p, C.c_size_t]
            L.jh_check_multi_register.argtypes = [C.c_void_p, H, C.POINTER(A.JhMultiRegisterOpts),
                                                  C.POINTER(A.JhKeyVerdict), C.POINTER(A.JhSummary),
                                                  C.c_char_p, C.c_size_t]
            L.jh_check_causal.argtypes = [C.c_void_p, H, C.POINTER(A.JhCausalOpts), C.POINTER(A.JhCausalResult),
                                          C.POINTER(A.JhCausalKey), C.c_char_p, C.c_size_t]
            L.jh_check_g2.argtypes = [C.c_void_p, H, C.POINTER(A.JhG2Opts), C.POINTER(A.JhG2Result), p64, C.c_int64,
                                      C.c_char_p, C.c_size_t]
            L.jh_perf.argtypes = [C.c_void_p, H, p64, C.POINTER(A.JhPerfOpts), C.POINTER(A.JhPerfResult),
                                  p64, C.c_int64, p64, C.c_int64, p64, C.c_int64, p64, C.c_int64, p64, C.c_int64,
                                  C.c_char_p, C.c_size_t]
            L.jh_scc.argtypes = [C.c_void_p, C.c_int64, p64, p64, C.c_int64, C.POINTER(A.JhCycleOpts),
                                 C.POINTER(A.JhCycleResult), p64, p64, p64, C.c_int64, C.c_int64, C.c_char_p, C.c_size_t]
            L.jh_check_cycle.argtypes = [C.c_void_p, H, C.POINTER(A.JhCycleOpts), C.POINTER(A.JhCycleResult), p64, p64,
                                         p64, C.c_int64, C.c_int64, p64, C.c_int64, C.c_char_p, C.c_size_t]
            L.jh_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
            L.jh_host_free.argtypes = [C.c_void_p]
            # history ingest (include/jh_io.h), host code in the same library
            pp = C.POINTER(C.c_void_p)
            L.jh_ingest_file.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, pp, C.c_char_p, C.c_size_t]
            L.jh_ingest_buffer.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, pp,
                                           C.c_char_p, C.c_size_t]
            io = C.POINTER(A.JhIngestOpts)
            L.jh_ingest_file_opts.argtypes = [C.c_char_p, C.c_int, C.c_int, io, pp, C.c_char_p, C.c_size_t]
            L.jh_ingest_buffer_opts.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, io, pp,
                                                C.c_char_p, C.c_size_t]
            L.jh_ingest_history.argtypes = [C.c_void_p, H]
            L.jh_ingest_history.restype = None
            L.jh_ingest_time.argtypes = [C.c_void_p]
            L.jh_ingest_time.restype = p64
            L.jh_ingest_values_interned.argtypes = [C.c_void_p]
            L.jh_ingest_table_size.argtypes = [C.c_void_p, C.c_int]
            L.jh_ingest_table_size.restype = C.c_int64
            L.jh_ingest_table_entry.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_char_p, C.c_size_t]
            L.jh_ingest_table_entry.restype = C.c_int64
            L.jh_ingest_free.argtypes = [C.c_void_p]
            L.jh_ingest_free.restype = None
            if L.jh_version() != A.JH_ABI_VERSION:
                raise RuntimeError("libjh.so ABI version mismatch")
            _lib = L
    return _lib


EXPORTED_SYMBOLS = ["jh_version", "jh_open", "jh_open_multi", "jh_open_devices", "jh_n_devices", "jh_key_costs", "jh_key_index",
                    "jh_stage_history",
                    "jh_close", "jh_check_cas_independent",
                    "jh_check_cas", "jh_check_cas_independent_device", "jh_lin_configs", "jh_check_counter",
                    "jh_check_set", "jh_check_set_bitmaps", "jh_check_set_full", "jh_check_set_full_opts", "jh_check_total_queue", "jh_check_queue",
                    "jh_check_unique_ids", "jh_check_bank", "jh_check_long_fork", "jh_check_causal_reverse",
                    "jh_check_set_independent", "jh_check_multi_register",
                    "jh_check_causal", "jh_check_g2", "jh_perf",
                    "jh_scc", "jh_check_cycle",
                    "jh_host_alloc", "jh_host_free",
                    # include/jh_io.h
                    "jh_ingest_file", "jh_ingest_buffer", "jh_ingest_file_opts", "jh_ingest_buffer_opts", "jh_ingest_history", "jh_ingest_time",
                    "jh_ingest_values_interned", "jh_ingest_table_size", "jh_ingest_table_entry", "jh_ingest_free"]


def _raise(rc, err):
    if rc != A.JH_OK:
        raise JhError(rc, err.value.decode(errors="replace"))


def _opts(init, budget, stream=0, algorithm=None, exact_count=True, **tune):
    """jh_lin_opts. tune: flags, quick_budget, phase2_budget, helpers,
    helper_late_us, helper_stall_min, bfs_stall_min, xw_waves, p2_waves_per_cu (jh.h; all decide the same
    verdicts, the tests use them to reach the less common search paths).
    exact_count: JH_LIN_EXACT_COUNT, WGL's cache size for every key (what the
    parity tests compare with the oracle); the checkers pass False -- their
    result maps carry no :explored, and the count pass then leaves the
    critical path."""
    o = A.JhLinOpts()
    o.init_value = A.NIL if init is None else int(init)
    o.budget = int(budget or 0)
    o.stream = int(stream)
    if isinstance(algorithm, str):
        algorithm = A.ALGORITHMS[algorithm]
    o.algorithm = int(algorithm or 0)
    for k, v in tune.items():
        if k not in dict(A.JhLinOpts._fields_) or k in ("init_value", "budget", "stream", "algorithm", "reserved"):
            raise TypeError(f"unknown jh_lin_opts field {k}")
        setattr(o, k, int(v))
    if exact_count:
        o.flags |= A.LIN_EXACT_COUNT
    o.flags |= A.LIN_TAIL_FIELDS          # JhLinOpts / JhSummary have the round-8 fields
    return o


def key_costs(cols):
    """jh_key_costs: per-key search-cost estimate (entries + window sum), the
    weight that splits keys between devices. Host-only: needs no GPU."""
    h = A.make_history(cols)
    out = np.zeros(max(cols.n_keys, 1), dtype=np.int64)
    err = C.create_string_buffer(256)
    rc = lib().jh_key_costs(C.byref(h), out.ctypes.data_as(C.POINTER(C.c_int64)), err, len(err))
    _raise(rc, err)
    return out[:cols.n_keys]


class HostBuffer:
    """Page-locked host memory from jh_host_alloc, viewed as a numpy array:
    result buffers reused across calls (check_counter's reads, the set
    bitmaps), so their D2H runs at PCIe speed. Freed with the object."""

    def __init__(self, count, dtype):
        dt = np.dtype(dtype)
        p = C.c_void_p()
        err = C.create_string_buffer(256)
        _raise(lib().jh_host_alloc(max(int(count), 1) * dt.itemsize, C.byref(p), err, len(err)), err)
        self._p = p
        buf = (C.c_char * (max(int(count), 1) * dt.itemsize)).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=dt, count=max(int(count), 1))

    def __del__(self):
        p = getattr(self, "_p", None)
        if p is not None and p.value:
            self.array = None
            lib().jh_host_free(p)
            self._p = None


class Context:
    """One jh_ctx on one HIP device (jh_open / jh_close), or, with n_gpus, one
    context over devices 0..n_gpus-1 (jh_open_multi: the independent check is
    split by key over them inside libjh)."""

    def __init__(self, device=0, n_gpus=None, devices=None):
        L = lib()
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int32 * len(devices))(*devices)
            rc = L.jh_open_devices(arr, len(devices), C.byref(h))
        elif n_gpus is None:
            rc = L.jh_open(int(device), C.byref(h))
        else:
            rc = L.jh_open_multi(int(n_gpus), C.byref(h))
        if rc != A.JH_OK:
            raise JhError(rc, f"jh_open({device}, n_gpus={n_gpus}) failed (no usable HIP device?)")
        self._h = h
        self.device = device
        self.n_devices = L.jh_n_devices(h)

    def close(self):
        if getattr(self, "_h", None):
            lib().jh_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def key_index(self, cols):
        """jh_key_index: (key_off [n_keys+1], rows [n]) -- key k's rows are
        rows[key_off[k]:key_off[k+1]] in history order, the un-keyed rows
        rows[key_off[n_keys]:]."""
        h = A.make_history(cols)
        off = np.zeros(cols.n_keys + 1, np.int64)
        rows = np.zeros(max(cols.n, 1), np.int64)
        err = C.create_string_buffer(512)
        p64 = C.POINTER(C.c_int64)
        rc = lib().jh_key_index(self._h, C.byref(h), off.ctypes.data_as(p64), rows.ctypes.data_as(p64),
                                err, len(err))
        _raise(rc, err)
        return off, rows[:cols.n]

    def stage_history(self, cols):
        """jh_stage_history: the six int64 columns (process, type, f, key,
        value, value2) as the device holds them after staging the host
        history -- the packed path for >= 2 M rows (jh_ingest.hip)."""
        h = A.make_history(cols)
        out = np.zeros(6 * max(cols.n, 1), np.int64)
        err = C.create_string_buffer(512)
        _raise(lib().jh_stage_history(self._h, C.byref(h), A.ptr64(out), err, len(err)), err)
        return out[:6 * cols.n].reshape(6, cols.n)

    # -- linearizability ---------------------------------------------------
    def check_cas_independent(self, cols, init=None, budget=None, **tune):
        """Returns (verdicts: structured array [n_keys] of VERDICT_DTYPE, JhSummary)."""
        h = A.make_history(cols)
        out = np.zeros(max(cols.n_keys, 1), dtype=A.VERDICT_DTYPE)
        s = A.JhSummary()
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_cas_independent(self._h, C.byref(h), C.byref(_opts(init, budget, **tune)),
                                            out.ctypes.data_as(C.POINTER(A.JhKeyVerdict)),
                                            C.byref(s), err, len(err))
        _raise(rc, err)
        return out[:cols.n_keys], s

    def check_cas_independent_device(self, dcols, verdicts_dev_ptr, init=None, budget=None,
                                     stream=0, **tune):
        """dcols: object whose column attributes are device pointers (ints)."""
        h = A.make_history(dcols, on_device=True)
        s = A.JhSummary()
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_cas_independent_device(
            self._h, C.byref(h), C.byref(_opts(init, budget, stream, **tune)),
            C.cast(C.c_void_p(int(verdicts_dev_ptr)), C.POINTER(A.JhKeyVerdict)),
            C.byref(s), err, len(err))
        _raise(rc, err)
        return s

    def check_cas(self, cols, init=None, budget=None, **tune):
        h = A.make_history(cols)
        v = A.JhKeyVerdict()
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_cas(self._h, C.byref(h), C.byref(_opts(init, budget, **tune)), C.byref(v),
                                err, len(err))
        _raise(rc, err)
        return v.valid, v.cause, v.fail_entry, v.explored

    def check_cas_full(self, cols, init=None, budget=None, **tune):
        """jh_check_cas -> {valid, cause, fail_entry, explored, previous_ok, last_op}."""
        h = A.make_history(cols)
        v = A.JhKeyVerdict()
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_cas(self._h, C.byref(h), C.byref(_opts(init, budget, **tune)), C.byref(v),
                                err, len(err))
        _raise(rc, err)
        return {f: getattr(v, f) for f, _ in A.JhKeyVerdict._fields_}

    def lin_configs(self, cols, keys, per_key=A.CONFIGS_PER_KEY, init=None, budget=None, **tune):
        """jh_lin_configs: {key: None | [(model_value, linearized rows, pending rows, last_row)]}
        -- each invalid key's frontier, each valid :linear key's final
        configurations (include/jh.h)."""
        h = A.make_history(cols)
        keys = np.ascontiguousarray(np.asarray(keys, dtype=np.int64))
        nq = len(keys)
        out = (A.JhLinConfig * max(nq * per_key, 1))()
        n_out = np.zeros(max(nq, 1), np.int32)
        rows = np.zeros(max(nq * per_key * A.MAX_WINDOW, 1), np.int64)
        err = C.create_string_buffer(1024)
        rc = lib().jh_lin_configs(self._h, C.byref(h), C.byref(_opts(init, budget, **tune)),
                                  keys.ctypes.data_as(C.POINTER(C.c_int64)), nq, per_key, out,
                                  n_out.ctypes.data_as(C.POINTER(C.c_int32)), A.ptr64(rows), len(rows),
                                  err, len(err))
        _raise(rc, err)
        res = {}
        for i, k in enumerate(keys.tolist()):
            if n_out[i] < 0:
                res[k] = None
                continue
            cs = []
            for j in range(n_out[i]):
                c = out[i * per_key + j]
                r = rows[c.rows_off:c.rows_off + c.n_linearized + c.n_pending]
                cs.append((int(c.model_value), r[:c.n_linearized].tolist(), r[c.n_linearized:].tolist(),
                           int(c.last_row)))
            res[k] = cs
        return res

    # -- counter / set -----------------------------------------------------
    def check_counter(self, cols, reads_cap=None, on_device=False, out=None):
        """on_device: cols' columns are device pointers (the history already in HBM).
        out: an int64 array of >= 3 * reads_cap to receive the triples (e.g. a
        HostBuffer's, reused across calls); the returned reads view it."""
        h = A.make_history(cols, on_device=on_device)
        cap = cols.n if reads_cap is None else reads_cap
        if out is not None:
            if out.dtype != np.int64 or len(out) < 3 * max(cap, 1) or not out.flags.c_contiguous:
                raise ValueError("out: contiguous int64 array of at least 3 * reads_cap")
            reads = out
        else:
            reads = np.zeros(3 * max(cap, 1), np.int64)
        nr, ne, fe = C.c_int64(), C.c_int64(), C.c_int64()
        valid, cause = C.c_int32(), C.c_int32()
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_counter(self._h, C.byref(h), A.ptr64(reads), cap, C.byref(nr),
                                    C.byref(ne), C.byref(fe), C.byref(valid), C.byref(cause),
                                    err, len(err))
        _raise(rc, err)
        k = min(nr.value, cap)
        return {"valid": valid.value, "cause": cause.value, "reads": reads[:3 * k].reshape(-1, 3),
                "n_reads": nr.value, "n_errors": ne.value, "first_err_entry": fe.value}

    def check_set(self, cols, runs_cap=None, on_device=False):
        h = A.make_history(cols, on_device=on_device)
        n_aux = int(cols.n_aux) if on_device else len(cols.aux)
        cap = (cols.n + n_aux + 2) if runs_cap is None else runs_cap
        runs = [np.zeros(2 * max(cap, 1), np.int64) for _ in range(4)]
        r = A.JhSetResult()
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_set(self._h, C.byref(h), C.byref(r), *[A.ptr64(x) for x in runs], cap,
                                err, len(err))
        _raise(rc, err)
        out = {name: getattr(r, name) for name, _ in A.JhSetResult._fields_ if name != "n_runs"}
        out["runs"] = [runs[i][:2 * min(r.n_runs[i], cap)].reshape(-1, 2) for i in range(4)]
        out["n_runs"] = list(r.n_runs)
        return out

    def check_set_bitmaps(self, cols, words_cap=None, on_device=False, out=None):
        """jh_check_set_bitmaps: the counts plus the four result sets (ok,
        lost, unexpected, recovered) as uint32 bitmaps over [base, base + 32 *
        n_words); bits_to_runs turns one into sorted [lo hi] runs. out: four
        uint32 arrays of words_cap words (e.g. HostBuffers', reused)."""
        h = A.make_history(cols, on_device=on_device)
        r = A.JhSetResult()
        err = C.create_string_buffer(1024)
        p32 = C.POINTER(C.c_uint32)
        base, nw = C.c_int64(), C.c_int64()
        cap = 0 if words_cap is None else int(words_cap)
        if words_cap is None:
            # the element span is bounded by the history's own values (the :add
            # rows' and the reads' elements): size the output from them on the
            # host so the device pass runs once; a device-resident history has
            # no host copy to bound, so it starts small and grows once
            cap = _set_span_words(cols) if not on_device else 1 << 16
        for _ in range(2):
            if out is not None:
                if words_cap is None or len(out) != 4 or any(
                        b.dtype != np.uint32 or len(b) < max(cap, 1) or not b.flags.c_contiguous for b in out):
                    raise ValueError("out: four contiguous uint32 arrays of words_cap words")
                bits = list(out)
            else:
                bits = [np.zeros(max(cap, 1), np.uint32) for _ in range(4)]
            rc = lib().jh_check_set_bitmaps(self._h, C.byref(h), C.byref(r), *[b.ctypes.data_as(p32) for b in bits],
                                            cap, C.byref(base), C.byref(nw), err, len(err))
            _raise(rc, err)
            if nw.value <= cap or words_cap is not None:
                break
            cap = int(nw.value)
        out = {name: getattr(r, name) for name, _ in A.JhSetResult._fields_ if name != "n_runs"}
        out["n_runs"] = list(r.n_runs)
        out["base"], out["n_words"] = base.value, nw.value
        out["bits"] = [b[:min(nw.value, cap)] for b in bits]
        return out

    def check_set_full(self, cols, time, linearizable=False, list_cap=None, on_device=False, read_batch=0):
        """(checker/set-full {:linearizable? linearizable}). `time` is the :time
        column (numpy int64, or a device pointer when on_device); read_batch > 0
        caps the :ok reads per bitmap batch (jh_set_full_opts, tests)."""
        h = A.make_history(cols, on_device=on_device)
        cap = int(cols.n) if list_cap is None else list_cap
        lists = [np.zeros(max(cap, 1), np.int64) for _ in range(3)]
        r = A.JhSetFullResult()
        err = C.create_string_buffer(1024)
        tp = C.cast(C.c_void_p(int(time)), C.POINTER(C.c_int64)) if on_device else A.ptr64(time)
        o = A.JhSetFullOpts(linearizable=int(bool(linearizable)), read_batch=int(read_batch))
        rc = lib().jh_check_set_full_opts(self._h, C.byref(h), tp, C.byref(o), C.byref(r),
                                          *[A.ptr64(x) for x in lists], cap, err, len(err))
        _raise(rc, err)
        out = {name: getattr(r, name) for name, _ in A.JhSetFullResult._fields_}
        out["stable_latencies"] = list(r.stable_latencies)
        out["lost_latencies"] = list(r.lost_latencies)
        out["worst_stale"] = [(w.element, w.stable_latency, w.known_entry, w.last_absent_entry)
                              for w in r.worst_stale[:r.n_worst]]
        for i, nm in enumerate(["lost", "never_read", "stale"]):
            k = min(out[nm + "_count"], cap)
            out[nm] = lists[i][:k]
        return out

    # -- queues --------------------------------------------------------------
    def _queue_out(self, r, pairs, names):
        out = {name: getattr(r, name) for name, _ in A.JhQueueResult._fields_ if name != "n_pairs"}
        out["n_pairs"] = list(r.n_pairs)
        cap = len(pairs[0]) // 2
        for i, nm in enumerate(names):
            out[nm] = pairs[i][:2 * min(r.n_pairs[i], cap)].reshape(-1, 2)
        return out

    def check_total_queue(self, cols, pairs_cap=None, on_device=False):
        h = A.make_history(cols, on_device=on_device)
        cap = (cols.n + (int(cols.n_aux) if on_device else len(cols.aux)) + 1) if pairs_cap is None else pairs_cap
        pairs = [np.zeros(2 * max(cap, 1), np.int64) for _ in range(4)]
        r = A.JhQueueResult()
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_total_queue(self._h, C.byref(h), C.byref(r), *[A.ptr64(x) for x in pairs],
                                        cap, err, len(err))
        _raise(rc, err)
        return self._queue_out(r, pairs, ["lost", "unexpected", "duplicated", "recovered"])

    def check_queue(self, cols, pairs_cap=None, on_device=False):
        h = A.make_history(cols, on_device=on_device)
        cap = (cols.n + 1) if pairs_cap is None else pairs_cap
        pairs = [np.zeros(2 * max(cap, 1), np.int64)]
        r = A.JhQueueResult()
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_queue(self._h, C.byref(h), C.byref(r), A.ptr64(pairs[0]), cap, err, len(err))
        _raise(rc, err)
        return self._queue_out(r, pairs, ["final_queue"])


    # -- unique-ids ----------------------------------------------------------
    def check_unique_ids(self, cols, f_generate, path=0, dup_cap=A.UID_DUP_CAP, on_device=False):
        """jh_check_unique_ids: the result fields plus `duplicated`, a (k, 2)
        array of (id, count) in ascending id. f_generate: the f code of
        :generate in cols; path: 0 auto, 1 dense bitmap, 2 sorted."""
        h = A.make_history(cols, on_device=on_device)
        cap = max(int(dup_cap), 0)
        pairs = np.zeros(2 * max(cap, 1), np.int64)
        r = A.JhUniqueIdsResult()
        o = A.JhUniqueIdsOpts(f_generate=int(f_generate), path=int(path))
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_unique_ids(self._h, C.byref(h), C.byref(o), C.byref(r), A.ptr64(pairs), cap,
                                       err, len(err))
        _raise(rc, err)
        out = {name: getattr(r, name) for name, _ in A.JhUniqueIdsResult._fields_}
        out["duplicated"] = pairs[:2 * min(r.duplicated_count, cap)].reshape(-1, 2)
        return out


    # -- bank -----------------------------------------------------------------
    def check_bank(self, cols, n_accounts, total_amount, negative_balances=False, reads_cap=None, on_device=False):
        """jh_check_bank: the scalar result fields, `errors` (one dict per type in
        cond order, A.BANK_TYPES), `reads` (a (k, 3) array of [row, total,
        class] per :ok :read, k = min(n_reads, reads_cap)) and `n_reads`.
        reads_cap None: every read."""
        h = A.make_history(cols, on_device=on_device)
        cap = int(cols.n) if reads_cap is None else max(int(reads_cap), 0)
        reads = np.zeros(3 * max(cap, 1), np.int64)
        r = A.JhBankResult()
        o = A.JhBankOpts(total_amount=int(total_amount), n_accounts=int(n_accounts),
                         negative_balances=1 if negative_balances else 0)
        nr = C.c_int64()
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_bank(self._h, C.byref(h), C.byref(o), C.byref(r), A.ptr64(reads), cap, C.byref(nr),
                                 err, len(err))
        _raise(rc, err)
        out = {name: getattr(r, name) for name, _ in A.JhBankResult._fields_ if name != "errors"}
        out["errors"] = [{name: getattr(e, name) for name, _ in A.JhBankErr._fields_} for e in r.errors]
        out["reads"] = reads[:3 * min(nr.value, cap)].reshape(-1, 3)
        out["n_reads"] = nr.value
        return out

    # -- long-fork ------------------------------------------------------------
    def check_long_fork(self, cols, n, path=0, fork_cap=0, on_device=False):
        """jh_check_long_fork: the result fields plus `forks`, a (k, 2) array
        of [row_a, row_b], k = min(fork_count, fork_cap), in group / row order.
        n: the group size; path: 0 auto, 1 dense, 2 sparse."""
        h = A.make_history(cols, on_device=on_device)
        cap = max(int(fork_cap), 0)
        forks = np.zeros(2 * max(cap, 1), np.int64)
        r = A.JhLongForkResult()
        o = A.JhLongForkOpts(n=int(n), path=int(path))
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_long_fork(self._h, C.byref(h), C.byref(o), C.byref(r), A.ptr64(forks), cap, err, len(err))
        _raise(rc, err)
        out = {name: getattr(r, name) for name, _ in A.JhLongForkResult._fields_}
        out["forks"] = forks[:2 * min(r.fork_count, cap)].reshape(-1, 2)
        return out

    # -- causal-reverse -------------------------------------------------------
    def check_causal_reverse(self, cols, path=0, err_cap=0, missing_cap=0, on_device=False, key_valid=True):
        """jh_check_causal_reverse: the result fields plus `key_valid` (int32
        per key, max(n_keys, 1) of them; None when not asked for), `errors`, a
        (k, 5) array of [row, key, expected_count, missing_count,
        missing_offset], k = min(error_count, err_cap), in row order, and
        `missing`, the first min(missing_total, missing_cap) missing values. A
        cap of 0 passes a NULL pointer. path: 0 auto, 1 on-chip, 2 global."""
        h = A.make_history(cols, on_device=on_device)
        ecap, mcap = max(int(err_cap), 0), max(int(missing_cap), 0)
        errs = np.zeros(5 * ecap, np.int64) if ecap else None
        miss = np.zeros(mcap, np.int64) if mcap else None
        kv = np.full(max(int(cols.n_keys), 1), -1, np.int32) if key_valid else None
        r = A.JhCausalReverseResult()
        o = A.JhCausalReverseOpts(path=int(path))
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_causal_reverse(self._h, C.byref(h), C.byref(o), C.byref(r),
                                           kv.ctypes.data_as(C.POINTER(C.c_int32)) if key_valid else None,
                                           A.ptr64(errs), ecap, A.ptr64(miss), mcap, err, len(err))
        _raise(rc, err)
        out = {name: getattr(r, name) for name, _ in A.JhCausalReverseResult._fields_ if name != "pad"}
        out["key_valid"] = kv
        out["errors"] = (errs[:5 * min(r.error_count, ecap)] if ecap else np.zeros(0, np.int64)).reshape(-1, 5)
        out["missing"] = miss[:min(r.missing_total, mcap)] if mcap else np.zeros(0, np.int64)
        return out

    # -- independent set ------------------------------------------------------
    def check_multi_register(self, cols, n_regs, bits, init=None, budget=None, waves=0, flags=0):
        """jh_check_multi_register over columns in the multi-register txn layout
        (jepsen_amd.multi_register.encode): (verdicts [max(n_keys, 1)] of
        VERDICT_DTYPE, JhSummary). init: n_regs value ids, or None."""
        h = A.make_history(cols)
        out = np.zeros(max(cols.n_keys, 1), dtype=A.VERDICT_DTYPE)
        s = A.JhSummary()
        o = A.JhMultiRegisterOpts(budget=int(budget or 0), n_regs=int(n_regs), bits=int(bits), waves=int(waves),
                                  flags=int(flags))
        ini = None
        if init is not None:
            ini = np.ascontiguousarray(init, np.int64)
            o.init = A.ptr64(ini) if len(ini) else None
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_multi_register(self._h, C.byref(h), C.byref(o), out.ctypes.data_as(C.POINTER(A.JhKeyVerdict)),
                                           C.byref(s), err, len(err))
        _raise(rc, err)
        return out, s

    def check_set_independent(self, cols, path=0, words_cap=None, on_device=False):
        """jh_check_set_independent: the result fields plus `keys`, a structured
        array (A.SET_KEY_DTYPE) of max(n_keys, 1) records, and `bits`, the four
        result bitmaps (ok, lost, unexpected, recovered) of min(total_words,
        words_cap) words: key k's sets are words [word_off, word_off + n_words)
        over [base, base + 32 n_words). words_cap=None bounds total_words from
        the columns on the host, so the device pass runs once."""
        h = A.make_history(cols, on_device=on_device)
        cap = 0 if words_cap is None else max(int(words_cap), 0)
        if words_cap is None:
            cap = _set_indep_words(cols) if not on_device else 1 << 16
        keys = np.zeros(max(int(cols.n_keys), 1), A.SET_KEY_DTYPE)
        r, o = A.JhSetIndepResult(), A.JhSetIndepOpts(path=int(path))
        err = C.create_string_buffer(1024)
        p32 = C.POINTER(C.c_uint32)
        for _ in range(2):
            bits = [np.zeros(max(cap, 1), np.uint32) for _ in range(4)]
            rc = lib().jh_check_set_independent(self._h, C.byref(h), C.byref(o), C.byref(r),
                                                keys.ctypes.data_as(C.POINTER(A.JhSetKey)),
                                                *[b.ctypes.data_as(p32) for b in bits], cap, err, len(err))
            _raise(rc, err)
            if r.total_words <= cap or words_cap is not None:
                break
            cap = int(r.total_words)
        out = {name: getattr(r, name) for name, _ in A.JhSetIndepResult._fields_ if name != "pad"}
        out["keys"] = keys
        out["bits"] = [b[:min(r.total_words, cap)] for b in bits]
        return out

    # -- causal ---------------------------------------------------------------
    def check_causal(self, cols, on_device=False, keys=True):
        """jh_check_causal: the result fields plus `keys`, a structured array
        (A.CAUSAL_KEY_DTYPE) of max(n_keys, 1) records; None when not asked
        for (a NULL keys_out)."""
        h = A.make_history(cols, on_device=on_device)
        out = np.zeros(max(int(cols.n_keys), 1), A.CAUSAL_KEY_DTYPE) if keys else None
        r, o = A.JhCausalResult(), A.JhCausalOpts()
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_causal(self._h, C.byref(h), C.byref(o), C.byref(r),
                                   out.ctypes.data_as(C.POINTER(A.JhCausalKey)) if keys else None, err, len(err))
        _raise(rc, err)
        res = {name: getattr(r, name) for name, _ in A.JhCausalResult._fields_}
        res["keys"] = out
        return res

    # -- adya g2 --------------------------------------------------------------
    def check_g2(self, cols, illegal_cap=0, on_device=False):
        """jh_check_g2: the result fields plus `illegal`, a (k, 2) array of
        [key id, count], k = min(illegal_count, illegal_cap), in ascending key
        id. A cap of 0 passes a NULL pointer."""
        h = A.make_history(cols, on_device=on_device)
        cap = max(int(illegal_cap), 0)
        pairs = np.zeros(2 * cap, np.int64) if cap else None
        r, o = A.JhG2Result(), A.JhG2Opts()
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_g2(self._h, C.byref(h), C.byref(o), C.byref(r), A.ptr64(pairs), cap, err, len(err))
        _raise(rc, err)
        res = {name: getattr(r, name) for name, _ in A.JhG2Result._fields_}
        res["illegal"] = (pairs[:2 * min(r.illegal_count, cap)] if cap else np.zeros(0, np.int64)).reshape(-1, 2)
        return res

    # -- perf -----------------------------------------------------------------
    def perf(self, cols, time, on_device=False, want=A.PERF_ALL, f_count=None, dt_quantiles=0, dt_rate=0,
             pair_cap=None, pt_cap=None, series_cap=None, group_cap=None, cell_cap=None):
        """jh_perf: the result fields plus numpy arrays `pair` (per row the
        partner row or -1), `pt_row` (the paired invokes in series order),
        `series` (k, 3: f, completion type, count), `groups` (k, 7: f, bucket,
        count, latency at 0.5 / 0.95 / 0.99 / 1) and `cells` (k, 4: f, type,
        bucket, count). `time`: the :time column (numpy int64, or a device
        pointer when on_device). A cap of None asks for the whole list (a second
        call when the first guess was too small); a list that is not wanted is
        empty. f_count: default 16 + the interned f of cols."""
        h = A.make_history(cols, on_device=on_device)
        n = int(cols.n)
        want = int(want) or A.PERF_ALL
        if f_count is None:
            f_count = A.F_FIRST_INTERNED + len(getattr(cols, "f_names", None) or [])
        o = A.JhPerfOpts(f_count=int(f_count), dt_quantiles=int(dt_quantiles), dt_rate=int(dt_rate), want=want)
        if on_device:
            tp = C.cast(C.c_void_p(int(time)), C.POINTER(C.c_int64))
        else:
            t_host = np.ascontiguousarray(time, np.int64) if n else np.zeros(1, np.int64)   # held until the call returns
            tp = A.ptr64(t_host)
        guess = {"pair": n, "pt_row": n // 2 + 1, "series": 64, "groups": 1024, "cells": 1024}
        caps = {"pair": pair_cap, "pt_row": pt_cap, "series": series_cap, "groups": group_cap, "cells": cell_cap}
        width = {"pair": 1, "pt_row": 1, "series": 3, "groups": 7, "cells": 4}
        wanted = {"pair": want & A.PERF_PAIR, "pt_row": want & A.PERF_POINTS, "series": want & A.PERF_POINTS,
                  "groups": want & A.PERF_QUANTILES, "cells": want & A.PERF_RATE}
        count_of = {"pair": lambda r: n if wanted["pair"] else 0, "pt_row": lambda r: r.n_paired if wanted["pt_row"] else 0,
                    "series": lambda r: r.n_series, "groups": lambda r: r.n_groups, "cells": lambda r: r.n_cells}
        cur = {k: (guess[k] if caps[k] is None else max(int(caps[k]), 0)) if wanted[k] else 0 for k in caps}
        r = A.JhPerfResult()
        err = C.create_string_buffer(1024)
        for _ in range(2):
            bufs = {k: np.zeros(width[k] * cur[k], np.int64) if cur[k] else None for k in cur}
            args = []
            for k in ("pair", "pt_row", "series", "groups", "cells"):
                args += [A.ptr64(bufs[k]), cur[k]]
            rc = lib().jh_perf(self._h, C.byref(h), tp, C.byref(o), C.byref(r), *args, err, len(err))
            _raise(rc, err)
            short = [k for k in cur if caps[k] is None and wanted[k] and count_of[k](r) > cur[k]]
            if not short:
                break
            for k in short:
                cur[k] = int(count_of[k](r))
        res = {name: getattr(r, name) for name, _ in A.JhPerfResult._fields_ if name != "pad"}
        for k in cur:
            kk = min(int(count_of[k](r)), cur[k])
            a = bufs[k][:width[k] * kk] if bufs[k] is not None else np.zeros(0, np.int64)
            res[k] = a.reshape(-1, width[k]) if width[k] > 1 else a
        return res

    # -- cycle ----------------------------------------------------------------
    @staticmethod
    def _cycle_out(r, labels, off, rows, scc_cap):
        out = {name: getattr(r, name) for name, _ in A.JhCycleResult._fields_ if name != "pad"}
        out["edge_count"] = list(r.edge_count)
        out["unknown_rows"] = list(r.unknown_rows)
        out["labels"] = labels
        k = min(r.scc_count, scc_cap)
        out["sccs"] = [rows[off[i]:off[i + 1]].tolist() for i in range(k) if off[i + 1] <= len(rows)]
        return out

    def scc(self, n, src, dst, path=0, scc_cap=A.CY_SCC_CAP, rows_cap=None, want_labels=True):
        """jh_scc: the result fields plus `labels` (per vertex the smallest
        vertex of its SCC, or -1; None unless want_labels) and `sccs`, the
        member lists of the first scc_cap SCCs by (size, smallest vertex) that
        fit rows_cap (default n; 0 without labels)."""
        src, dst = np.ascontiguousarray(src, np.int64), np.ascontiguousarray(dst, np.int64)
        n = int(n)
        scc_cap = max(int(scc_cap), 0)
        rows_cap = (n if want_labels else 0) if rows_cap is None else max(int(rows_cap), 0)
        labels = np.full(max(n, 1), -1, np.int64) if want_labels else None
        off, rows = np.zeros(scc_cap + 1, np.int64), np.zeros(max(rows_cap, 1), np.int64)
        r, o = A.JhCycleResult(), A.JhCycleOpts(path=int(path))
        err = C.create_string_buffer(1024)
        rc = lib().jh_scc(self._h, n, A.ptr64(src), A.ptr64(dst), len(src), C.byref(o), C.byref(r), A.ptr64(labels),
                          A.ptr64(off), A.ptr64(rows), scc_cap, rows_cap, err, len(err))
        _raise(rc, err)
        return self._cycle_out(r, labels[:n] if want_labels else None, off, rows[:rows_cap], scc_cap)

    def check_cycle(self, cols, analyzers, path=0, extra=None, scc_cap=A.CY_SCC_CAP, rows_cap=None, edge_cap=0,
                    on_device=False):
        """jh_check_cycle: the result fields plus `labels`, `sccs` (as `scc`)
        and `edges`, a (k, 2) array of [src_row, dst_row], k = min(edges,
        edge_cap). extra: (src, dst) rows of edges built by the caller."""
        h = A.make_history(cols, on_device=on_device)
        n = int(cols.n)
        scc_cap = max(int(scc_cap), 0)
        rows_cap = n if rows_cap is None else max(int(rows_cap), 0)
        ecap = max(int(edge_cap), 0)
        labels, off, rows = np.full(max(n, 1), -1, np.int64), np.zeros(scc_cap + 1, np.int64), np.zeros(max(rows_cap, 1), np.int64)
        edges = np.zeros(2 * max(ecap, 1), np.int64)
        r, o = A.JhCycleResult(), A.JhCycleOpts(analyzers=int(analyzers), path=int(path))
        if extra is not None:
            xs, xd = np.ascontiguousarray(extra[0], np.int64), np.ascontiguousarray(extra[1], np.int64)
            o.extra_src, o.extra_dst, o.n_extra = A.ptr64(xs), A.ptr64(xd), len(xs)
        err = C.create_string_buffer(1024)
        rc = lib().jh_check_cycle(self._h, C.byref(h), C.byref(o), C.byref(r), A.ptr64(labels), A.ptr64(off),
                                  A.ptr64(rows), scc_cap, rows_cap, A.ptr64(edges) if ecap else None, ecap, err, len(err))
        _raise(rc, err)
        out = self._cycle_out(r, labels[:n], off, rows[:rows_cap], scc_cap)
        out["edges"] = edges[:2 * min(sum(r.edge_count), ecap)].reshape(-1, 2)
        return out


def _set_span_words(cols):
    """Bitmap words covering every element jh_check_set_bitmaps can see: the
    non-nil values of the :add invocations / completions and every read
    element in aux (a superset of the final read's), as jh_set.hip's
    k_set_scan / k_set_range bound [vmin, vmax]."""
    v = np.asarray(cols.value)
    t = np.asarray(cols.type)
    sel = (np.asarray(cols.f) == A.F_ADD) & ((t == A.TYPE_INVOKE) | (t == A.TYPE_OK)) & (v != A.NIL)
    vals = v[sel]
    aux = np.asarray(cols.aux) if cols.aux is not None else np.zeros(0, np.int64)
    lo = min([int(x.min()) for x in (vals, aux) if len(x)], default=0)
    hi = max([int(x.max()) for x in (vals, aux) if len(x)], default=0)
    # (a span over 2^34 elements is refused by the library before any copy)
    return max(1, min(((hi - lo) >> 5) + 2, (1 << 29) + 1))


def _set_indep_words(cols):
    """An upper bound of jh_check_set_independent's total_words from the
    columns: per key the span of its :add elements and of every read element of
    its :ok :read rows (a superset of its final read's), in words."""
    v, t, f = np.asarray(cols.value), np.asarray(cols.type), np.asarray(cols.f)
    n_keys = int(cols.n_keys)
    key = np.asarray(cols.key) if n_keys > 0 and cols.key is not None else np.zeros(len(v), np.int64)
    K = max(n_keys, 1)
    aux = np.asarray(cols.aux) if cols.aux is not None else np.zeros(0, np.int64)
    ok = (key >= 0) & (key < K)
    add = ok & (f == A.F_ADD) & ((t == A.TYPE_INVOKE) | (t == A.TYPE_OK)) & (v != A.NIL)
    lo = np.full(K, np.iinfo(np.int64).max, np.int64)
    hi = np.full(K, np.iinfo(np.int64).min, np.int64)
    np.minimum.at(lo, key[add], v[add])
    np.maximum.at(hi, key[add], v[add])
    c = np.asarray(cols.value2)
    rd = ok & (f == A.F_READ) & (t == A.TYPE_OK) & (v != A.NIL) & (v >= 0) & (c > 0) & (v <= len(aux)) & (c <= len(aux) - v)
    rows = np.nonzero(rd)[0]
    if len(rows):
        # per read the min / max of its aux range (ranges may overlap or come in any order)
        starts, counts = v[rows], c[rows]
        idx = np.repeat(starts - np.concatenate(([0], np.cumsum(counts)[:-1])), counts) + np.arange(int(counts.sum()))
        kk = np.repeat(key[rows], counts)
        np.minimum.at(lo, kk, aux[idx])
        np.maximum.at(hi, kk, aux[idx])
    some = lo <= hi
    d = np.where(some, hi.astype(np.uint64) - lo.astype(np.uint64), np.uint64(0))     # (exact: the difference wraps)
    words = np.where(d < np.uint64(A.SI_SPAN_MAX), d // np.uint64(32) + np.uint64(1), np.uint64(0))   # (a wider key is refused)
    return int(max(1, min(int(words.sum()), A.SI_WORDS_MAX + 1)))


def bits_to_runs(words, base):
    """Sorted [lo hi] runs of the elements base + i for the set bits i of a
    uint32 bitmap (bit b of word w is element base + 32 w + b)."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    if words.size == 0:
        return np.zeros((0, 2), np.int64)
    b = np.unpackbits(words.view(np.uint8), bitorder="little").astype(np.int8)
    d = np.diff(np.concatenate(([0], b, [0])))
    lo = np.nonzero(d == 1)[0]
    hi = np.nonzero(d == -1)[0] - 1
    return np.stack([lo + base, hi + base], axis=1).astype(np.int64)


_default = {}


def default_context(device=None):
    """Process-wide context per device (LOCAL_RANK by default)."""
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    with _lock:
        ctx = _default.get(device)
    if ctx is None:
        ctx = Context(device)
        with _lock:
            _default[device] = ctx
    return ctx
