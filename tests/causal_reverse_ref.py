"""CPU restatements of jepsen.tests.causal-reverse for the tests.

clj_check   a literal transcription of causal_reverse.clj:21-84: the loop with
            its sorted-set snapshots, (reduce set/union), clojure.set's
            difference with its (contains? seen x) branch -- an index test on a
            vector -- and nil behaving as Clojure's nil does. A Python list /
            tuple is a Clojure vector, a set / frozenset a set.
ref_cols    the closed form of include/jh.h over Columns, in numpy, key by key:
            what jh_check_causal_reverse must return, field by field, return
            code included. It is also the CPU baseline of
            tools/bench_causal_reverse.py.
FakeCtx     ref_cols behind _native.Context.check_causal_reverse's signature,
            so that the mirror's device paths run in the CPU tests.
"""
import numpy as np

from jepsen_amd import _abi as A
from jepsen_amd import _native

RAW_FIELDS = ("valid", "cause", "path", "read_count", "error_count", "invalid_keys", "first_error_row",
              "missing_total", "entries")
BIG = np.iinfo(np.int64).max


# -- the literal transcription ------------------------------------------------------
def _count(s):
    return 0 if s is None else len(s)


def _conj_all(s, xs):
    for x in (xs or ()):
        s = s | {x}
    return s


def clj_union(s1, s2):
    """(set/union s1 s2): (reduce conj bigger smaller)."""
    return _conj_all(s2, s1) if _count(s1) < _count(s2) else _conj_all(s1, s2)


def _contains(coll, x):
    if coll is None:
        return False
    if isinstance(coll, (list, tuple)):          # a vector: is x one of its indices
        return isinstance(x, int) and not isinstance(x, bool) and 0 <= x < len(coll)
    return x in coll


def clj_difference(s1, s2):
    """(set/difference s1 s2)."""
    if _count(s1) < _count(s2):
        out = s1
        for item in (s1 or ()):
            if _contains(s2, item):
                out = out - {item}
        return out
    out = s1
    for item in (s2 or ()):
        if out is not None:
            out = out - {item}
    return out


def clj_graph(history):
    completed, expected = frozenset(), {}
    for op in history:
        if op.get("f") == "write":
            if op.get("type") == "invoke":
                expected[op.get("value")] = completed
            elif op.get("type") == "ok":
                completed = completed | {op.get("value")}
    return expected


def clj_errors(history, expected):
    errs = []
    for op in history:
        if op.get("type") != "ok" or op.get("f") != "read":
            continue
        seen = op.get("value")
        mapped = [expected.get(x) for x in (seen or ())]
        if not mapped:
            ours = frozenset()                     # (reduce set/union ()) = (set/union) = #{}
        else:
            ours = mapped[0]
            for s in mapped[1:]:
                ours = clj_union(ours, s)
        missing = clj_difference(ours, seen)
        if missing:
            e = {k: v for k, v in op.items() if k != "value"}
            e["missing"] = sorted(missing)
            e["expected-count"] = _count(ours)
            errs.append(e)
    return errs


def clj_check(history, as_sets=False):
    """The reference's result map. as_sets: every read's :value as a set first
    (what checker(vectors_as_sets=True) and the device decide)."""
    history = list(history)
    if as_sets:
        history = [dict(op, value=frozenset(op["value"])) if op.get("f") == "read" and op.get("type") == "ok"
                   and isinstance(op.get("value"), (list, tuple)) else op for op in history]
    errs = clj_errors(history, clj_graph(history))
    return {"valid?": not errs, "errors": errs}


# -- the closed form over Columns ----------------------------------------------------
def ref_cols(cols, path=0, err_cap=None, missing_cap=None):
    """What jh_check_causal_reverse returns for these Columns: rc, the raw
    fields, key_valid, errors (k, 5) and missing, with the caps applied (None:
    everything)."""
    n = int(cols.n)
    keyed = cols.key is not None and cols.n_keys > 0
    K = int(cols.n_keys) if keyed else 1
    n_out = max(int(cols.n_keys), 1)
    out = {"rc": A.JH_OK, "valid": A.VALID, "cause": 0, "path": 0, "read_count": 0, "error_count": 0,
           "invalid_keys": 0, "first_error_row": -1, "missing_total": 0, "entries": 0,
           "key_valid": np.full(n_out, A.VALID, np.int32), "errors": np.zeros((0, 5), np.int64),
           "missing": np.zeros(0, np.int64)}
    if n == 0:
        return out
    typ, f = np.asarray(cols.type), np.asarray(cols.f)
    val, val2 = np.asarray(cols.value), np.asarray(cols.value2)
    aux = np.asarray(cols.aux) if cols.aux is not None else np.zeros(0, np.int64)
    n_aux = len(aux)
    wm = (f == A.F_WRITE) & ((typ == A.TYPE_INVOKE) | (typ == A.TYPE_OK))
    rm = (f == A.F_READ) & (typ == A.TYPE_OK)
    out["read_count"] = int(rm.sum())
    key = np.asarray(cols.key) if keyed else np.zeros(n, np.int64)
    used = wm | rm
    if (key[used] >= K).any():
        return dict(out, rc=A.JH_EINVAL)
    cnt = np.where(rm, val2, 0)
    start = np.where(cnt == 0, 0, val)
    bad = rm & ((cnt < 0) | ((cnt != 0) & ((start < 0) | (start > n_aux) | (cnt > n_aux - start))))
    if bad.any():
        return dict(out, rc=A.JH_EINVAL)
    if (key[used] < 0).any() or (val[wm] == A.NIL).any():
        return dict(out, rc=A.JH_EUNSUPPORTED)
    out["entries"] = int(cnt.sum())
    rows = np.arange(n)
    errs, missing, over = [], [], False
    for k in range(K):
        mine = key == k
        wr = rows[wm & mine]
        uniq, idx = np.unique(val[wr], return_inverse=True)
        over |= len(uniq) > A.CR_LDS_VALUES
        inv = typ[wr] == A.TYPE_INVOKE
        last_inv = np.full(len(uniq), -1, np.int64)
        first_ok = np.full(len(uniq), BIG, np.int64)
        np.maximum.at(last_inv, idx[inv], wr[inv])
        np.minimum.at(first_ok, idx[~inv], wr[~inv])
        done = np.sort(first_ok[first_ok < BIG])
        for r in rows[rm & mine]:
            el = aux[start[r]:start[r] + cnt[r]]
            pos = np.searchsorted(uniq, el)
            pos[pos >= len(uniq)] = 0
            hit = pos[uniq[pos] == el] if len(uniq) else pos[:0]
            M = int(last_inv[hit].max()) if len(hit) else -1
            c = int(np.searchsorted(done, M, "left"))
            gone = np.setdiff1d(uniq[first_ok < M], el)
            if len(gone):
                errs.append([int(r), k, c, len(gone), 0])
                missing.append(gone)
                out["key_valid"][k] = A.INVALID
    if over and path == A.CR_PATH_LDS:
        return dict(out, rc=A.JH_EINVAL, key_valid=np.full(n_out, A.VALID, np.int32))
    out["path"] = 2 if (path == A.CR_PATH_GLOBAL or over) else 1
    order = sorted(range(len(errs)), key=lambda i: errs[i][0])
    errs = [errs[i] for i in order]
    missing = [missing[i] for i in order]
    at = 0
    for e, g in zip(errs, missing):
        e[4] = at
        at += len(g)
    out["error_count"], out["missing_total"] = len(errs), at
    out["invalid_keys"] = int((out["key_valid"] == A.INVALID).sum())
    if errs:
        out["valid"] = A.INVALID
        out["first_error_row"] = errs[0][0]
        ea = np.asarray(errs, np.int64).reshape(-1, 5)
        ma = np.concatenate(missing).astype(np.int64)
        out["errors"] = ea if err_cap is None else ea[:max(int(err_cap), 0)]
        out["missing"] = ma if missing_cap is None else ma[:max(int(missing_cap), 0)]
    return out


class FakeCtx:
    """_native.Context.check_causal_reverse, answered by ref_cols."""

    def __init__(self):
        self.calls = 0

    def check_causal_reverse(self, cols, path=0, err_cap=0, missing_cap=0, on_device=False, key_valid=True):
        self.calls += 1
        r = ref_cols(cols, path, err_cap, missing_cap)
        if r["rc"] != A.JH_OK:
            raise _native.JhError(r["rc"], "ref_cols")
        return {k: v for k, v in r.items() if k != "rc"}
