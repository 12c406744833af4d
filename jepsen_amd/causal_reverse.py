"""jepsen.tests.causal-reverse on MI355X: the "sequential" strict-serializability
workload's checker (T1 < T2, but T2 is visible without T1).

Mirrors jepsen/src/jepsen/tests/causal_reverse.clj (names, argument meaning,
result maps). The checker is per key; `independent.checker(checker())` checks
every key of a history with ONE jh_check_causal_reverse call.

Encoding (include/jh.h, "Causal-reverse"): the standard columns. A :write has
f = F_WRITE and value = the written integer; an :ok :read has f = F_READ,
value = the offset of its elements in aux and value2 = their number (a nil or
empty :value: value2 = 0). Values that are not integers have no encoding
(TypeError): the checker then runs `check_host`, which follows the Clojure
literally.

The vector quirk. The reference computes (set/difference our-expected seen)
with `seen` the read's :value as it is. clojure.set/difference walks the smaller
collection and asks (contains? seen x): on a VECTOR that tests indices, not
elements, whenever |our-expected| < |seen|. The device reads :value as the set
of its elements. The mirror stays exact by default: a set / frozenset read goes
to the device, a list / tuple read (a Clojure vector) is judged by `check_host`,
index test included; `checker(vectors_as_sets=True)` sends vectors to the
device as sets (the stated deviation). :missing is a sorted
list.
"""
from collections.abc import Mapping

import numpy as np

from . import _abi as A
from . import history as H

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ERR_CAP = 1024                # failing reads asked for by the first call
MISSING_CAP = 1 << 16         # missing values asked for by the first call
OUT_LIMIT = 1 << 24           # the most of either a second call asks for; past it :errors holds the
#                               first OUT_LIMIT and :error-count the exact number


# -- the namespace --------------------------------------------------------------
class Graph(Mapping):
    """(graph history): value -> the set of values known complete when the
    value's last write was invoked. The reference's snapshots of one sorted-set
    are prefixes of the completion order, kept here as a length each."""

    def __init__(self, order, counts):
        self.order = order            # distinct values in order of their first :ok
        self.counts = counts          # value -> how many of `order` were complete at its last :invoke

    def __getitem__(self, v):
        return frozenset(self.order[:self.counts[v]])

    def __iter__(self):
        return iter(self.counts)

    def __len__(self):
        return len(self.counts)


def graph(history):
    """causal_reverse.clj:21-49: a first-order write precedence graph."""
    order, done, counts = [], set(), {}
    for op in history:
        if op.get("f") != "write":
            continue
        t = op.get("type")
        if t == "invoke":
            counts[op.get("value")] = len(order)
        elif t == "ok":
            v = op.get("value")
            if v not in done:
                done.add(v)
                order.append(v)
    return Graph(order, counts)


def _difference(s1, seen, vectors_as_sets):
    """(set/difference s1 seen), clojure.set: with fewer elements in s1 it keeps
    the x of s1 for which (contains? seen x) is false -- an index test when
    seen is a vector; otherwise (reduce disj s1 seen)."""
    n_seen = 0 if seen is None else len(seen)
    if isinstance(seen, (list, tuple)) and not vectors_as_sets and len(s1) < n_seen:
        return {x for x in s1 if not (H._is_int(x) and 0 <= x < n_seen)}
    return set(s1) - set(seen or ())


def _sorted(xs):
    try:
        return sorted(xs)
    except TypeError:
        return sorted(xs, key=repr)


def error_map(op, missing, expected_count):
    out = {k: v for k, v in op.items() if k != "value"}
    out["missing"] = _sorted(missing)
    out["expected-count"] = int(expected_count)
    return out


def errors(history, expected, vectors_as_sets=False):
    """causal_reverse.clj:51-73: the :ok reads that violate the expected write
    order, each without :value and with :missing and :expected-count."""
    out = []
    for op in history:
        if op.get("type") != "ok" or op.get("f") != "read":
            continue
        seen = op.get("value")
        if isinstance(expected, Graph):           # nested prefixes: the union is the longest
            n = max((expected.counts.get(w, 0) for w in (seen or ())), default=0)
            ours = expected.order[:n]
        else:
            ours = set()
            for w in (seen or ()):
                ours |= set(expected.get(w) or ())
        missing = _difference(ours, seen, vectors_as_sets)
        if missing:
            out.append(error_map(op, missing, len(ours)))
    return out


def check_host(history, vectors_as_sets=False):
    """The checker's result map, computed on the host as the Clojure does."""
    history = list(history)
    errs = errors(history, graph(history), vectors_as_sets)
    return {"valid?": not errs, "errors": errs}


def r():
    return {"type": "invoke", "f": "read", "value": None}


def w(k):
    return {"type": "invoke", "f": "write", "value": k}


# -- encoding ---------------------------------------------------------------------
def _long(x):
    if not H._is_int(x):
        raise TypeError(f"causal-reverse: value {x!r} is not an integer")
    if not I64_MIN < x <= I64_MAX:
        raise OverflowError(f"causal-reverse: value {x!r} is not a long, or collides with the nil sentinel")
    return int(x)


def encode(history, keyed=False):
    """Op maps -> Columns (module docstring). keyed: independent tuples give the
    key column (interned in first-appearance order). A set read's elements are
    stored ascending, a vector's in its order. TypeError / OverflowError for a
    write or a read element that is no long."""
    history = list(history)
    n = len(history)
    proc = np.empty(n, np.int64)
    typ = np.empty(n, np.int64)
    fcol = np.empty(n, np.int64)
    key = np.full(n, -1, np.int64)
    val = np.full(n, A.NIL, np.int64)
    val2 = np.full(n, A.NIL, np.int64)
    aux = []
    key_ids, keys = {}, []
    f_ids, f_names, other_procs = {}, [], {"nemesis": -1}
    for i, op in enumerate(history):
        p = op.get("process")
        if H._is_int(p) and p >= 0:
            proc[i] = int(p)
        else:
            if p not in other_procs:
                other_procs[p] = -1 - len(other_procs)
            proc[i] = other_procs[p]
        t = op.get("type")
        if t not in H.TYPES:
            raise ValueError(f"unknown :type {t!r} in op {op!r}")
        typ[i] = H.TYPES[t]
        v = op.get("value")
        if keyed and H.is_tuple(v):
            if v.key not in key_ids:
                key_ids[v.key] = len(keys)
                keys.append(v.key)
            key[i] = key_ids[v.key]
            v = v.val
        f = op.get("f")
        if f == "write":
            fcol[i] = A.F_WRITE
            if t in ("invoke", "ok"):
                if v is None:
                    raise TypeError("causal-reverse: a write of nil")
                val[i] = _long(v)
            elif H._is_int(v) and I64_MIN < v <= I64_MAX:
                val[i] = int(v)                   # :fail / :info writes are never looked at
        elif f == "read":
            fcol[i] = A.F_READ
            val2[i] = 0
            if t == "ok" and v is not None:
                if not isinstance(v, (list, tuple, set, frozenset)):
                    raise TypeError(f"causal-reverse: a read of {v!r}")
                elems = [_long(x) for x in v]
                if isinstance(v, (set, frozenset)):
                    elems.sort()
                val[i] = len(aux)
                val2[i] = len(elems)
                aux += elems
        else:
            if f not in f_ids:
                f_ids[f] = A.F_FIRST_INTERNED + len(f_names)
                f_names.append(f)
            fcol[i] = f_ids[f]
    return H.Columns(n=n, process=proc, type=typ, f=fcol, key=key, value=val, value2=val2, n_keys=len(keys),
                     aux=np.asarray(aux, np.int64) if aux else np.zeros(1, np.int64), keys=keys, f_names=f_names)


def decode_op(cols, i, unwrap=False):
    """One row back to an op map: an :ok read gets its elements as a list in
    aux order, any other read nil, a write its value; a keyed row's :value is
    the independent tuple again unless `unwrap`."""
    p, fi = int(cols.process[i]), int(cols.f[i])
    t = H.TYPE_NAMES[int(cols.type[i])]
    if fi == A.F_READ:
        f, v = "read", None
        if t == "ok" and int(cols.value2[i]) > 0:
            s, c = int(cols.value[i]), int(cols.value2[i])
            v = [int(x) for x in np.asarray(cols.aux[s:s + c]).tolist()]
        elif t == "ok" and int(cols.value[i]) != A.NIL:
            v = []
    elif fi == A.F_WRITE:
        f, v = "write", (None if int(cols.value[i]) == A.NIL else int(cols.value[i]))
    else:
        j = fi - A.F_FIRST_INTERNED
        f, v = (cols.f_names[j] if 0 <= j < len(cols.f_names) else fi), None
    k = int(cols.key[i]) if cols.key is not None and cols.n_keys else -1
    if k >= 0 and not unwrap:
        v = H.tuple_(cols.keys[k] if k < len(cols.keys) else k, v)
    return {"process": p if p >= 0 else ("nemesis" if p == -1 else p), "type": t, "f": f, "value": v}


def decode(cols):
    return [decode_op(cols, i) for i in range(cols.n)]


# -- the checker ---------------------------------------------------------------
def device_ok(history, vectors_as_sets):
    """Whether every :ok read's :value is something the device may judge."""
    kinds = (set, frozenset, list, tuple) if vectors_as_sets else (set, frozenset)
    for op in history:
        if op.get("type") == "ok" and op.get("f") == "read":
            v = op.get("value")
            if H.is_tuple(v):
                v = v.val
            if v is not None and not isinstance(v, kinds):
                return False
    return True


def device_errors(ctx, cols, path):
    """The raw result of jh_check_causal_reverse with every error row and
    missing value (up to OUT_LIMIT): a second call when the first caps were
    too small."""
    res = ctx.check_causal_reverse(cols, path, ERR_CAP, MISSING_CAP)
    if res["error_count"] > ERR_CAP or res["missing_total"] > MISSING_CAP:
        res = ctx.check_causal_reverse(cols, path, min(res["error_count"], OUT_LIMIT),
                                       min(res["missing_total"], OUT_LIMIT))
    return res


def error_maps(res, op_at):
    """[(key id, error map)] of the listed error rows whose missing values
    arrived whole."""
    out = []
    missing = res["missing"]
    for row, kid, exp, cnt, off in res["errors"].tolist():
        if off + cnt > len(missing):
            break
        out.append((kid, error_map(op_at(row), missing[off:off + cnt].tolist(), exp)))
    return out


class CausalReverseChecker:
    """(causal-reverse/checker), causal_reverse.clj:75-84, through
    jh_check_causal_reverse. check(test, history, opts): history is op maps, or
    un-keyed Columns from `encode` (whose reads are sets by construction). What
    the device does not judge (a vector read unless vectors_as_sets, values
    without an encoding, JH_EUNSUPPORTED) runs through check_host."""

    def __init__(self, vectors_as_sets=False, path=A.CR_PATH_AUTO):
        self.vectors_as_sets = vectors_as_sets
        self.path = path

    def check(self, test, history, opts):
        from . import _native
        from . import checker as K
        if isinstance(history, H.Columns):
            cols, ops, as_sets = history, None, True
            op_at = lambda row: decode_op(cols, int(row), unwrap=True)          # noqa: E731
        else:
            ops, as_sets = list(history), self.vectors_as_sets
            if not device_ok(ops, as_sets):
                return check_host(ops, as_sets)
            try:
                cols = encode(ops)
            except (TypeError, OverflowError):
                return check_host(ops, as_sets)
            op_at = lambda row: ops[row]                                         # noqa: E731
        try:
            res = device_errors(K._ctx(), cols, self.path)
        except _native.JhError as e:
            if e.code != A.JH_EUNSUPPORTED:
                raise
            return check_host(ops if ops is not None else [decode_op(cols, i, unwrap=True) for i in range(cols.n)],
                              as_sets)
        errs = [m for _, m in error_maps(res, op_at)]
        out = {"valid?": res["valid"] == A.VALID, "errors": errs}
        if res["error_count"] > len(errs):
            out["error-count"] = int(res["error_count"])
        return out


def checker(vectors_as_sets=False, path=A.CR_PATH_AUTO):
    return CausalReverseChecker(vectors_as_sets, path)


def check_independent(inner, history):
    """{key: result map} for every key of an independent history with one
    device call, or None when the device does not judge it (the caller then
    checks key by key)."""
    from . import _native
    from . import checker as K
    if not device_ok(history, inner.vectors_as_sets):
        return None
    try:
        cols = encode(history, keyed=True)
    except (TypeError, OverflowError):
        return None
    if not cols.n_keys:
        return None
    try:
        res = device_errors(K._ctx(), cols, inner.path)
    except _native.JhError:
        # JH_EUNSUPPORTED, and any other refusal of the batched call (JH_ENOMEM of the global tier,
        # JH_EINVAL of a forced path): key by key, where check_safe turns what a key raises into :unknown
        return None
    if res["error_count"] > len(res["errors"]) or res["missing_total"] > len(res["missing"]):
        return None

    def op_at(row):
        op = dict(history[row])
        op["value"] = op["value"].val
        return op
    out = {key: {"valid?": bool(res["key_valid"][kid] == A.VALID), "errors": []} for kid, key in enumerate(cols.keys)}
    for kid, m in error_maps(res, op_at):
        out[cols.keys[kid]]["errors"].append(m)
    return out


def workload(opts=None):
    """causal_reverse.clj:89-111: the checker package (the generator stays on
    the JVM; synth.causal_reverse_history follows it)."""
    from . import checker as K
    from . import independent
    return {"checker": K.compose({"sequential": independent.checker(checker())})}
