"""jepsen.tests.long-fork on MI355X: the long-fork workload's checker (parallel
snapshot isolation's anomaly: two reads of one group of keys observe two
single-key writes in conflicting order).

Mirrors jepsen/src/jepsen/tests/long_fork.clj (names, argument meaning, result
maps, error behaviour). A txn is a list of micro-ops ["r", k, v] / ["w", k, v];
:valid? :unknown is the string "unknown".

Encoding (include/jh.h, "Long-fork txns"): f comes from the SHAPE of :value,
never from the op's :f. A read txn (every micro-op an "r"; None and [] too) has
f = F_READ, value = the index of its first pair in aux, value2 = its number of
pairs; pair j is aux[2*(value+j)] (key) and aux[2*(value+j)+1] (value, NIL =
nil). Only :ok rows carry their pairs; a nil :value, and a read txn of any
other type, is value = NIL, value2 = 0. A write txn (exactly one micro-op, a
"w") has f = F_WRITE, value = key, value2 = written value. Any other row has an
interned f >= 16 and value = value2 = NIL. Keys that are not integers and
values that are not integers or nil have no encoding (TypeError): the checker
then runs its host implementation, which follows the Clojure directly, handles
arbitrary key sets, and is the reference of the tests.

Stated deviations: forks are [a b] with a before b in the
history, ordered by group (ascending keys) then rows; rows are distinct ops;
two distinct non-nil values for one key of a group always raise; an
illegal-history error names the smallest row.
"""
import random

import numpy as np

from . import _abi as A
from . import history as H

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
OPAQUE = "opaque"             # decode: the :value of a row that held neither a read nor a write txn
FORK_CAP = 1024               # pairs asked for by the first call
FORK_LIMIT = 1 << 24          # the most pairs a second call asks for (256 MiB of rows); past it
#                               :forks holds the first FORK_LIMIT pairs and :fork-count the exact number
MSG_KEYS = "These reads did not query for the same keys, and therefore cannot be compared."
MSG_VALUES = ("These two read states contain distinct values for the same key; this checker assumes only one "
              "write occurs per key.")


class IllegalHistory(Exception):
    """(throw+ {:type :illegal-history ...}): .type, .msg, .row (the :index of
    the read named, or None) and the reference's other keys in .data."""

    def __init__(self, msg, row=None, **data):
        super().__init__(msg)
        self.type = "illegal-history"
        self.msg = msg
        self.row = row
        self.data = data


# -- micro-ops (jepsen.txn.micro-op) -------------------------------------------
def _mf(mop):
    return mop[0]


def _mk(mop):
    return mop[1]


def _mv(mop):
    return mop[2]


def _truthy(v):
    return v is not None and v is not False


# -- the namespace --------------------------------------------------------------
def group_for(n, k):
    """long_fork.clj:97-104: the keys of k's group, lower inclusive, upper
    exclusive (Clojure's floored mod, as Python's %)."""
    lo = k - k % n
    return range(lo, lo + n)


def read_txn_for(n, k, rng=random):
    """long_fork.clj:106-112."""
    ks = list(group_for(n, k))
    rng.shuffle(ks)
    return [["r", k, None] for k in ks]


_NOT_FOUND = object()


def read_compare(a, b):
    """long_fork.clj:158-196: -1 if a dominates, 0 if equal, 1 if b dominates,
    None if incomparable; (keys a) is a's insertion order."""
    if len(a) != len(b):
        raise IllegalHistory(MSG_KEYS, reads=[a, b])
    res = 0
    for k in a:
        va, vb = a[k], b.get(k, _NOT_FOUND)
        if vb is _NOT_FOUND:
            raise IllegalHistory(MSG_KEYS, reads=[a, b], key=k)
        if va == vb:
            continue
        if vb is None:
            if res > 0:
                return None
            res = -1
        elif va is None:
            if res < 0:
                return None
            res = 1
        else:
            raise IllegalHistory(MSG_VALUES, reads=[a, b], key=k)
    return res


def read_op_to_value_map(op):
    """long_fork.clj:198-206."""
    return {_mk(m): _mv(m) for m in (op.get("value") or ())}


def distinct_pairs(coll):
    """long_fork.clj:208-214, as [a b] with a before b in coll. Elements are
    told apart by position: rows are distinct ops (they carry :index)."""
    coll = list(coll)
    return [[coll[i], coll[j]] for i in range(len(coll)) for j in range(i + 1, len(coll))]


def find_forks(ops):
    """long_fork.clj:216-224."""
    ops = list(ops)
    maps = [read_op_to_value_map(op) for op in ops]
    return [[ops[i], ops[j]] for i in range(len(ops)) for j in range(i + 1, len(ops))
            if read_compare(maps[i], maps[j]) is None]


def read_txn_p(txn):
    return all(_mf(m) == "r" for m in (txn or ()))


def write_txn_p(txn):
    return txn is not None and len(txn) == 1 and _mf(txn[0]) == "w"


def legal_txn_p(txn):
    return read_txn_p(txn) or write_txn_p(txn)


def op_read_keys(op):
    return frozenset(_mk(m) for m in (op.get("value") or ()))


def _pr_set(ks):
    try:
        ks = sorted(ks)
    except TypeError:
        ks = list(ks)
    return "#{" + " ".join("nil" if k is None else str(k) for k in ks) + "}"


def _group_size_error(n, group, op):
    return IllegalHistory(f"Every read in this history should have observed exactly {n} keys, but this read "
                          f"observed {len(group)} instead: {_pr_set(group)}", row=op.get("index"), op=op)


def groups(n, read_ops):
    """long_fork.clj:248-261: the read ops partitioned by key set, in order of
    first appearance; throws for a group of the wrong size."""
    by = {}
    for op in read_ops:
        by.setdefault(op_read_keys(op), []).append(op)
    for group, ops in by.items():
        if len(group) != n:
            raise _group_size_error(n, group, ops[0])
    return list(by.values())


def reads(history):
    return [op for op in history if op.get("type") == "ok" and _is_txn(op.get("value")) and read_txn_p(op.get("value"))]


def early_reads(rs):
    return [op.get("value") for op in rs if not any(_truthy(_mv(m)) for m in (op.get("value") or ()))]


def late_reads(rs):
    return [op.get("value") for op in rs if all(_truthy(_mv(m)) for m in (op.get("value") or ()))]


def _is_txn(v):
    return v is None or isinstance(v, (list, tuple))


def ensure_no_multiple_writes_to_one_key(history):
    """long_fork.clj:273-288."""
    ks = set()
    for op in history:
        v = op.get("value")
        if op.get("type") == "invoke" and _is_txn(v) and write_txn_p(v):
            k = _mk(v[0])
            if k in ks:
                return {"valid?": "unknown", "error": ["multiple-writes", k]}
            ks.add(k)
    return None


def _group_key(ops):
    ks = op_read_keys(ops[0])
    try:
        return (0, sorted(ks))
    except TypeError:
        return (1, sorted(map(repr, ks)))


def _distinct_values_error(ops, row=None):
    """The illegal-history error of a group that holds two distinct non-nil
    values for one key, naming the smallest row involved; None without one."""
    seen, bad = {}, set()
    for op in ops:
        for k, v in read_op_to_value_map(op).items():
            if v is not None and seen.setdefault(k, v) != v:
                bad.add(k)
    if not bad:
        return None
    maps = [read_op_to_value_map(op) for op in ops]
    i = next(i for i, m in enumerate(maps) if any(m.get(k) is not None for k in bad))
    a = maps[i]
    for m in maps:
        for k in a:
            if k in bad and a[k] is not None and m[k] is not None and a[k] != m[k]:
                return IllegalHistory(MSG_VALUES, row=ops[i].get("index") if row is None else row, reads=[a, m], key=k)
    raise AssertionError("unreachable")


def ensure_no_long_forks(n, rs):
    """long_fork.clj:263-271, groups in ascending key order."""
    gs = sorted(groups(n, rs), key=_group_key)
    errs = [e for e in (_distinct_values_error(g) for g in gs) if e is not None]
    if errs:
        raise min(errs, key=lambda e: (e.row is None, e.row))
    forks = [f for g in gs for f in find_forks(g)]
    return {"valid?": False, "forks": forks} if forks else None


def _indexed(history):
    return [op if "index" in op else dict(op, index=i) for i, op in enumerate(history)]


def check_host(n, history):
    """The checker's result map, computed on the host as the Clojure does."""
    history = _indexed(history)
    rs = reads(history)
    out = {"reads-count": len(rs), "early-read-count": len(early_reads(rs)), "late-read-count": len(late_reads(rs))}
    out.update(ensure_no_multiple_writes_to_one_key(history) or ensure_no_long_forks(n, rs) or {"valid?": True})
    return out


# -- encoding ---------------------------------------------------------------------
def _long(x, what):
    if not H._is_int(x):
        raise TypeError(f"long-fork: {what} {x!r} is not an integer")
    if not I64_MIN <= x <= I64_MAX:
        raise OverflowError(f"long-fork: {what} {x!r} is not a long")
    return int(x)


def _value(v, what):
    if v is None:
        return A.NIL
    v = _long(v, what)
    if v == A.NIL:
        raise OverflowError(f"long-fork: {what} {v!r} collides with the nil sentinel")
    return v


def encode(history):
    """Op maps -> Columns (module docstring)."""
    history = list(history)
    n = len(history)
    proc = np.empty(n, np.int64)
    typ = np.empty(n, np.int64)
    fcol = np.empty(n, np.int64)
    val = np.full(n, A.NIL, np.int64)
    val2 = np.full(n, A.NIL, np.int64)
    aux = []
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
        if _is_txn(v) and read_txn_p(v):
            fcol[i] = A.F_READ
            val2[i] = 0
            if v is not None and t == "ok":
                val[i] = len(aux) // 2
                val2[i] = len(v)
                for m in v:
                    aux += [_long(_mk(m), "key"), _value(_mv(m), "value")]
        elif _is_txn(v) and write_txn_p(v):
            fcol[i] = A.F_WRITE
            val[i] = _long(_mk(v[0]), "key")
            val2[i] = _value(_mv(v[0]), "value")
        else:
            f = op.get("f")
            if f not in f_ids:
                f_ids[f] = A.F_FIRST_INTERNED + len(f_names)
                f_names.append(f)
            fcol[i] = f_ids[f]
    return H.Columns(n=n, process=proc, type=typ, f=fcol, key=np.full(n, -1, np.int64), value=val, value2=val2,
                     n_keys=0, aux=np.asarray(aux, np.int64).reshape(-1), f_names=f_names)


def decode_op(cols, i):
    """One row back to an op map (:index included): an :ok read gets its txn
    back, a write its [["w" k v]], a read txn of another type a nil :value.
    A row that was neither (interned f) gets the :value OPAQUE, which is no
    txn either: the encoding keeps nothing else of it. :f is the shape's name
    ("read" / "write") or the interned name."""
    p, fi = int(cols.process[i]), int(cols.f[i])
    t = H.TYPE_NAMES[int(cols.type[i])]
    nil = lambda x: None if x == A.NIL else int(x)          # noqa: E731
    if fi == A.F_READ:
        f, v = "read", None
        if int(cols.value[i]) != A.NIL:
            s, c = int(cols.value[i]), int(cols.value2[i])
            v = [["r", int(k), nil(x)] for k, x in np.asarray(cols.aux[2 * s:2 * (s + c)]).reshape(-1, 2).tolist()]
    elif fi == A.F_WRITE:
        f, v = "write", [["w", int(cols.value[i]), nil(int(cols.value2[i]))]]
    else:
        j = fi - A.F_FIRST_INTERNED
        f, v = (cols.f_names[j] if 0 <= j < len(cols.f_names) else fi), OPAQUE
    return {"process": p if p >= 0 else ("nemesis" if p == -1 else p), "type": t, "f": f, "value": v, "index": int(i)}


def decode(cols):
    return [decode_op(cols, i) for i in range(cols.n)]


# -- the checker ---------------------------------------------------------------
class LongForkChecker:
    """(long-fork/checker n), long_fork.clj:311-324, through
    jh_check_long_fork. check(test, history, opts): history is op maps, or
    Columns from `encode`. The fork op maps are rebuilt on the host from the
    rows the device names. What the device does not handle (JH_EUNSUPPORTED:
    n > 64, key sets other than group-for's, a key named twice; or a history
    without an encoding) runs through check_host."""

    def __init__(self, n, path=A.LF_PATH_AUTO):
        self.n = n
        self.path = path

    def check(self, test, history, opts):
        from . import _native
        from . import checker as K
        ops = None
        if isinstance(history, H.Columns):
            cols = history
        else:
            ops = _indexed(history)
            try:
                cols = encode(ops)
            except (TypeError, OverflowError):
                return check_host(self.n, ops)
        op_at = (lambda row: ops[row]) if ops is not None else (lambda row: decode_op(cols, int(row)))
        if not (H._is_int(self.n) and self.n >= 1):
            return check_host(self.n, ops if ops is not None else decode(cols))
        ctx = K._ctx()
        try:
            r = ctx.check_long_fork(cols, self.n, self.path, FORK_CAP)
            if r["fork_count"] > FORK_CAP:
                r = ctx.check_long_fork(cols, self.n, self.path, min(r["fork_count"], FORK_LIMIT))
        except _native.JhError as e:
            if e.code != A.JH_EUNSUPPORTED:
                raise
            return check_host(self.n, ops if ops is not None else decode(cols))
        out = {"reads-count": int(r["reads_count"]), "early-read-count": int(r["early_count"]),
               "late-read-count": int(r["late_count"])}
        if r["cause"] == A.CAUSE_MULTIPLE_WRITES:
            out.update({"valid?": "unknown", "error": ["multiple-writes", int(r["multiple_key"])]})
        elif r["illegal_kind"] == A.LF_ILLEGAL_GROUP_SIZE:
            op = op_at(r["illegal_row"])
            raise _group_size_error(self.n, op_read_keys(op), op)
        elif r["illegal_kind"] == A.LF_ILLEGAL_DISTINCT_VALUES:
            row = int(r["illegal_row"])
            ks = op_read_keys(op_at(row))
            rows = np.nonzero((np.asarray(cols.type) == A.TYPE_OK) & (np.asarray(cols.f) == A.F_READ))[0]
            group = [op for op in (op_at(int(i)) for i in rows) if op_read_keys(op) == ks]
            raise _distinct_values_error(group, row)
        elif r["fork_count"]:
            out.update({"valid?": False, "forks": [[op_at(a), op_at(b)] for a, b in r["forks"].tolist()]})
            if r["fork_count"] > len(r["forks"]):
                out["fork-count"] = int(r["fork_count"])
        else:
            out["valid?"] = True
        return out


def checker(n, path=A.LF_PATH_AUTO):
    return LongForkChecker(n, path)


def workload(n=2):
    """long_fork.clj:326-332: the checker (the generator stays on the JVM;
    synth.long_fork_history follows its state machine)."""
    return {"checker": checker(n)}
