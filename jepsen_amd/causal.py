"""jepsen.tests.causal on MI355X: the causal-order workload's checker (a causal
order of five ops, read-init write read write read, against one register per
key; every op carries the :position it took effect at and a :link to the
position it follows).

Mirrors jepsen/src/jepsen/tests/causal.clj (names, argument meaning, result
maps). The checker is per key; `independent.checker(check(causal_register()))`
checks every key of a history with ONE jh_check_causal call.

Encoding (include/jh.h, "Causal ops"): the standard columns. f = F_READ /
F_WRITE / F_READ_INIT or an interned id; value = :value (NIL for nil); aux holds
a (position, link) pair per row, NIL for nil and CAUSAL_INIT for the keyword
:init (the string "init" here). Only :ok rows are read, so only they are
encoded. A value, position or link that is no long in (I64_MIN + 1, I64_MAX]
has no encoding (TypeError / OverflowError): the checker then runs
`check_host`, which follows the Clojure literally. So does a model other than
the default (causal-register).
"""
from dataclasses import dataclass
from typing import Any

import numpy as np

from . import _abi as A
from . import history as H

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
INIT = "init"                 # the keyword :init of a :link


# -- Clojure's = and str on what an op may hold ---------------------------------------
def _is_num(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)


def clj_eq(a, b):
    """(= a b): numbers are equal within their category only (1 is not 1.0) and
    a boolean is no number."""
    if _is_num(a) and _is_num(b):
        return H._is_int(a) == H._is_int(b) and a == b
    if _is_num(a) or _is_num(b) or isinstance(a, bool) or isinstance(b, bool):
        return type(a) is type(b) and a == b
    return a == b


def clj_str(x):
    """(str x) of one value: nil is the empty string."""
    if x is None:
        return ""
    if isinstance(x, bool):
        return "true" if x else "false"
    return str(x)


# -- the namespace --------------------------------------------------------------
@dataclass(frozen=True)
class Inconsistent:
    """causal.clj:15-20: an invalid termination of a model."""
    msg: str

    def step(self, op):
        return self

    def __str__(self):
        return self.msg


def inconsistent(msg):
    return Inconsistent(msg)


def is_inconsistent(model):
    return isinstance(model, Inconsistent)


@dataclass(frozen=True)
class CausalRegister:
    """causal.clj:33-83."""
    value: Any
    counter: Any
    last_pos: Any

    def step(self, op):
        c = self.counter + 1
        v, pos, link = op.get("value"), op.get("position"), op.get("link")
        if not (clj_eq(link, INIT) or clj_eq(link, self.last_pos)):
            return inconsistent(f"Cannot link {clj_str(link)} to last-seen position {clj_str(self.last_pos)}")
        f = op.get("f")
        if f == "write":
            if clj_eq(v, c):
                return CausalRegister(v, c, pos)
            return inconsistent(f"expected value {clj_str(c)} attempting to write {clj_str(v)} instead")
        if f == "read-init":
            if clj_eq(0, self.counter) and not clj_eq(0, v):
                return inconsistent(f"expected init value 0, read {clj_str(v)}")
            if v is None or clj_eq(self.value, v):
                return CausalRegister(self.value, self.counter, pos)
            return inconsistent(f"can't read {clj_str(v)} from register {clj_str(self.value)}")
        if f == "read":
            if v is None or clj_eq(self.value, v):
                return CausalRegister(self.value, self.counter, pos)
            return inconsistent(f"can't read {clj_str(v)} from register {clj_str(self.value)}")
        raise ValueError(f"No matching clause: {f!r}")        # condp without a default throws

    def __str__(self):
        return "nil" if self.value is None else clj_str(self.value)


def causal_register():
    return CausalRegister(0, 0, None)


def check_host(model, history):
    """causal.clj:88-110, the loop as it is written: the result map, or what
    `step` raises."""
    s = model
    for op in history:
        if op.get("type") != "ok":
            continue
        s = s.step(op)
        if is_inconsistent(s):
            return {"valid?": False, "error": s.msg}
    return {"valid?": True, "model": s}


def r(_test=None, _process=None):
    return {"type": "invoke", "f": "read"}


def ri(_test=None, _process=None):
    return {"type": "invoke", "f": "read-init"}


def cw1(_test=None, _process=None):
    return {"type": "invoke", "f": "write", "value": 1}


def cw2(_test=None, _process=None):
    return {"type": "invoke", "f": "write", "value": 2}


# -- encoding ---------------------------------------------------------------------
def _long(x, what):
    if not H._is_int(x):
        raise TypeError(f"causal: {what} {x!r} is not an integer")
    if not I64_MIN + 1 < x <= I64_MAX:
        raise OverflowError(f"causal: {what} {x!r} is not a long, or collides with a sentinel")
    return int(x)


def encode(history, keyed=False):
    """Op maps -> Columns (module docstring). keyed: independent tuples give the
    key column (interned in first-appearance order). TypeError / OverflowError
    for an :ok op's value, position or link without an encoding, and in a keyed
    history for an :ok op without a tuple (it belongs to every key)."""
    history = list(history)
    n = len(history)
    proc = np.empty(n, np.int64)
    typ = np.empty(n, np.int64)
    fcol = np.empty(n, np.int64)
    key = np.full(n, -1, np.int64)
    val = np.full(n, A.NIL, np.int64)
    aux = np.full(2 * n, A.NIL, np.int64)
    key_ids, keys = {}, []
    f_ids, f_names, other_procs = {}, [], {"nemesis": -1}
    known = {"read": A.F_READ, "write": A.F_WRITE, "read-init": A.F_READ_INIT}
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
        elif keyed and t == "ok":
            raise TypeError("causal: an :ok op without a key in a keyed history")
        f = op.get("f")
        if isinstance(f, str) and f in known:
            fcol[i] = known[f]
        else:
            try:
                hash(f)
            except TypeError:
                f = repr(f)
            if f not in f_ids:
                f_ids[f] = A.F_FIRST_INTERNED + len(f_names)
                f_names.append(f)
            fcol[i] = f_ids[f]
        if t != "ok":
            continue                                  # the checker reads :ok ops only
        if fcol[i] < A.F_FIRST_INTERNED and v is not None:
            val[i] = _long(v, "value")
        pos, link = op.get("position"), op.get("link")
        if pos is not None:
            aux[2 * i] = _long(pos, "position")
        if isinstance(link, str) and link == INIT:
            aux[2 * i + 1] = A.CAUSAL_INIT
        elif link is not None:
            aux[2 * i + 1] = _long(link, "link")
    return H.Columns(n=n, process=proc, type=typ, f=fcol, key=key, value=val, value2=np.zeros(n, np.int64),
                     n_keys=len(keys), aux=aux, keys=keys, f_names=f_names)


def decode_op(cols, i, unwrap=False):
    """One row back to an op map (:position / :link only where they are not
    nil); a keyed row's :value is the independent tuple again unless `unwrap`."""
    p, fi = int(cols.process[i]), int(cols.f[i])
    names = {A.F_READ: "read", A.F_WRITE: "write", A.F_READ_INIT: "read-init"}
    j = fi - A.F_FIRST_INTERNED
    f = names.get(fi, cols.f_names[j] if 0 <= j < len(cols.f_names) else fi)
    v = None if int(cols.value[i]) == A.NIL else int(cols.value[i])
    k = int(cols.key[i]) if cols.key is not None and cols.n_keys else -1
    if k >= 0 and not unwrap:
        v = H.tuple_(cols.keys[k] if k < len(cols.keys) else k, v)
    op = {"process": p if p >= 0 else ("nemesis" if p == -1 else p), "type": H.TYPE_NAMES[int(cols.type[i])], "f": f,
          "value": v}
    pos, link = int(cols.aux[2 * i]), int(cols.aux[2 * i + 1])
    if pos != A.NIL:
        op["position"] = pos
    if link != A.NIL:
        op["link"] = INIT if link == A.CAUSAL_INIT else link
    return op


def decode(cols):
    return [decode_op(cols, i) for i in range(cols.n)]


# -- the checker ---------------------------------------------------------------
def _nil(x):
    return None if int(x) == A.NIL else int(x)


def key_result(rec, value, link):
    """One jh_causal_key record as the checker's result map. value, link: the
    event row's own :value and :link. None for a key the device left unknown
    (the reference throws there)."""
    valid, kind, counter, last = int(rec["valid"]), int(rec["kind"]), int(rec["counter"]), _nil(rec["last_pos"])
    if valid == A.VALID:
        return {"valid?": True, "model": CausalRegister(counter, counter, last)}
    if valid == A.UNKNOWN:
        return None
    if kind == 1:
        msg = f"Cannot link {clj_str(link)} to last-seen position {clj_str(last)}"
    elif kind == 2:
        msg = f"expected value {counter + 1} attempting to write {clj_str(value)} instead"
    elif kind == 3 and counter == 0:
        msg = f"expected init value 0, read {clj_str(value)}"
    else:
        msg = f"can't read {clj_str(value)} from register {counter}"
    return {"valid?": False, "error": msg}


class CausalChecker:
    """(causal/check model), causal.clj:88-110, through jh_check_causal when
    the model is (causal-register). check(test, history, opts): history is op
    maps, or un-keyed Columns from `encode`. What the device does not judge (an
    op without an encoding, another model, an unknown :f, JH_EUNSUPPORTED) runs
    through check_host, which raises where the reference throws."""

    def __init__(self, model):
        self.model = model

    def on_device(self):
        return type(self.model) is CausalRegister and self.model == causal_register()

    def check(self, test, history, opts):
        from . import _native
        from . import checker as K
        if isinstance(history, H.Columns):
            cols = history
            ops = None
        else:
            ops = list(history)
            cols = None
            if self.on_device():
                try:
                    cols = encode(ops)
                except (TypeError, OverflowError):
                    pass
        host = lambda: check_host(self.model, ops if ops is not None else            # noqa: E731
                                  [decode_op(cols, i, unwrap=True) for i in range(cols.n)])
        if cols is None or not self.on_device():
            return host()
        try:
            res = K._ctx().check_causal(cols)
        except _native.JhError as e:
            if e.code != A.JH_EUNSUPPORTED:
                raise
            return host()
        rec = res["keys"][0]
        row = int(rec["row"])
        op = {} if row < 0 else (ops[row] if ops is not None else decode_op(cols, row, unwrap=True))
        out = key_result(rec, op.get("value"), op.get("link"))
        return host() if out is None else out


def check(model):
    return CausalChecker(model)


def check_independent(inner, history):
    """({key: result map}, [the keys the device left unknown]) for every key of
    an independent history with one device call, or None when the device does
    not judge it (the caller then checks key by key)."""
    from . import _native
    from . import checker as K
    if not inner.on_device():
        return None
    try:
        cols = encode(history, keyed=True)
    except (TypeError, OverflowError):
        return None
    if not cols.n_keys:
        return None
    try:
        res = K._ctx().check_causal(cols)
    except _native.JhError:
        return None                          # JH_EUNSUPPORTED and any other refusal: key by key
    out, unknown = {}, []
    for kid, key in enumerate(cols.keys):
        rec = res["keys"][kid]
        row = int(rec["row"])
        v = history[row]["value"].val if row >= 0 else None
        m = key_result(rec, v, history[row].get("link") if row >= 0 else None)
        if m is None:
            unknown.append(key)
        out[key] = m
    return out, unknown


def workload(opts=None):
    """causal.clj:118-130: the checker package (the generator stays on the JVM;
    synth.causal_history follows it)."""
    from . import independent
    return {"checker": independent.checker(check(causal_register()))}
