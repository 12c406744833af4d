"""jepsen.tests.adya on MI355X: the G2 (anti-dependency cycle over predicates)
workload's checker: at most one :insert may complete :ok for any key.

Mirrors jepsen/src/jepsen/tests/adya.clj:62-88 (names, result map). The checker
works over one flat history of {:f :insert :value [key [a-id b-id]]} ops, the
:value an independent tuple (a MapEntry); it is not lifted by
independent/checker.

Encoding (include/jh.h, "G2 ops"): the standard columns; f = F_INSERT for
:insert, an interned id otherwise; key = the interned (key (:value op)) of an
insert, -1 elsewhere. Only type, f and key are read. An :insert whose :value is
no map entry throws in the reference: `encode` raises TypeError and the checker
runs `check_host`, which raises the same way.
"""
import numpy as np

from . import _abi as A
from . import history as H

ILLEGAL_CAP = 1024            # illegal keys asked for by the first call


def check_host(history):
    """adya.clj:68-88, the reduce as it is written."""
    keys = {}
    for op in history:
        if op.get("f") != "insert":
            continue
        v = op.get("value")
        if not H.is_tuple(v):
            raise TypeError(f"g2: the :value {v!r} of an :insert is no map entry")
        k = v.key
        if op.get("type") == "ok":
            keys[k] = keys.get(k, 0) + 1
        else:
            keys.setdefault(k, 0)
    insert_count = sum(1 for c in keys.values() if c > 0)
    illegal = {k: keys[k] for k in sorted(k for k, c in keys.items() if c > 1)}
    return {"valid?": not illegal, "key-count": len(keys), "legal-count": insert_count - len(illegal),
            "illegal-count": len(illegal), "illegal": illegal}


def encode(history):
    """Op maps -> Columns (module docstring); keys are interned in order of
    their first insert. TypeError for an :insert without a tuple."""
    history = list(history)
    n = len(history)
    proc = np.empty(n, np.int64)
    typ = np.empty(n, np.int64)
    fcol = np.empty(n, np.int64)
    key = np.full(n, -1, np.int64)
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
        f = op.get("f")
        if isinstance(f, str) and f == "insert":
            fcol[i] = A.F_INSERT
            v = op.get("value")
            if not H.is_tuple(v):
                raise TypeError(f"g2: the :value {v!r} of an :insert is no map entry")
            if v.key not in key_ids:
                key_ids[v.key] = len(keys)
                keys.append(v.key)
            key[i] = key_ids[v.key]
        else:
            try:
                hash(f)
            except TypeError:
                f = repr(f)
            if f not in f_ids:
                f_ids[f] = A.F_FIRST_INTERNED + len(f_names)
                f_names.append(f)
            fcol[i] = f_ids[f]
    zeros = np.zeros(n, np.int64)
    return H.Columns(n=n, process=proc, type=typ, f=fcol, key=key, value=zeros, value2=zeros.copy(), n_keys=len(keys),
                     aux=np.zeros(1, np.int64), keys=keys, f_names=f_names)


def device_result(ctx, cols):
    """The raw result of jh_check_g2 with every illegal pair: a second call
    when the first cap was too small."""
    res = ctx.check_g2(cols, ILLEGAL_CAP)
    if res["illegal_count"] > ILLEGAL_CAP:
        res = ctx.check_g2(cols, res["illegal_count"])
    return res


def result_map(res, keys):
    """The checker's map from the raw result; keys: key id -> key. :illegal is
    in the order of the real keys (the reference's sorted-map)."""
    counts = {keys[int(kid)]: int(c) for kid, c in res["illegal"].tolist()}
    illegal = {k: counts[k] for k in sorted(counts)}
    return {"valid?": res["valid"] == A.VALID, "key-count": int(res["key_count"]),
            "legal-count": int(res["legal_count"]), "illegal-count": int(res["illegal_count"]), "illegal": illegal}


class G2Checker:
    """(adya/g2-checker) through jh_check_g2. check(test, history, opts):
    history is op maps, or Columns from `encode`."""

    def check(self, test, history, opts):
        from . import _native
        from . import checker as K
        if isinstance(history, H.Columns):
            cols = history
        else:
            ops = list(history)
            try:
                cols = encode(ops)
            except TypeError:
                return check_host(ops)           # raises what the reference throws
        try:
            res = device_result(K._ctx(), cols)
        except _native.JhError as e:
            if e.code != A.JH_EUNSUPPORTED or isinstance(history, H.Columns):
                raise
            return check_host(ops)
        return result_map(res, cols.keys if cols.keys else list(range(int(cols.n_keys))))


def g2_checker():
    return G2Checker()


def workload(opts=None):
    """The checker package of the G2 test maps (cockroachdb adya.clj:95-98,
    faunadb g2.clj:75); the generator g2-gen stays on the JVM
    (synth.g2_history follows it)."""
    return {"checker": g2_checker()}
