"""CPU restatements of jepsen.tests.causal for the tests.

clj_check   a literal transcription of causal.clj:33-110: the CausalRegister's
            step with Clojure's = (1 is not 1.0, a boolean is no number, nil =
            nil), (str nil) = "", condp throwing on an :f without a clause, and
            the checker's loop over the :ok ops. It shares nothing with
            jepsen_amd.causal but the CausalRegister record the result map holds.
ref_cols    the closed form of include/jh.h over Columns, in numpy: what
            jh_check_causal must return, field by field, return code and every
            jh_causal_key included. It is also the CPU baseline's cross-check in
            tools/bench_causal.py.
FakeCtx     ref_cols behind _native.Context.check_causal's signature, so that
            the mirror's device paths run in the CPU tests.
"""
import numpy as np

from jepsen_amd import _abi as A
from jepsen_amd import _native
from jepsen_amd.causal import CausalRegister

RAW_FIELDS = ("valid", "cause", "ok_count", "invalid_keys", "unknown_keys", "first_event_row")


class NoMatchingClause(Exception):
    """condp's IllegalArgumentException."""


# -- the literal transcription ------------------------------------------------------
def _number(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool)


def _eq(a, b):
    if _number(a) and _number(b):
        return isinstance(a, int) == isinstance(b, int) and a == b
    if type(a) is not type(b):
        return False
    return a == b


def _str(x):
    if x is None:
        return ""
    if x is True or x is False:
        return "true" if x else "false"
    return str(x)


def clj_step(reg, op):
    """(step r op): the next (value, counter, last-pos), or the message of an
    Inconsistent as a string."""
    value, counter, last_pos = reg
    c = counter + 1
    v, pos, link = op.get("value"), op.get("position"), op.get("link")
    if not (_eq(link, "init") or _eq(link, last_pos)):
        return "Cannot link " + _str(link) + " to last-seen position " + _str(last_pos)
    f = op.get("f")
    if f == "write":
        if _eq(v, c):
            return (v, c, pos)
        return "expected value " + _str(c) + " attempting to write " + _str(v) + " instead"
    if f == "read-init":
        if _eq(0, counter) and not _eq(0, v):
            return "expected init value 0, read " + _str(v)
        if v is None or _eq(value, v):
            return (value, counter, pos)
        return "can't read " + _str(v) + " from register " + _str(value)
    if f == "read":
        if v is None or _eq(value, v):
            return (value, counter, pos)
        return "can't read " + _str(v) + " from register " + _str(value)
    raise NoMatchingClause(f)


def clj_check(history):
    """The reference's result map; raises NoMatchingClause where it throws."""
    s = (0, 0, None)
    for op in history:
        if op.get("type") != "ok":
            continue
        s = clj_step(s, op)
        if isinstance(s, str):
            return {"valid?": False, "error": s}
    return {"valid?": True, "model": CausalRegister(*s)}


def clj_verdict(history):
    """True / False / "unknown" (what check-safe makes of the exception)."""
    try:
        return clj_check(history)["valid?"]
    except NoMatchingClause:
        return "unknown"


# -- the closed form over Columns ----------------------------------------------------
def ref_cols(cols):
    """What jh_check_causal returns for these Columns: rc, the raw fields and
    `keys` (A.CAUSAL_KEY_DTYPE, max(n_keys, 1) records)."""
    n = int(cols.n)
    keyed = cols.key is not None and cols.n_keys > 0
    K = int(cols.n_keys) if keyed else 1
    keys = np.zeros(max(int(cols.n_keys), 1), A.CAUSAL_KEY_DTYPE)
    keys["valid"], keys["row"], keys["last_pos"] = A.VALID, -1, A.NIL
    out = {"rc": A.JH_OK, "valid": A.VALID, "cause": 0, "ok_count": 0, "invalid_keys": 0, "unknown_keys": 0,
           "first_event_row": -1, "keys": keys}
    aux = np.asarray(cols.aux) if cols.aux is not None else np.zeros(0, np.int64)
    if len(aux) != 2 * n:
        return dict(out, rc=A.JH_EINVAL)
    if n == 0:
        return out
    typ, f, val, proc = (np.asarray(x) for x in (cols.type, cols.f, cols.value, cols.process))
    sel = typ == A.TYPE_OK
    if keyed:
        key = np.asarray(cols.key)
        if (sel & (key >= K)).any():
            return dict(out, rc=A.JH_EINVAL)
        if (sel & (key < 0) & (proc >= 0)).any():
            return dict(out, rc=A.JH_EUNSUPPORTED)
        sel = sel & (key >= 0)
    else:
        key = np.zeros(n, np.int64)
    rows = np.nonzero(sel)[0]
    M = len(rows)
    out["ok_count"] = M
    if M == 0:
        return out
    sr = rows[np.argsort(key[rows], kind="stable")]                 # the sorted slots
    sk = key[sr]
    isw = f[sr] == A.F_WRITE
    S = np.concatenate([[0], np.cumsum(isw)])
    off = np.searchsorted(sk, np.arange(K + 1))
    w = S[:-1] - S[off[sk]]
    v, pos, link = val[sr], aux[2 * sr], aux[2 * sr + 1]
    head = np.concatenate([[True], sk[1:] != sk[:-1]])
    prev = np.where(head, A.NIL, np.concatenate([[A.NIL], pos[:-1]]))
    fs = f[sr]
    kind = np.full(M, 5, np.int64)
    kind[fs == A.F_WRITE] = np.where(v == w + 1, 0, 2)[fs == A.F_WRITE]
    bad_ri = ((w == 0) & (v != 0)) | ((v != A.NIL) & (v != w))
    kind[fs == A.F_READ_INIT] = np.where(bad_ri, 3, 0)[fs == A.F_READ_INIT]
    kind[fs == A.F_READ] = np.where((v != A.NIL) & (v != w), 4, 0)[fs == A.F_READ]
    kind[(link != A.CAUSAL_INIT) & (link != prev)] = 1
    first = np.full(K, M, np.int64)
    ev = np.nonzero(kind)[0]
    np.minimum.at(first, sk[ev], ev)
    for k in range(K):
        b, e, i = int(off[k]), int(off[k + 1]), int(first[k])
        if i < M:
            keys[k] = (A.UNKNOWN if kind[i] == 5 else A.INVALID, kind[i], sr[i], S[i] - S[b], pos[i - 1] if i > b else A.NIL)
        elif e > b:
            keys[k] = (A.VALID, 0, -1, S[e] - S[b], pos[e - 1])
    out["invalid_keys"] = int((keys["valid"][:K] == A.INVALID).sum())
    out["unknown_keys"] = int((keys["valid"][:K] == A.UNKNOWN).sum())
    hit = keys["row"][:K][keys["row"][:K] >= 0]
    out["first_event_row"] = int(hit.min()) if len(hit) else -1
    out["valid"] = A.INVALID if out["invalid_keys"] else A.UNKNOWN if out["unknown_keys"] else A.VALID
    out["cause"] = A.CAUSE_BAD_F if out["unknown_keys"] else 0
    return out


class FakeCtx:
    """_native.Context.check_causal, answered by ref_cols."""

    def __init__(self):
        self.calls = 0

    def check_causal(self, cols, on_device=False, keys=True):
        self.calls += 1
        r = ref_cols(cols)
        if r["rc"] != A.JH_OK:
            raise _native.JhError(r["rc"], "ref_cols")
        r = {k: v for k, v in r.items() if k != "rc"}
        if not keys:
            r["keys"] = None
        return r
