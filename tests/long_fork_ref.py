"""Two CPU restatements of jepsen.tests.long-fork/checker
(jepsen/src/jepsen/tests/long_fork.clj:158-324), independent of
jepsen_amd/long_fork.py and of the device's counter test:

  ref_ops(n, history)   brute force on op dicts: every pair of reads of a
                        group, read-compare as written
  ref_cols(cols, n)     numpy on the columns, yielding the raw result in the
                        shape of jh_long_fork_result (plus every fork pair)
"""
import numpy as np

from jepsen_amd import _abi as A

NIL = A.NIL


class Illegal(Exception):
    def __init__(self, kind, row=None):
        super().__init__(f"illegal-history kind {kind} row {row}")
        self.kind, self.row = kind, row


def read_compare(a, b):
    """long_fork.clj:158-196, as written."""
    if len(a) != len(b):
        raise Illegal(1)
    res = 0
    for k in a:
        if k not in b:
            raise Illegal(1)
        va, vb = a[k], b[k]
        if va == vb:
            pass
        elif vb is None:
            if res > 0:
                return None
            res = -1
        elif va is None:
            if res < 0:
                return None
            res = 1
        else:
            raise Illegal(2)
    return res


def _txn(op):
    v = op.get("value")
    return [] if v is None else v


def _is_read(op):
    v = op.get("value")
    return (v is None or isinstance(v, (list, tuple))) and all(m[0] == "r" for m in _txn(op))


def _is_write(op):
    v = op.get("value")
    return isinstance(v, (list, tuple)) and len(v) == 1 and v[0][0] == "w"


def ref_ops(n, history):
    """The checker's map; forks as [row_a, row_b] with row_a < row_b, ordered
    by group (ascending keys) then rows. Raises Illegal."""
    rs = [(i, op) for i, op in enumerate(history) if op["type"] == "ok" and _is_read(op)]
    out = {"reads-count": len(rs),
           "early-read-count": sum(1 for _, op in rs if all(m[2] is None for m in _txn(op))),
           "late-read-count": sum(1 for _, op in rs if all(m[2] is not None for m in _txn(op)))}
    seen = set()
    for op in history:
        if op["type"] == "invoke" and _is_write(op):
            k = op["value"][0][1]
            if k in seen:
                return dict(out, **{"valid?": "unknown", "error": ["multiple-writes", k]})
            seen.add(k)
    by = {}
    for i, op in rs:
        by.setdefault(frozenset(m[1] for m in _txn(op)), []).append((i, {m[1]: m[2] for m in _txn(op)}))
    wrong = [g[0][0] for ks, g in by.items() if len(ks) != n]
    if wrong:
        raise Illegal(1, min(wrong))
    forks = []
    for ks in sorted(by, key=sorted):
        g = by[ks]
        for x in range(len(g)):
            for y in range(x + 1, len(g)):
                if read_compare(g[x][1], g[y][1]) is None:
                    forks.append([g[x][0], g[y][0]])
    if forks:
        return dict(out, **{"valid?": False, "forks": forks})
    return dict(out, **{"valid?": True})


def strip(result):
    """A checker result with its fork op maps replaced by their rows."""
    r = dict(result)
    if "forks" in r:
        r["forks"] = [[a["index"], b["index"]] for a, b in r["forks"]]
    return r


def ref_cols(cols, n):
    """The raw result. "rc": JH_OK / JH_EINVAL / JH_EUNSUPPORTED (nothing else
    is filled then); "forks": every pair, in the C entry point's order."""
    typ, f, v, v2 = (np.asarray(getattr(cols, k)) for k in ("type", "f", "value", "value2"))
    aux = np.asarray(cols.aux if cols.aux is not None else np.zeros(0, np.int64))
    if len(aux) % 2 or n < 1:
        return {"rc": A.JH_EINVAL}
    if n > 64:
        return {"rc": A.JH_EUNSUPPORTED}
    half = len(aux) // 2
    out = {"rc": A.JH_OK, "valid": A.VALID, "cause": 0, "illegal_kind": 0, "illegal_row": -1, "multiple_key": NIL,
           "multiple_row": -1, "fork_groups": 0, "fork_count": 0, "forks": np.zeros((0, 2), np.int64),
           "reads_count": 0, "early_count": 0, "late_count": 0, "entries": 0}
    rows = np.nonzero((typ == A.TYPE_OK) & (f == A.F_READ))[0]
    start, cnt = v[rows].copy(), v2[rows].copy()
    nilv = (start == NIL) & (cnt == 0)
    start[nilv] = 0
    if ((start < 0) | (cnt < 0) | (start > half) | (cnt > half - start)).any():
        return {"rc": A.JH_EINVAL}
    R = len(rows)
    rid = np.repeat(np.arange(R), cnt)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if R else np.zeros(0, np.int64)
    at = start[rid] + (np.arange(len(rid)) - first[rid])
    keys, vals = aux[2 * at], aux[2 * at + 1]
    nn = np.bincount(rid[vals != NIL], minlength=R) if R else np.zeros(0, np.int64)
    out.update(reads_count=R, early_count=int((nn == 0).sum()), late_count=int((nn == cnt).sum()),
               entries=int(cnt.sum()))
    sized = cnt[rid] == n
    g, bit = keys // n, keys % n                                # floored, as Clojure's quot-by-mod / mod
    if sized.any():
        r_s, g_s, b_s = rid[sized], g[sized], bit[sized]
        g0 = np.zeros(R, np.int64)
        g0[r_s[::-1]] = g_s[::-1]                               # the group of each read's first key
        pos = np.zeros(R, np.uint64)
        np.bitwise_or.at(pos, r_s, np.uint64(1) << b_s.astype(np.uint64))
        full = np.uint64((1 << n) - 1)
        if (g_s != g0[r_s]).any() or (pos[cnt == n] != full).any():
            return {"rc": A.JH_EUNSUPPORTED}
    w = np.nonzero((typ == A.TYPE_INVOKE) & (f == A.F_WRITE))[0]
    if len(w):
        _, firsts = np.unique(v[w], return_index=True)
        rep = np.setdiff1d(np.arange(len(w)), firsts)
        if len(rep):
            row = int(w[rep.min()])
            out.update(valid=A.UNKNOWN, cause=A.CAUSE_MULTIPLE_WRITES, multiple_key=int(v[row]), multiple_row=row)
            return out
    if (cnt != n).any():
        out.update(valid=A.UNKNOWN, cause=A.CAUSE_ILLEGAL_HISTORY, illegal_kind=1,
                   illegal_row=int(rows[cnt != n].min()))
        return out
    if R == 0:
        return out
    # every read has n pairs of one aligned group
    grp = g.reshape(R, n)[:, 0]
    seen = np.zeros(R, np.uint64)
    live = vals != NIL
    np.bitwise_or.at(seen, rid[live], np.uint64(1) << bit[live].astype(np.uint64))
    # two distinct non-nil values for one (group, key)
    order = np.lexsort((vals[live], keys[live]))
    ks, vs, rr = keys[live][order], vals[live][order], rows[rid[live][order]]
    clash = (ks[1:] == ks[:-1]) & (vs[1:] != vs[:-1])
    if clash.any():
        bad = np.isin(ks, ks[1:][clash])
        out.update(valid=A.UNKNOWN, cause=A.CAUSE_ILLEGAL_HISTORY, illegal_kind=2, illegal_row=int(rr[bad].min()))
        return out
    forks, groups = [], 0
    order = np.argsort(grp, kind="stable")
    gs = grp[order]
    cuts = np.nonzero(np.concatenate([[True], gs[1:] != gs[:-1], [True]]))[0]
    for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
        if b - a < 2:
            continue
        m = seen[order[a:b]]
        if (m == m[0]).all():
            continue
        x, y = m[:, None], m[None, :]
        inc = np.triu(((x & ~y) != 0) & ((y & ~x) != 0), 1)
        ia, ib = np.nonzero(inc)
        if len(ia):
            groups += 1
            r = rows[order[a:b]]
            forks.append(np.stack([r[ia], r[ib]], axis=1))
    if forks:
        fk = np.concatenate(forks).astype(np.int64)
        out.update(valid=A.INVALID, fork_groups=groups, fork_count=len(fk), forks=fk)
    return out


RAW_FIELDS = ("valid", "cause", "illegal_kind", "illegal_row", "multiple_key", "multiple_row", "fork_groups",
              "fork_count", "reads_count", "early_count", "late_count", "entries")


def raw_of_map(result_or_exc, history):
    """A ref_ops answer (map, or Illegal) in ref_cols' shape, for comparing the
    two restatements; entries is not derived."""
    base = {"valid": A.VALID, "cause": 0, "illegal_kind": 0, "illegal_row": -1, "multiple_key": NIL,
            "multiple_row": -1, "fork_groups": 0, "fork_count": 0, "forks": []}
    if isinstance(result_or_exc, Illegal):
        return dict(base, valid=A.UNKNOWN, cause=A.CAUSE_ILLEGAL_HISTORY, illegal_kind=result_or_exc.kind,
                    illegal_row=result_or_exc.row)
    r = result_or_exc
    base.update(reads_count=r["reads-count"], early_count=r["early-read-count"], late_count=r["late-read-count"])
    if r["valid?"] == "unknown":
        k = r["error"][1]
        seen = set()
        for i, op in enumerate(history):
            if op["type"] == "invoke" and _is_write(op):
                if op["value"][0][1] in seen:
                    return dict(base, valid=A.UNKNOWN, cause=A.CAUSE_MULTIPLE_WRITES, multiple_key=k, multiple_row=i)
                seen.add(op["value"][0][1])
    if r["valid?"] is False:
        fk = r["forks"]
        return dict(base, valid=A.INVALID, fork_count=len(fk), forks=[list(p) for p in fk])
    return base
