"""A numpy closed form of jh_perf's four outputs (include/jh.h), written from
the header's text and independent of jepsen_amd/perf.py. Everything is integer
but the bucket, which is the reference's two double divisions:
numpy's int64 -> float64 conversion and `/` are IEEE, correctly rounded."""
import numpy as np

from jepsen_amd import _abi as A

SCALARS = ("n_invokes", "n_paired", "n_unpaired_invokes", "first_unpaired_invoke", "t_max",
           "n_series", "n_groups", "n_cells", "has_quantiles")
LISTS = ("pair", "pt_row", "series", "groups", "cells")
MAX_F = 1 << 20


def bucket(t, dt):
    return ((np.asarray(t, np.int64).astype(np.float64) / 1e9) / float(dt)).astype(np.int64)


def pick_index(count, q):
    """min(count - 1, (long)floor(count * q)), one rounded double multiply."""
    return min(count - 1, int(np.floor(np.float64(count) * np.float64(q))))


def ref_cols(cols, time, f_count=None, dt_quantiles=0, dt_rate=0, want=A.PERF_ALL):
    n = int(cols.n)
    want = int(want) or A.PERF_ALL
    if f_count is None:
        f_count = A.F_FIRST_INTERNED + len(cols.f_names or [])
    dtq, dtr = dt_quantiles or A.PERF_DT_QUANTILES, dt_rate or A.PERF_DT_RATE
    e = np.zeros(0, np.int64)
    out = {k: 0 for k in SCALARS}
    out.update(rc=A.JH_OK, first_unpaired_invoke=-1, pair=e, pt_row=e, series=e.reshape(0, 3),
               groups=e.reshape(0, 7), cells=e.reshape(0, 4))
    if n == 0:
        return out
    proc, typ, f = (np.asarray(x, np.int64)[:n] for x in (cols.process, cols.type, cols.f))
    t = np.asarray(time, np.int64)[:n]
    if f_count > MAX_F or (t < 0).any() or (f < 0).any() or (f >= f_count).any():
        out["rc"] = A.JH_EUNSUPPORTED
        return out
    out["t_max"] = int(max(0, t.max()))
    inv = typ == A.TYPE_INVOKE
    pair = np.full(n, -1, np.int64)
    if want & (A.PERF_PAIR | A.PERF_POINTS | A.PERF_QUANTILES):
        order = np.argsort(proc, kind="stable")
        ps, isinv = proc[order], inv[order]
        hit = np.nonzero((ps[1:] == ps[:-1]) & isinv[:-1] & ~isinv[1:])[0]     # slot i an invoke, slot i + 1 its completion
        pair[order[hit]] = order[hit + 1]
        pair[order[hit + 1]] = order[hit]
        unp = np.nonzero(inv & (pair < 0))[0]
        out.update(n_invokes=int(inv.sum()), n_paired=len(hit), n_unpaired_invokes=len(unp),
                   first_unpaired_invoke=int(unp[0]) if len(unp) else -1)
        if want & A.PERF_PAIR:
            out["pair"] = pair
    if want & A.PERF_POINTS:
        rows = np.nonzero(inv & (pair >= 0))[0]
        place = np.zeros(4, np.int64)
        place[list(A.PERF_TYPE_ORDER)] = np.arange(3)
        key = f[rows] * 3 + place[typ[pair[rows]]]
        o = np.argsort(key, kind="stable")
        out["pt_row"] = rows[o]
        ks, cnt = np.unique(key, return_counts=True)
        out["series"] = np.stack([ks // 3, np.asarray(A.PERF_TYPE_ORDER)[ks % 3], cnt], axis=1).reshape(-1, 3)
        out["n_series"] = len(ks)
    if (want & A.PERF_QUANTILES) and out["n_unpaired_invokes"] == 0:
        out["has_quantiles"] = 1
        rows = np.nonzero(inv)[0]
        lat = t[pair[rows]] - t[rows]
        b = bucket(t[rows], dtq)
        o = np.lexsort((lat, b, f[rows]))
        fs, bs, ls = f[rows][o], b[o], lat[o]
        head = np.nonzero(np.concatenate(([True], (fs[1:] != fs[:-1]) | (bs[1:] != bs[:-1]))))[0] if len(rows) else e
        end = np.concatenate((head[1:], [len(rows)])) if len(rows) else e
        recs = []
        for s, x in zip(head.tolist(), end.tolist()):
            c = x - s
            recs.append([fs[s], bs[s], c] + [ls[s + pick_index(c, q)] for q in A.PERF_QS])
        out["groups"] = np.asarray(recs, np.int64).reshape(-1, 7)
        out["n_groups"] = len(recs)
    if want & A.PERF_RATE:
        rows = np.nonzero(~inv & (proc >= 0))[0]
        trip = np.stack([f[rows], typ[rows], bucket(t[rows], dtr)], axis=1).reshape(-1, 3)
        u, cnt = np.unique(trip, axis=0, return_counts=True) if len(rows) else (trip, e)
        out["cells"] = np.concatenate([u, cnt.reshape(-1, 1)], axis=1).astype(np.int64).reshape(-1, 4)
        out["n_cells"] = len(u)
    return out
