"""A deliberately naive restatement of monotonic-key-graph
(jepsen/src/jepsen/tests/cycle.clj:238-267), the reference of the monotonic-key
tests: per key a dict of value -> rows, the values sorted (nil first), nested
loops over successive groups. `links` gives one (a, b) per link call;
`ref_check_mono` what jh_check_cycle must return with JH_CY_MONOTONIC in the
mask (the process and realtime graphs come from tests/cycle_ref.py). Nothing
here shares code with jepsen_amd.cycle."""
from jepsen_amd import _abi as A
import cycle_ref as R


def links(history):
    """[(a, b), ...] over positions in `history`: one per link call, repeats kept."""
    oks = [i for i, op in enumerate(history) if op["type"] == "ok"]
    keys = []
    for i in oks:
        for k in (history[i].get("value") or {}):
            if k not in keys:
                keys.append(k)
    out = []
    for k in keys:
        index = {}
        for i in oks:
            v = history[i].get("value") or {}
            if k in v:
                index.setdefault(v[k], []).append(i)
        values = sorted(index, key=lambda v: (v is not None, 0 if v is None else v))
        for v1, v2 in zip(values, values[1:]):
            for a in index[v1]:
                for b in index[v2]:
                    out.append((a, b))
    return out


def graph(history):
    g = {}
    for a, b in links(history):
        R.link(g, a, b)
    return g


def ref_check_mono(history, analyzers, extra=()):
    """What jh_check_cycle must return for the op maps `history`: rows are
    positions in `history`, the :nemesis rows are removed first."""
    rows = [i for i, op in enumerate(history) if op.get("process") != "nemesis"]
    h = [history[i] for i in rows]
    out = {"valid": A.UNKNOWN, "cause": 0, "unknown_row": -1,
           "entries": sum(len(op.get("value") or {}) for op in h if op["type"] == "ok") if analyzers & A.CY_MONOTONIC else 0}
    edges, counts = [], [0, 0, 0, len(extra)]
    try:
        for bit, slot, fn in ((A.CY_REALTIME, 1, R.realtime_graph), (A.CY_PROCESS, 0, R.process_graph)):
            if analyzers & bit:
                es = [(rows[a], rows[b]) for a, succ in fn(h).items() for b in succ]
                counts[slot] = len(es)
                edges += es
    except R.RefUnknown as e:
        out.update(cause=e.cause, unknown_row=rows[e.row])
        return out
    if analyzers & A.CY_MONOTONIC:
        es = [(rows[a], rows[b]) for a, b in links(h)]
        counts[2] = len(es)
        edges += es
    edges += [tuple(e) for e in extra]
    out.update(R.scc_answer(len(history), edges))
    out.update(edges=set(edges), edge_count=counts)
    return out
