"""A literal transcription of appends-and-reads-graph and its verification
passes, jepsen/src/jepsen/tests/cycle.clj:381-699, the reference of the
list-append tests: dicts and sets, the reduce-mops order, sort-by count. A read
value is a list or None; inside sets it stands as a tuple (None stays None, so
nil and [] are two values, as in Clojure). Where the reference's order is that
of a hash set (sort-by count over equal lengths, the order of :errors across
keys) this file keeps first-appearance order.

`ref_check_append` runs the checker (:911-934) over rows and gives what
jh_check_cycle must return with JH_CY_APPEND. Nothing here shares code with
jepsen_amd.cycle; process / realtime graphs and Tarjan come from cycle_ref."""
from jepsen_amd import _abi as A
import cycle_ref as R


class Thrown(Exception):
    """throw+ of a map with :valid? (the checker returns it), or a failed
    assert (m is None). at = (position in the history given, micro-op index)."""

    def __init__(self, m, at, **kw):
        super().__init__(repr(m))
        self.m, self.at, self.kw = m, at, kw


def frozen(v):
    return None if v is None else tuple(v)


def count(v):
    return 0 if v is None else len(v)


def reduce_mops(f, state, history):
    for i, op in enumerate(history):
        for j, mop in enumerate(op.get("value") or ()):
            state = f(state, (i, j), op, mop)
    return state


def verify_mop_types(history):
    bad = [op for op in history if not all(mop[0] in ("r", "append") for mop in (op.get("value") or ()))]
    if bad:
        raise Thrown({"valid?": "unknown", "type": "unexpected-txn-micro-op-types",
                      "message": "history contained operations other than appends or reads", "examples": bad[:8]}, None)


def verify_unique_appends(history):
    def step(written, at, op, mop):
        f, k, v = mop
        if op["type"] == "invoke" and f == "append":
            writes_of_k = written.get(k, set())
            if v in writes_of_k:
                raise Thrown({"valid?": "unknown", "type": "duplicate-appends", "op": op, "key": k, "value": v,
                              "message": f"value {v} appended to key {pr(k)} multiple times!"}, at)
            written[k] = writes_of_k | {v}
        return written
    reduce_mops(step, {}, history)


def pr(k):
    return ":" + k if isinstance(k, str) else repr(k)


def prefix(a, b):
    a, b = a or (), b or ()
    return len(a) <= len(b) and all(x == y for x, y in zip(a, b))


def sorted_values(history):
    states = {}
    for op in history:
        for f, k, v in (op.get("value") or ()):
            if f == "r":
                states.setdefault(k, {}).setdefault(frozen(v), None)          # a set, in first-appearance order
    return {k: sorted(vs, key=count) for k, vs in states.items()}             # sort-by count (stable)


def verify_total_order(sv):
    errors = []
    for k, values in sv.items():
        for a, b in zip(values, values[1:]):
            if not prefix(a, b):
                errors.append({"key": k, "values": [thaw(a), thaw(b)]})
                break
    if errors:
        raise Thrown({"valid?": False, "type": "no-total-state-order",
                      "message": "observed mutually incompatible orders of appends", "errors": errors}, None)


def thaw(v):
    return None if v is None else list(v)


def verify_no_dups(history):
    def step(_, at, op, mop):
        f, k, v = mop
        if f == "r":
            freq = {}
            for x in (v or ()):
                freq[x] = freq.get(x, 0) + 1
            dups = {x: c for x, c in sorted(freq.items()) if c > 1}
            if dups:
                raise Thrown({"valid?": False, "type": "duplicate-elements",
                              "message": "Observed multiple copies of a value which was only inserted once",
                              "op": op, "key": k, "value": v, "duplicates": dups}, at)
        return None
    reduce_mops(step, None, history)


def append_index(sv):
    out = {}
    for k, values in sv.items():
        vs = values[-1] or ()
        out[k] = {"values": vs, "indices": {v: i for i, v in enumerate(vs)}}
    return out


def write_index(history, pos):
    index = {}
    for i, op in zip(pos, history):
        for f, k, v in (op.get("value") or ()):
            if f == "append":
                index.setdefault(k, {})[v] = i
    return index


INIT = ("::init",)


def read_index(history, pos):
    index = {}
    for i, op in zip(pos, history):
        for f, k, v in (op.get("value") or ()):
            if f == "r":
                index.setdefault(k, {}).setdefault(v[-1] if v else INIT, []).insert(0, i)      # conj on a list
    return index


def graph(history, links=None):
    """[graph over positions in `history`, number of link calls]; raises Thrown."""
    verify_mop_types(history)
    verify_unique_appends(history)
    verify_no_dups(history)
    pos = [i for i, op in enumerate(history) if op["type"] in ("ok", "info")]
    h = [history[i] for i in pos]
    sv = sorted_values(h)
    verify_total_order(sv)
    ai, wi, ri = append_index(sv), write_index(h, pos), read_index(h, pos)
    g, n_links = {}, 0
    for i, op in zip(pos, h):
        for j, (f, k, v) in enumerate(op.get("value") or ()):
            if f == "r":
                if v:
                    w = wi.get(k, {}).get(v[-1])
                    if w is None:                                 # (assert append-op)
                        raise Thrown(None, (i, j), key=k, value=v[-1])
                    if w != i:
                        R.link(g, w, i)
                        n_links += 1
            else:
                index = ai.get(k, {}).get("indices", {}).get(v)
                if index is None:
                    continue
                prev_v = ai[k]["values"][index - 1] if index > 0 else INIT
                prev_append = wi.get(k, {}).get(prev_v) if index > 0 else None
                if index > 0 and prev_append != i:
                    if prev_append is None:                       # link's (assert (not (nil? a)))
                        raise Thrown(None, (i, j), key=k, value=prev_v)
                    R.link(g, prev_append, i)
                    n_links += 1
                for r in ri.get(k, {}).get(prev_v, ()):
                    if r != i:
                        R.link(g, r, i)
                        n_links += 1
    if links is not None:
        links.append(n_links)
    return g


def intern_keys(history):
    """The dense key ids of the encoding: first appearance over the non-nemesis rows."""
    ids = {}
    for op in history:
        if op.get("process") != "nemesis":
            for mop in (op.get("value") or ()):
                ids.setdefault(mop[1], len(ids))
    return ids


def first_repeat(v):
    seen = set()
    for x in v:
        if x in seen:
            return x
        seen.add(x)


def total_order_fields(h, rows, ids):
    """Cause 15's fields from their definition: per key the longest :ok / :info
    read (the first of that length); the bad keys; the smallest bad key id and
    its smallest row with a read that is no prefix of the longest."""
    longest, bad = {}, {}
    counted = [(rows[i], op) for i, op in enumerate(h) if op["type"] in ("ok", "info")]
    for _, op in counted:
        for f, k, v in (op.get("value") or ()):
            if f == "r" and (k not in longest or count(v) > count(longest[k])):
                longest[k] = v
    for row, op in counted:
        for f, k, v in (op.get("value") or ()):
            if f == "r" and not prefix(v, longest[k]):
                bad.setdefault(k, row)
    key = min(bad, key=lambda k: ids[k])
    return key, bad[key], len(bad)


def ref_check_append(history, analyzers, extra=()):
    """What jh_check_cycle must return for the op maps `history` with
    JH_CY_APPEND in `analyzers`: rows are positions in `history`, the :nemesis
    rows are removed first. With a cause: valid, cause, unknown_row,
    unknown_rows, unknown_key (the key itself), unknown_value, and "map", what
    the checker returns (None for cause 16, an assert)."""
    rows = [i for i, op in enumerate(history) if op.get("process") != "nemesis"]
    h = [history[i] for i in rows]
    ids = intern_keys(history)
    out = {"valid": A.UNKNOWN, "cause": 0, "unknown_row": -1, "unknown_key": None, "unknown_value": None,
           "unknown_rows": [-1, -1], "map": None,
           "entries": sum(len(op.get("value") or ()) + sum(count(m[2]) for m in (op.get("value") or ()) if m[0] == "r") for op in h)}
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
    try:
        links = []
        edges += [(rows[a], rows[b]) for a, succ in graph(h, links).items() for b in succ]
        counts[2] = links[0]
    except Thrown as e:
        out["map"] = e.m
        if e.m is None:
            out.update(cause=A.CAUSE_NO_WRITER, unknown_row=rows[e.at[0]], unknown_rows=[e.at[1], -1],
                       unknown_key=e.kw["key"], unknown_value=e.kw["value"])
        elif e.m["type"] == "duplicate-appends":
            out.update(cause=A.CAUSE_DUPLICATE_APPENDS, unknown_row=rows[e.at[0]], unknown_rows=[e.at[1], -1],
                       unknown_key=e.m["key"], unknown_value=e.m["value"])
        elif e.m["type"] == "duplicate-elements":
            out.update(valid=A.INVALID, cause=A.CAUSE_DUPLICATE_ELEMENTS, unknown_row=rows[e.at[0]], unknown_rows=[e.at[1], -1],
                       unknown_key=e.m["key"], unknown_value=first_repeat(e.m["value"]))
        elif e.m["type"] == "no-total-state-order":
            key, row, n_bad = total_order_fields(h, rows, ids)
            assert n_bad == len(e.m["errors"]) and key in [x["key"] for x in e.m["errors"]]
            out.update(valid=A.INVALID, cause=A.CAUSE_NO_TOTAL_ORDER, unknown_row=row, unknown_rows=[n_bad, -1], unknown_key=key)
        else:
            raise
        return out
    edges += [tuple(e) for e in extra]
    out.update(R.scc_answer(len(history), edges))
    out.update(edges=set(edges), edge_count=counts)
    return out
