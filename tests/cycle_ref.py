"""Literal transcriptions of jepsen/src/jepsen/tests/cycle.clj and
txn/src/jepsen/txn.clj, the references of the cycle tests: the realtime loop
with its `oks` buffer (cycle.clj:315-377) over knossos' pair-index,
process-order (:271-300), ext-reads / ext-writes (txn.clj:5-28), ext-index
(:703-719), wr-graph (:736-779) and an iterative Tarjan. Graphs are
{position: set of positions} over the history they are given; `ref_check` runs
the checker (:911-934) over rows and gives what jh_check_cycle must return.
Nothing here shares code with jepsen_amd.cycle."""
from jepsen_amd import _abi as A


class RefUnknown(Exception):
    def __init__(self, cause, row, **kw):
        super().__init__(f"{cause} at {row}")
        self.cause, self.row, self.kw = cause, row, kw


def link(g, a, b):
    assert a is not None
    if b is None:                                  # (assert (not (nil? succ)))
        raise AssertionError("succ is nil")
    g.setdefault(a, set()).add(b)
    g.setdefault(b, set())


def pair_index(history):
    pairs, invokes = {}, {}
    for i, op in enumerate(history):
        t, p = op["type"], op.get("process")
        if t == "invoke":
            if p in invokes:
                raise RefUnknown(A.CAUSE_DOUBLE_INVOKE, i)
            invokes[p] = i
        elif t == "info":
            if p in invokes:
                j = invokes.pop(p)
                pairs[j], pairs[i] = i, j
            else:
                pairs[i] = None
        else:
            if p not in invokes:
                raise RefUnknown(A.CAUSE_ORPHAN, i)
            j = invokes.pop(p)
            pairs[j], pairs[i] = i, j
    return pairs


def realtime_graph(history):
    pairs = pair_index(history)
    oks, g = set(), {}
    for i, op in enumerate(history):
        t = op["type"]
        if t == "invoke":
            c = pairs.get(i)
            for ok in sorted(oks):
                try:
                    link(g, ok, c)
                except AssertionError:
                    raise RefUnknown(A.CAUSE_UNMATCHED_INVOKE, i)
        elif t == "ok":
            implied = {a for a, succ in g.items() if i in succ}      # (in g op)
            oks = (oks - implied) | {i}
    return g


def process_order(history, oks, process):
    g = {}
    mine = [i for i in oks if history[i].get("process") == process]
    for a, b in zip(mine, mine[1:]):
        link(g, a, b)
    return g


def process_graph(history):
    oks = [i for i, op in enumerate(history) if op["type"] == "ok"]
    g, seen = {}, []
    for i in oks:
        p = history[i].get("process")
        if p not in seen:
            seen.append(p)
            for a, succ in process_order(history, oks, p).items():
                g.setdefault(a, set()).update(succ)
    return g


def ext_reads(txn):
    ext, ignore = {}, set()
    for f, k, v in (txn or []):
        if not (f == "w" or k in ignore):
            ext[k] = v
        ignore.add(k)
    return ext


def ext_writes(txn):
    ext = {}
    for f, k, v in (txn or []):
        if f != "r":
            ext[k] = v
    return ext


def ext_index(ext_fn, history):
    idx = {}
    for i, op in enumerate(history):
        if op["type"] == "ok":
            for k, v in ext_fn(op.get("value")).items():
                idx.setdefault(k, {}).setdefault(v, []).insert(0, i)      # conj on a list
    return idx


def wr_graph(history, links=None):
    """links (a list): receives the number of link calls, one per external read
    with exactly one writer (the device counts those, repeats included)."""
    writes, reads = ext_index(ext_writes, history), ext_index(ext_reads, history)
    g, bad, n_links = {}, {}, 0
    for k, by_value in reads.items():
        for v, readers in by_value.items():
            w = writes.get(k, {}).get(v, [])
            if len(w) == 1:
                for r in readers:
                    link(g, w[0], r)
                    n_links += 1
            elif len(w) > 1:
                bad[(k, v)] = (min(readers), sorted(w)[:2])
    if bad:
        # the reference throws at the first pair its map order reaches; the device names
        # the smallest reader row and that row's first such pair in micro-op order
        row = min(b[0] for b in bad.values())
        for k, v in ext_reads(history[row].get("value")).items():
            if (k, v) in bad:
                raise RefUnknown(A.CAUSE_MULTIPLE_WRITES, row, key=k, value=v, rows=bad[(k, v)][1])
    if links is not None:
        links.append(n_links)
    return g


def tarjan(n, edges):
    """labels[v] = the smallest vertex of v's SCC of more than one vertex, else
    -1 (iterative Tarjan over the whole graph)."""
    succ = [[] for _ in range(n)]
    for a, b in edges:
        succ[a].append(b)
    labels = [-1] * n
    index, low, on, stack, counter = {}, {}, set(), [], [0]
    for root in range(n):
        if root in index:
            continue
        work = [(root, iter(succ[root]))]
        index[root] = low[root] = counter[0]
        counter[0] += 1
        stack.append(root)
        on.add(root)
        while work:
            v, it = work[-1]
            advanced = False
            for w in it:
                if w not in index:
                    index[w] = low[w] = counter[0]
                    counter[0] += 1
                    stack.append(w)
                    on.add(w)
                    work.append((w, iter(succ[w])))
                    advanced = True
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            if advanced:
                continue
            work.pop()
            if work:
                low[work[-1][0]] = min(low[work[-1][0]], low[v])
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on.discard(w)
                    comp.append(w)
                    if w == v:
                        break
                if len(comp) > 1:
                    for w in comp:
                        labels[w] = min(comp)
    return labels


def sccs_of(labels):
    groups = {}
    for v, l in enumerate(labels):
        if l >= 0:
            groups.setdefault(l, []).append(v)
    return sorted(groups.values(), key=lambda g: (len(g), g[0]))


def count_back(edges):
    return sum(1 for a, b in edges if b < a)


def scc_answer(n, edges):
    labels = tarjan(n, edges)
    sccs = sccs_of(labels)
    return {"labels": labels, "sccs": sccs, "scc_count": len(sccs), "scc_vertices": sum(map(len, sccs)),
            "back_edges": count_back(edges), "valid": A.INVALID if sccs else A.VALID}


def ref_check(history, analyzers, extra=()):
    """What jh_check_cycle must return for the op maps `history`: rows are
    positions in `history`, the :nemesis rows are removed first."""
    rows = [i for i, op in enumerate(history) if op.get("process") != "nemesis"]
    h = [history[i] for i in rows]
    out = {"valid": A.UNKNOWN, "cause": 0, "unknown_row": -1, "unknown_key": None, "unknown_value": None,
           "unknown_rows": [-1, -1]}
    edges, counts = [], [0, 0, 0, len(extra)]
    try:
        for bit, slot, fn in ((A.CY_REALTIME, 1, realtime_graph), (A.CY_PROCESS, 0, process_graph), (A.CY_WR, 2, wr_graph)):
            if analyzers & bit:
                links = []
                g = fn(h, links) if fn is wr_graph else fn(h)
                es = [(rows[a], rows[b]) for a, succ in g.items() for b in succ]
                counts[slot] = links[0] if links else len(es)
                edges += es
    except RefUnknown as e:
        out.update(cause=e.cause, unknown_row=rows[e.row])
        if e.kw:
            out.update(unknown_key=e.kw["key"], unknown_value=e.kw["value"], unknown_rows=[rows[r] for r in e.kw["rows"]])
        return out
    edges += [tuple(e) for e in extra]
    out.update(scc_answer(len(history), edges))
    out.update(edges=set(edges), edge_count=counts)
    return out
