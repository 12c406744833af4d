"""jepsen.tests.cycle on MI355X: dependency graphs over completion ops, their
strongly connected components, and an explanation of each.

Mirrors jepsen/src/jepsen/tests/cycle.clj (names, argument meaning, result
maps). An analyzer is a function history -> (Graph, explainer); `combine` takes
the union; `checker(analyze_fn)` removes the :nemesis ops, analyzes, and reports
every SCC of more than one op as an anomaly:

    {"valid?": bool, "scc-count": int, "cycles": [[op, why, op, ..., op], ...]}

Vertices are positions in the history the analyzer was given (the checker gives
every op an "index" first, so they are history rows). The module's own analyzers
(process_graph, realtime_graph, wr_graph, appends_and_reads_graph,
monotonic_key_graph and their `combine`) carry a mask of JH_CY_* bits: a checker
over them makes ONE jh_check_cycle call when the values encode (include/jh.h,
"Cycle txns", "Append txns" and "Map reads encoding": keys are interned, values
and list elements must be longs) and runs the host implementation otherwise
(also for two of wr_graph, appends_and_reads_graph and monotonic_key_graph
combined, which the device refuses). The host implementation is the
numpy closed forms below; tests/cycle_ref.py holds the literal transcriptions
they are tested against. Explanations run on the host over the at most 8
reported SCCs.

Deviations: SCCs of equal size are ordered by their smallest
row (Bifurcan's order is unpinned); find_cycle starts at the SCC's smallest row
and follows successors in ascending row order (Bifurcan's first vertex is
unpinned); a Python str key or value prints as a keyword.
"""
import numpy as np

from . import _abi as A
from . import history as H

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
READ_FS, WRITE_FS = ("r", "read"), ("w", "write")
APPEND_F = "append"


class IllegalArgument(ValueError):
    """IllegalArgumentException: wr-graph's value written by more than one op."""


class IllegalHistory(AssertionError):
    """An assert of knossos' pair-index or of cycle/link failed."""

    def __init__(self, cause, row):
        super().__init__(f"{cause} at index {row}")
        self.cause, self.row = cause, row


# -- graphs -----------------------------------------------------------------------
class Graph:
    """A directed graph over 0..n-1 as an (E, 2) int64 edge array."""

    def __init__(self, n, edges=None):
        self.n = int(n)
        self.edges = np.zeros((0, 2), np.int64) if edges is None or len(edges) == 0 else \
            np.asarray(edges, np.int64).reshape(-1, 2)

    def out(self, v, within=None):
        e = self.edges
        succ = sorted(set(e[e[:, 0] == v, 1].tolist()))
        return [s for s in succ if within is None or s in within]

    def to_map(self):
        """{vertex: sorted successors} over every vertex that carries an edge."""
        m = {}
        for s, d in self.edges.tolist():
            m.setdefault(s, set()).add(d)
            m.setdefault(d, set())
        return {k: sorted(v) for k, v in sorted(m.items())}

    def union(self, other):
        return Graph(max(self.n, other.n), np.concatenate([self.edges, other.edges]))


def map_to_graph(m):
    """{node: successors} (cycle/map->bdigraph) -> Graph over 0..max node."""
    edges = [(int(a), int(b)) for a, succ in m.items() for b in succ]
    n = 1 + max([int(a) for a in m] + [b for _, b in edges], default=-1)
    return Graph(n, edges)


def _encode_rows(history):
    proc = np.empty(len(history), np.int64)
    typ = np.empty(len(history), np.int64)
    others = {"nemesis": -1}
    for i, op in enumerate(history):
        p = op.get("process")
        if H._is_int(p) and p >= 0:
            proc[i] = int(p)
        else:
            proc[i] = others.setdefault(p, -1 - len(others)) if p != "nemesis" else -1
        typ[i] = H.TYPES[op.get("type")]
    return proc, typ


# -- numpy closed forms -----------------------------------------------------------
def process_edges(proc, typ):
    """cycle.clj:271-300: each :ok row -> the next :ok row of its process."""
    ok = np.nonzero((typ == A.TYPE_OK) & (proc != -1))[0]
    o = ok[np.argsort(proc[ok], kind="stable")]
    same = proc[o[:-1]] == proc[o[1:]] if len(o) > 1 else np.zeros(0, bool)
    return np.stack([o[:-1][same], o[1:][same]], axis=1) if len(o) > 1 else np.zeros((0, 2), np.int64)


def pair_rows(proc, typ):
    """knossos' pair-index over the non-nemesis rows: comp[i] = the completion
    row of the invoke at i (-1: none). IllegalHistory for a double invoke or an
    :ok / :fail without an open invoke (an :info without one stays unpaired)."""
    n = len(proc)
    comp = np.full(n, -1, np.int64)
    rows = np.nonzero(proc != -1)[0]
    o = rows[np.argsort(proc[rows], kind="stable")]
    if len(o) == 0:
        return comp
    t, p = typ[o], proc[o]
    prev_inv = np.concatenate(([False], (p[1:] == p[:-1]) & (t[:-1] == A.TYPE_INVOKE)))
    dbl = o[(t == A.TYPE_INVOKE) & prev_inv]
    orphan = o[((t == A.TYPE_OK) | (t == A.TYPE_FAIL)) & ~prev_inv]
    if len(dbl):
        raise IllegalHistory("double-invoke", int(dbl.min()))
    if len(orphan):
        raise IllegalHistory("orphan-completion", int(orphan.min()))
    done = np.concatenate(((p[1:] == p[:-1]) & (t[:-1] == A.TYPE_INVOKE) & (t[1:] != A.TYPE_INVOKE), [False]))
    comp[o[done]] = o[np.nonzero(done)[0] + 1]
    return comp


def realtime_edges(proc, typ):
    """cycle.clj:315-377 in closed form: an :ok completion c links to the
    completion of every invoke in (c, R(c)), R(c) = the smallest completion row
    over the ops invoked after c that complete :ok (none: the end)."""
    n = len(proc)
    comp = pair_rows(proc, typ)
    inv = (typ == A.TYPE_INVOKE) & (proc != -1)
    oks = np.nonzero((typ == A.TYPE_OK) & (proc != -1))[0]
    if len(oks):
        bad = np.nonzero(inv & (comp < 0) & (np.arange(n) > oks[0]))[0]
        if len(bad):
            raise IllegalHistory("unmatched-invoke", int(bad[0]))
    key = np.full(n + 1, n, np.int64)
    has_ok = inv & (comp >= 0)
    has_ok[has_ok] = typ[comp[has_ok]] == A.TYPE_OK
    key[:n][has_ok] = comp[has_ok]
    suf = np.minimum.accumulate(key[::-1])[::-1]          # suf[i] = min key[i:]
    r = suf[oks + 1]
    ip = np.concatenate(([0], np.cumsum(inv)))             # invokes in rows < i
    cnt = ip[r] - ip[oks + 1]
    inv_comp = comp[inv]
    src = np.repeat(oks, cnt)
    first = np.repeat(ip[oks + 1], cnt)
    within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return np.stack([src, inv_comp[first + within]], axis=1) if len(src) else np.zeros((0, 2), np.int64)


def ext_reads(txn):
    """txn.clj:5-17: {k: v} of the values a txn observed and did not write."""
    ext, ignore = {}, set()
    for f, k, v in (txn or ()):
        if f not in WRITE_FS and k not in ignore:
            ext[k] = v
        ignore.add(k)
    return ext


def ext_writes(txn):
    """txn.clj:19-28: {k: v} of the final values a txn wrote."""
    ext = {}
    for f, k, v in (txn or ()):
        if f not in READ_FS:
            ext.pop(k, None)
            ext[k] = v
    return ext


def ext_index(ext_fn, history):
    """cycle.clj:703-719: {k: {v: [op, ...]}} over the :ok ops (each list newest
    first, as conj on a list builds it)."""
    idx = {}
    for op in history:
        if op.get("type") == "ok":
            for k, v in ext_fn(op.get("value")).items():
                idx.setdefault(k, {}).setdefault(v, []).insert(0, op)
    return idx


def wr_edges(history):
    """cycle.clj:736-779 over positions: writer -> every external reader of its
    (k, v). IllegalArgument when a read pair has two or more writers: the
    smallest reader row, its first such pair in micro-op order."""
    writers = {}
    for i, op in enumerate(history):
        if op.get("type") == "ok" and op.get("process") != "nemesis":
            for k, v in ext_writes(op.get("value")).items():
                writers.setdefault((k, v), []).append(i)
    edges = []
    for i, op in enumerate(history):
        if op.get("type") == "ok" and op.get("process") != "nemesis":
            for k, v in ext_reads(op.get("value")).items():
                w = writers.get((k, v), ())
                if len(w) > 1:
                    e = IllegalArgument(f"Key {pr_str(k)} had value {pr_str(v)} written by more than one op: "
                                        f"{[history[j] for j in w]!r}")
                    e.row, e.key, e.value, e.rows = i, k, v, w[:2]
                    raise e
                if w:
                    edges.append((w[0], i))
    return np.asarray(edges, np.int64).reshape(-1, 2)


def regions(n, edges):
    """The merged row intervals [dst, src] of the back edges (dst < src) as an
    (R, 2) array of [start, end], regions of two or more vertices only. Every
    SCC of more than one vertex lies inside one of them."""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    reach = np.arange(n, dtype=np.int64)
    back = edges[edges[:, 1] < edges[:, 0]]
    np.maximum.at(reach, back[:, 1], back[:, 0])
    mx = np.maximum.accumulate(reach) if n else reach
    start = np.ones(n, bool)
    start[1:] = mx[:-1] < np.arange(1, n)
    big = start & (reach > np.arange(n))
    s = np.nonzero(big)[0]
    e = np.nonzero((mx == np.arange(n)) & ~start)[0]
    return np.stack([s, e], axis=1) if len(s) else np.zeros((0, 2), np.int64)


def _tarjan_labels(n, edges, labels, base=0):
    """Iterative Tarjan over vertices base..base+n-1: labels[v] = the smallest
    vertex of v's SCC for the SCCs of more than one vertex."""
    succ = [[] for _ in range(n)]
    for s, d in edges:
        succ[s - base].append(d - base)
    index, low, on, stack, k = [-1] * n, [0] * n, [False] * n, [], 0
    for root in range(n):
        if index[root] >= 0:
            continue
        work = [(root, 0)]
        while work:
            v, i = work.pop()
            if i == 0:
                index[v] = low[v] = k
                k += 1
                stack.append(v)
                on[v] = True
            recurse = False
            while i < len(succ[v]):
                w = succ[v][i]
                i += 1
                if index[w] < 0:
                    work.append((v, i))
                    work.append((w, 0))
                    recurse = True
                    break
                if on[w]:
                    low[v] = min(low[v], index[w])
            if recurse:
                continue
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    comp.append(w)
                    if w == v:
                        break
                if len(comp) > 1:
                    for w in comp:
                        labels[base + w] = base + min(comp)
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])


def scc_labels(n, edges):
    """labels[v] = the smallest vertex of v's SCC, -1 when v is in none: Tarjan
    inside each region of the back-edge decomposition (what the device does with
    one workgroup per region)."""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    labels = np.full(n, -1, np.int64)
    reg = regions(n, edges)
    if len(reg) == 0:
        return labels
    rid = np.searchsorted(reg[:, 0], edges, side="right") - 1
    inside = (rid[:, 0] == rid[:, 1]) & (rid[:, 0] >= 0) & (edges[:, 0] != edges[:, 1])
    inside[inside] = (edges[inside] <= reg[rid[inside, 0], 1][:, None]).all(axis=1)
    for r in np.unique(rid[inside, 0]):
        a, b = reg[r]
        _tarjan_labels(int(b - a + 1), edges[inside & (rid[:, 0] == r)].tolist(), labels, int(a))
    return labels


def sccs_of(labels):
    """The SCCs as ascending member lists, ordered by (size, smallest row)."""
    groups = {}
    for v in np.nonzero(labels >= 0)[0].tolist():
        groups.setdefault(int(labels[v]), []).append(v)
    return sorted(groups.values(), key=lambda g: (len(g), g[0]))


def tarjan(graph):
    """cycle.clj:155-160: the SCCs of more than one node of {node: successors}
    (non-negative ints), as a list of sets."""
    g = graph if isinstance(graph, Graph) else map_to_graph(graph)
    return [set(c) for c in sccs_of(scc_labels(g.n, g.edges))]


strongly_connected_components = tarjan


# -- explainers ---------------------------------------------------------------------
def pr_str(x):
    if x is None:
        return "nil"
    if isinstance(x, bool):
        return "true" if x else "false"
    if isinstance(x, str):
        return ":" + x
    return repr(x)


class ProcessExplainer:
    def explain_pair(self, a, b):
        if a.get("process") == b.get("process") and a["index"] < b["index"]:
            return f"which process {a.get('process')} completed before"
        return None


class RealtimeExplainer:
    """pairs: the invocation of a completion, found by walking back to the
    latest invoke of its process."""

    def __init__(self, history):
        self.history = history
        self.pos = {op["index"]: i for i, op in enumerate(history)}

    def invocation(self, op):
        for i in range(self.pos[op["index"]] - 1, -1, -1):
            o = self.history[i]
            if o.get("process") == op.get("process"):
                return o if o.get("type") == "invoke" else None
        return None

    def explain_pair(self, a, b):
        inv = self.invocation(b)
        if inv is None or not a["index"] < inv["index"]:
            return None
        gap = ""
        if a.get("time") is not None and inv.get("time") is not None:     # 0 is truthy in Clojure
            gap = "%.3f seconds " % ((inv["time"] - a["time"]) / 1e9)
        return "which completed" + gap + " before the invocation of"


class WRExplainer:
    def explain_pair(self, a, b):
        writes, reads = ext_writes(a.get("value")), ext_reads(b.get("value"))
        for k in reads:
            if reads.get(k) == writes.get(k):
                return f"which wrote {pr_str(k)} = {pr_str(writes.get(k))}, which was read by"
        return None


class AppendsAndReadsExplainer:
    def explain_pair(self, a, b):
        return "something something"


class MonotonicKeyExplainer:
    """cycle.clj:220-236: the first key of a's map, in a's own key order, that b
    holds too with both values non-nil and a's below b's."""

    def explain_pair(self, a, b):
        a, b = a.get("value") or {}, b.get("value") or {}
        for k in a:
            x, y = a[k], b.get(k)
            if x is not None and y is not None and x < y:
                return f"which observed {pr_str(k)} = {pr_str(x)}, and a higher value {pr_str(y)} was observed by"
        return None


class CombinedExplainer:
    def __init__(self, explainers):
        self.explainers = list(explainers)

    def explain_pair(self, a, b):
        for e in self.explainers:
            s = e.explain_pair(a, b)
            if s is not None:
                return s
        return None


# -- analyzers ----------------------------------------------------------------------
def _indexed(history):
    return [op if "index" in op else dict(op, index=i) for i, op in enumerate(history)]


def process_graph(history):
    history = list(history)
    proc, typ = _encode_rows(history)
    return Graph(len(history), process_edges(proc, typ)), ProcessExplainer()


def realtime_graph(history):
    history = _indexed(history)
    proc, typ = _encode_rows(history)
    return Graph(len(history), realtime_edges(proc, typ)), RealtimeExplainer(history)


def wr_graph(history):
    history = list(history)
    return Graph(len(history), wr_edges(history)), WRExplainer()


process_graph.analyzers, realtime_graph.analyzers, wr_graph.analyzers = A.CY_PROCESS, A.CY_REALTIME, A.CY_WR
# (appends_and_reads_graph, defined with its closed forms below, carries A.CY_APPEND)


def combine(*analyzers):
    """cycle.clj:202-216: the union of the analyzers' graphs."""
    def analyze(history):
        history = list(history)
        g, ex = Graph(len(history)), []
        for an in analyzers:
            g2, e = an(history)
            g, ex = g.union(g2), ex + [e]
        return g, CombinedExplainer(ex)
    masks = [getattr(an, "analyzers", None) for an in analyzers]
    analyze.analyzers = None if None in masks or not masks else int(np.bitwise_or.reduce(masks))
    analyze.parts = analyzers
    return analyze


# -- cycles -------------------------------------------------------------------------
def prune_alternate_paths(paths):
    first = {}
    for p in paths:
        first.setdefault(p[-1], p)
    return list(first.values())


def prune_longer_paths(paths):
    old = {v for p in paths for v in p[:-1]}
    return [p for p in paths if p[-1] not in old]


def grow_paths(g, paths, within=None):
    return [p + [s] for p in paths for s in g.out(p[-1], within)]


def path_shells(g, start, within=None):
    """cycle.clj:825-832: longer and longer paths from start (a generator)."""
    paths = [[start]]
    while True:
        yield paths
        paths = prune_alternate_paths(grow_paths(g, prune_longer_paths(paths), within))


def find_cycle(graph, scc):
    """cycle.clj:868-882: a short cycle in the SCC, from its smallest vertex."""
    within = set(scc)
    for k, shell in enumerate(path_shells(graph, min(within), within)):
        for p in shell:
            if len(p) > 1 and p[0] == p[-1]:
                return p
        if k > len(within) + 1 or not shell:
            raise RuntimeError(f"no cycle through {min(within)} in {sorted(within)}")


def explain_scc(graph, explainer, scc, history):
    """cycle.clj:884-909: [op why op why ... op] around a cycle of the SCC."""
    cyc = find_cycle(graph, scc)
    out = [history[cyc[0]]]
    for a, b in zip(cyc, cyc[1:]):
        why = explainer.explain_pair(history[a], history[b])
        if why is None:
            raise RuntimeError(f"Explainer {explainer!r} was unable to explain the relationship between "
                               f"{history[a]!r} and {history[b]!r}")
        out += [why, history[b]]
    return out


# -- encoding -----------------------------------------------------------------------
def _long(x):
    if x is None:
        return A.NIL
    if not H._is_int(x) or not I64_MIN < x <= I64_MAX:
        raise TypeError(f"cycle: value {x!r} has no encoding")
    return int(x)


def encode(history, txns=True):
    """Op maps -> Columns (include/jh.h, "Cycle txns"). txns: encode the :ok
    rows' :value as micro-op triples (keys interned in first-appearance order;
    TypeError for a value that is no long, a micro-op that is no read / write or
    a :value that is no sequence of triples)."""
    history = list(history)
    n = len(history)
    proc, typ = _encode_rows(history)
    val, val2 = np.full(n, A.NIL, np.int64), np.zeros(n, np.int64)
    aux, key_ids = [], {}
    if txns:
        for i, op in enumerate(history):
            v = op.get("value")
            if op.get("type") != "ok" or op.get("process") == "nemesis" or v is None:
                continue
            if not isinstance(v, (list, tuple)):
                raise TypeError(f"cycle: a txn of {v!r}")
            val[i], val2[i] = len(aux) // 3, len(v)
            for mop in v:
                f, k, x = mop
                if f not in READ_FS + WRITE_FS:
                    raise TypeError(f"cycle: a micro-op {f!r}")
                aux += [A.F_READ if f in READ_FS else A.F_WRITE, key_ids.setdefault(k, len(key_ids)), _long(x)]
    return H.Columns(n=n, process=proc, type=typ, f=np.full(n, A.F_FIRST_INTERNED, np.int64), key=None, value=val,
                     value2=val2, n_keys=0, aux=np.asarray(aux if aux else [0, 0, 0], np.int64)[:max(len(aux), 3)],
                     keys=list(key_ids))


# -- appends-and-reads-graph (cycle.clj:381-699) ---------------------------------------
class AnalysisMap(Exception):
    """throw+ of a map with :valid?: the checker returns the map as its result."""

    def __init__(self, m):
        super().__init__(m.get("message"))
        self.map = m


def encode_append(history, strict=True):
    """Op maps -> Columns (include/jh.h, "Append txns"): every non-nemesis row
    carries its txn as [f, k, a, b] words, the reads' elements behind them in
    the same aux array, keys dense in first-appearance order. TypeError for an
    f outside r / append, a read value that is no list / nil, an element that is
    no long or is nil. strict=False (the host analyzer): elements are interned,
    so anything hashable stands (only their equality is used)."""
    history = list(history)
    n = len(history)
    proc, typ = _encode_rows(history)
    val, val2 = np.full(n, A.NIL, np.int64), np.zeros(n, np.int64)
    words, elems, key_ids, interned = [], [], {}, {}

    def elem(x):
        if strict:
            if x is None or _long(x) == A.NIL:
                raise TypeError(f"cycle: element {x!r} has no encoding")
            return int(x)
        return interned.setdefault(x, len(interned))

    for i, op in enumerate(history):
        v = op.get("value")
        if op.get("process") == "nemesis" or v is None:
            continue
        if not isinstance(v, (list, tuple)):
            raise TypeError(f"cycle: a txn of {v!r}")
        val[i], val2[i] = len(words), len(v)
        for mop in v:
            f, k, x = mop
            kid = key_ids.setdefault(k, len(key_ids))
            if f in READ_FS:
                if x is not None and not isinstance(x, (list, tuple)):
                    raise TypeError(f"cycle: a read of {x!r}")
                words += [A.F_READ, kid, -1 - len(elems), len(x or ())]       # the offset: placed below
                elems += [elem(e) for e in (x or ())]
            elif f == APPEND_F:
                words += [A.F_APPEND, kid, elem(x), 0]
            else:
                raise TypeError(f"cycle: a micro-op {f!r}")
    aux = np.asarray(words + elems, np.int64) if words else np.zeros(0, np.int64)
    w = aux[:len(words)].reshape(-1, 4)
    reads = w[:, 0] == A.F_READ
    w[reads, 2] = len(words) + (-1 - w[reads, 2])
    return H.Columns(n=n, process=proc, type=typ, f=np.full(n, A.F_FIRST_INTERNED, np.int64), key=None, value=val,
                     value2=val2, n_keys=len(key_ids), aux=aux if len(aux) else np.zeros(4, np.int64)[:0], keys=list(key_ids))


class _Mops:
    """The read and append records of encoded append txns, in (row, micro-op) order."""

    def __init__(self, cols):
        proc, typ, aux = np.asarray(cols.process), np.asarray(cols.type), np.asarray(cols.aux, np.int64)
        val2 = np.asarray(cols.value2)
        rows = np.nonzero((proc != -1) & (val2 > 0))[0]
        cnt = val2[rows]
        mrow = np.repeat(rows, cnt)
        mj = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        base = np.repeat(np.asarray(cols.value)[rows], cnt) + 4 * mj
        f = aux[base] if len(base) else np.zeros(0, np.int64)
        pick = lambda sel, off: aux[base[sel] + off] if len(base) else np.zeros(0, np.int64)
        r, a = f == A.F_READ, f == A.F_APPEND
        self.aux, self.n_keys = aux, int(cols.n_keys)
        self.rrow, self.rmop, self.rk, self.roff, self.rlen = mrow[r], mj[r], pick(r, 1), pick(r, 2), pick(r, 3)
        self.arow, self.amop, self.ak, self.av = mrow[a], mj[a], pick(a, 1), pick(a, 2)
        self.rcnt = np.isin(typ[self.rrow], (A.TYPE_OK, A.TYPE_INFO))
        self.atype = typ[self.arow]
        self.entries = int(len(f) + self.rlen.sum())

    def elements(self, reads):
        """(read, place, element) of every element of the reads `reads` (record indices)."""
        ln = self.rlen[reads]
        rid = np.repeat(reads, ln)
        place = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
        return rid, place, self.aux[self.roff[rid] + place]

    def longest(self):
        """lrec[k] = the record of k's longest counted read (the first of that length), -1: none."""
        c = np.nonzero(self.rcnt)[0]
        o = c[np.lexsort((c, -self.rlen[c], self.rk[c]))]
        first = np.ones(len(o), bool)
        first[1:] = self.rk[o[1:]] != self.rk[o[:-1]]
        lrec = np.full(self.n_keys, -1, np.int64)
        lrec[self.rk[o[first]]] = o[first]
        return lrec


def duplicate_append(m):
    """cycle.clj:407-426: (row, micro-op) of the first :invoke append whose (k, v)
    an earlier :invoke micro-op appended, or None."""
    idx = np.nonzero(m.atype == A.TYPE_INVOKE)[0]
    if len(idx) < 2:
        return None
    o = idx[np.lexsort((idx, m.av[idx], m.ak[idx]))]
    again = (m.ak[o[1:]] == m.ak[o[:-1]]) & (m.av[o[1:]] == m.av[o[:-1]])
    if not again.any():
        return None
    x = int(o[1:][again].min())
    return int(m.arow[x]), int(m.amop[x])


def duplicate_read(m):
    """cycle.clj:499-519: (row, micro-op) of the first read, on a row of any
    type, that holds an element twice, or None."""
    rid, place, ev = m.elements(np.nonzero(m.rlen > 1)[0])
    if len(rid) == 0:
        return None
    o = np.lexsort((ev, rid))
    again = (rid[o[1:]] == rid[o[:-1]]) & (ev[o[1:]] == ev[o[:-1]])
    if not again.any():
        return None
    x = int(rid[o[1:]][again].min())
    return int(m.rrow[x]), int(m.rmop[x])


def bad_order_keys(m):
    """cycle.clj:438-497 in closed form: {key id: smallest row with a counted read
    of it that is no prefix of the key's longest counted read}."""
    lrec = m.longest()
    rid, place, ev = m.elements(np.nonzero(m.rcnt & (m.rlen > 0))[0])
    if len(rid) == 0:
        return {}
    bad = rid[ev != m.aux[m.roff[lrec[m.rk[rid]]] + place]]
    out = {}
    for x in np.unique(bad).tolist():
        out.setdefault(int(m.rk[x]), int(m.rrow[x]))
    return out


def append_edges(m):
    """cycle.clj:641-699 in closed form over the records of a history that passed
    the three checks: the (E, 2) wr, ww and rw edges, one per link call (repeats
    kept, a row never links to itself). IllegalHistory("no-writer") at the first
    micro-op whose wr / ww writer does not exist; .key / .value name the pair."""
    lrec = m.longest()
    ca = np.nonzero(np.isin(m.atype, (A.TYPE_OK, A.TYPE_INFO)))[0]
    cr = np.nonzero(m.rcnt)[0]
    # L_k's elements, key after key (lstart[k] = where L_k starts)
    keys = np.nonzero(lrec >= 0)[0]
    _, lj, lv = m.elements(lrec[keys])
    lk = np.repeat(keys, m.rlen[lrec[keys]])
    lstart = np.zeros(m.n_keys + 1, np.int64)
    lstart[keys + 1] = m.rlen[lrec[keys]]
    lstart = np.cumsum(lstart)
    nz = cr[m.rlen[cr] > 0]
    last = m.aux[m.roff[nz] + m.rlen[nz] - 1]
    uniq = np.unique(np.concatenate([m.av[ca], lv, last]))

    def pair(k, v):                          # (k, v) as one word that compares like the pair
        return k * max(len(uniq), 1) + np.searchsorted(uniq, v)

    def lookup(table_keys, table_vals, q):   # table_keys ascending; -1 where q is not in it
        if len(table_keys) == 0:
            return np.full(len(q), -1, np.int64)
        at = np.minimum(np.searchsorted(table_keys, q), len(table_keys) - 1)
        return np.where(table_keys[at] == q, table_vals[at], -1)
    # writers: the last counted append of (k, v)
    wkey = pair(m.ak[ca], m.av[ca])
    o = np.lexsort((ca, wkey))
    lastof = np.ones(len(o), bool)
    lastof[:-1] = wkey[o[1:]] != wkey[o[:-1]]
    wkeys, wrows = wkey[o[lastof]], m.arow[ca[o[lastof]]]
    # the counted appends' positions in L_k
    lkey = pair(lk, lv)
    lo = np.argsort(lkey, kind="stable")
    pos = lookup(lkey[lo], lj[lo], wkey)
    missing, edges = [], []
    # wr
    w = lookup(wkeys, wrows, pair(m.rk[nz], last))
    missing += [(int(m.rrow[x]), int(m.rmop[x]), int(m.rk[x]), int(e)) for x, e in zip(nz[w < 0].tolist(), last[w < 0].tolist())]
    keep = (w >= 0) & (w != m.rrow[nz])
    edges.append(np.stack([w[keep], m.rrow[nz][keep]], axis=1))
    # ww
    xs = ca[pos > 0]
    prev = lv[lstart[m.ak[xs]] + pos[pos > 0] - 1]
    w = lookup(wkeys, wrows, pair(m.ak[xs], prev))
    missing += [(int(m.arow[x]), int(m.amop[x]), int(m.ak[x]), int(e)) for x, e in zip(xs[w < 0].tolist(), prev[w < 0].tolist())]
    keep = (w >= 0) & (w != m.arow[xs])
    edges.append(np.stack([w[keep], m.arow[xs][keep]], axis=1))
    if missing:
        row, mop, k, v = min(missing)
        e = IllegalHistory("no-writer", row)
        e.mop, e.key, e.value = mop, k, v
        raise e
    # rw: the counted reads of k of length i -> the append at position i
    span = int(m.rlen[cr].max()) + 1 if len(cr) else 1
    rsort = cr[np.argsort(m.rk[cr] * span + m.rlen[cr], kind="stable")]
    rkeys = m.rk[rsort] * span + m.rlen[rsort]
    xs = ca[pos >= 0]
    q = m.ak[xs] * span + pos[pos >= 0]
    lo_, hi_ = np.searchsorted(rkeys, q, side="left"), np.searchsorted(rkeys, q, side="right")
    cnt = hi_ - lo_
    dst = np.repeat(m.arow[xs], cnt)
    within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    src = m.rrow[rsort[np.repeat(lo_, cnt) + within]]
    edges.append(np.stack([src, dst], axis=1)[src != dst])
    return np.concatenate(edges).astype(np.int64).reshape(-1, 2)


def _mop_types_map(history):
    bad = [op for op in history if not all(m[0] in READ_FS + (APPEND_F,) for m in (op.get("value") or ()))]
    return {"valid?": "unknown", "type": "unexpected-txn-micro-op-types",
            "message": "history contained operations other than appends or reads", "examples": bad[:8]} if bad else None


def _duplicate_appends_map(op, mop):
    _, k, v = op["value"][mop]
    return {"valid?": "unknown", "type": "duplicate-appends", "op": op, "key": k, "value": v,
            "message": f"value {pr_str(v)} appended to key {pr_str(k)} multiple times!"}


def _duplicate_elements_map(op, mop):
    _, k, v = op["value"][mop]
    freq = {}
    for x in v:
        freq[x] = freq.get(x, 0) + 1
    return {"valid?": False, "type": "duplicate-elements",
            "message": "Observed multiple copies of a value which was only inserted once",
            "op": op, "key": k, "value": v, "duplicates": {x: c for x, c in sorted(freq.items()) if c > 1}}


def _is_prefix(a, b):
    a, b = a or (), b or ()
    return len(a) <= len(b) and all(x == y for x, y in zip(a, b))


def total_order_map(history, bad_keys):
    """The :no-total-state-order map over the keys `bad_keys`: per key its distinct
    :ok / :info reads sorted by (length, first appearance) and their first
    adjacent pair that is no prefix pair; keys in first-appearance order."""
    seen = {}
    for op in history:
        if op.get("type") in ("ok", "info") and op.get("process") != "nemesis":
            for f, k, v in (op.get("value") or ()):
                if f in READ_FS and k in bad_keys:
                    seen.setdefault(k, {}).setdefault(None if v is None else tuple(v), v)
    errors = []
    for k, by_value in seen.items():
        vs = sorted(by_value.values(), key=lambda v: len(v or ()))
        for a, b in zip(vs, vs[1:]):
            if not _is_prefix(a, b):
                errors.append({"key": k, "values": [a, b]})
                break
    return {"valid?": False, "type": "no-total-state-order",
            "message": "observed mutually incompatible orders of appends", "errors": errors}


def appends_and_reads_graph(history):
    """cycle.clj:575-699. Raises AnalysisMap for a check that throws a map with
    :valid? (check_host returns it) and IllegalHistory for a missing writer."""
    history = list(history)
    bad = _mop_types_map(history)
    if bad:
        raise AnalysisMap(bad)
    try:
        cols = encode_append(history)
    except TypeError:
        cols = encode_append(history, strict=False)
    m = _Mops(cols)
    at = duplicate_append(m)
    if at:
        raise AnalysisMap(_duplicate_appends_map(history[at[0]], at[1]))
    at = duplicate_read(m)
    if at:
        raise AnalysisMap(_duplicate_elements_map(history[at[0]], at[1]))
    bad_keys = bad_order_keys(m)
    if bad_keys:
        raise AnalysisMap(total_order_map(history, {cols.keys[k] for k in bad_keys}))
    return Graph(len(history), append_edges(m)), AppendsAndReadsExplainer()


# -- monotonic-key-graph (cycle.clj:218-267) -------------------------------------------
def _map_records(history):
    """(key id, value, row) of every pair of the :ok non-nemesis rows' maps, in row
    order; keys interned in first-appearance order. TypeError for an :ok :value
    that is neither a map nor nil."""
    kid, val, row, key_ids = [], [], [], {}
    for i, op in enumerate(history):
        v = op.get("value")
        if op.get("type") != "ok" or op.get("process") == "nemesis" or v is None:
            continue
        if not isinstance(v, dict):
            raise TypeError(f"cycle: a map of {v!r}")
        for k, x in v.items():
            kid.append(key_ids.setdefault(k, len(key_ids)))
            val.append(x)
            row.append(i)
    return np.asarray(kid, np.int64), val, np.asarray(row, np.int64), key_ids


def _value_ranks(kid, val):
    """Per record the rank of its value among its key's distinct values in
    Python's own order, nil first (values that are no longs; TypeError for a
    key whose values do not compare)."""
    by_key = {}
    for k, x in zip(kid.tolist(), val):
        if x is not None:
            by_key.setdefault(k, set()).add(x)
    rank = {k: {x: i + 1 for i, x in enumerate(sorted(xs))} for k, xs in by_key.items()}
    return np.asarray([0 if x is None else rank[k][x] for k, x in zip(kid.tolist(), val)], np.int64)


def link_groups(kid, v, row):
    """The closed form over records (key, value, row) as int64 arrays: sorted by
    (k, v, row), every record links to every record of the next (k, v) group of
    its key. One edge per link call. MemoryError, before anything of that size
    is allocated, for more than 2^31 - 2 link calls."""
    if len(kid) == 0:
        return np.zeros((0, 2), np.int64)
    o = np.lexsort((row, v, kid))
    k_s, v_s, r_s = kid[o], v[o], row[o]
    start = np.ones(len(o), bool)
    start[1:] = (k_s[1:] != k_s[:-1]) | (v_s[1:] != v_s[:-1])
    gid = np.cumsum(start) - 1
    gstart = np.nonzero(start)[0]
    gsize = np.diff(np.append(gstart, len(o)))
    # per group: the start and size of the next group when it is of the same key
    nsize = np.zeros(len(gstart), np.int64)
    nstart = np.zeros(len(gstart), np.int64)
    same = k_s[gstart[1:]] == k_s[gstart[:-1]]
    nsize[:-1][same], nstart[:-1][same] = gsize[1:][same], gstart[1:][same]
    cnt = nsize[gid]
    total = int(cnt.sum(dtype=np.int64))
    if total > (1 << 31) - 2:
        raise MemoryError(f"cycle: monotonic-key-graph of {total} link calls (more than 2^31 - 2)")
    if total == 0:
        return np.zeros((0, 2), np.int64)
    within = np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return np.stack([np.repeat(r_s, cnt), r_s[np.repeat(nstart[gid], cnt) + within]], axis=1)


def monotonic_key_edges(history):
    """cycle.clj:238-267 over positions (link_groups over the maps' records). A
    pair of rows linked through two keys stands twice. Values that are no longs
    are ordered with Python's own comparison, nil first."""
    kid, val, row, _ = _map_records(history)
    try:
        v = np.asarray([_long(x) for x in val], np.int64)
    except TypeError:
        v = _value_ranks(kid, val)
    return link_groups(kid, v, row)


def map_edges(cols):
    """link_groups over Columns in the map reads encoding (what the device builds from them)."""
    proc, typ, val2 = np.asarray(cols.process), np.asarray(cols.type), np.asarray(cols.value2)
    rows = np.nonzero((typ == A.TYPE_OK) & (proc != -1) & (val2 > 0))[0]
    cnt = val2[rows]
    row = np.repeat(rows, cnt)
    at = 2 * (np.repeat(np.asarray(cols.value)[rows], cnt) + np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    aux = np.asarray(cols.aux, np.int64)
    return link_groups(aux[at], aux[at + 1], row) if len(row) else np.zeros((0, 2), np.int64)


def monotonic_key_graph(history):
    history = list(history)
    return Graph(len(history), monotonic_key_edges(history)), MonotonicKeyExplainer()


monotonic_key_graph.analyzers = A.CY_MONOTONIC


def encode_map(history):
    """Op maps -> Columns (include/jh.h, "Map reads encoding"): an :ok row's map
    as (key, value) pairs in aux, keys interned in first-appearance order, nil ->
    JH_NIL. TypeError for an :ok :value that is neither a map nor nil and for a
    value that is no long."""
    history = list(history)
    n = len(history)
    proc, typ = _encode_rows(history)
    kid, vals, row, key_ids = _map_records(history)
    val, val2 = np.full(n, A.NIL, np.int64), np.zeros(n, np.int64)
    aux = np.zeros(2 * len(kid) + 2, np.int64)[:2 * len(kid)]
    aux[0::2], aux[1::2] = kid, [_long(x) for x in vals]
    rows, first, cnt = np.unique(row, return_index=True, return_counts=True)
    val[rows], val2[rows] = first, cnt
    return H.Columns(n=n, process=proc, type=typ, f=np.full(n, A.F_FIRST_INTERNED, np.int64), key=None, value=val,
                     value2=val2, n_keys=0, aux=aux, keys=list(key_ids))


# -- the checker --------------------------------------------------------------------
def _result(graph, explainer, sccs, history):
    return {"valid?": not sccs, "scc-count": len(sccs),
            "cycles": [explain_scc(graph, explainer, c, history) for c in sccs[:A.CY_SCC_CAP]]}


def check_host(analyze_fn, history):
    """The checker's map on the host: cycle.clj:911-934."""
    history = [op for op in _indexed(history) if op.get("process") != "nemesis"]
    try:
        graph, explainer = analyze_fn(history)
    except AnalysisMap as e:                  # the reference's try+: a map with :valid? is the result
        return e.map
    except IllegalArgument as e:              # positions in the filtered history -> the ops' own :index
        e.row, e.rows = history[e.row]["index"], [history[j]["index"] for j in e.rows]
        raise
    except IllegalHistory as e:
        raise IllegalHistory(e.cause, history[e.row]["index"]) from None
    sccs = sccs_of(scc_labels(graph.n, graph.edges))
    return _result(graph, explainer, sccs, history)


def _explainer_for(analyze_fn, history):
    table = {process_graph: ProcessExplainer, wr_graph: WRExplainer, appends_and_reads_graph: AppendsAndReadsExplainer,
             monotonic_key_graph: MonotonicKeyExplainer}
    parts = getattr(analyze_fn, "parts", (analyze_fn,))
    out = []
    for p in parts:
        if p is realtime_graph:
            out.append(RealtimeExplainer([op for op in history if op.get("process") != "nemesis"]))
        elif p in table:
            out.append(table[p]())
        else:
            out.append(_explainer_for(p, history))
    return out[0] if len(out) == 1 and not hasattr(analyze_fn, "parts") else CombinedExplainer(out)


def raise_unknown(res, history, keys):
    """What the reference raises for a JH_UNKNOWN result."""
    cause, row = res["cause"], res["unknown_row"]
    if cause == A.CAUSE_MULTIPLE_WRITES:
        k, v = keys[res["unknown_key"]], (None if res["unknown_value"] == A.NIL else res["unknown_value"])
        e = IllegalArgument(f"Key {pr_str(k)} had value {pr_str(v)} written by more than one op: "
                            f"{[history[j] for j in res['unknown_rows']]!r}")
        e.row, e.key, e.value, e.rows = row, k, v, list(res["unknown_rows"])
        raise e
    raise IllegalHistory(A.CAUSES[cause], row)


def append_map(res, history, cols):
    """The reference's map for causes 13-15, from the row the device names."""
    op, at = history[res["unknown_row"]], res["unknown_rows"][0]
    if res["cause"] == A.CAUSE_DUPLICATE_APPENDS:
        return _duplicate_appends_map(op, at)
    if res["cause"] == A.CAUSE_DUPLICATE_ELEMENTS:
        return _duplicate_elements_map(op, at)
    out = total_order_map(history, {cols.keys[k] for k in bad_order_keys(_Mops(cols))})
    if len(out["errors"]) != at:
        raise RuntimeError(f"cycle: the device names {at} keys without a total order, the host {len(out['errors'])}")
    return out


class CycleChecker:
    """(cycle/checker analyze-fn). path: 0 auto, 1 on-chip, 2 global tier.
    device=False keeps everything on the host."""

    def __init__(self, analyze_fn, path=A.CY_PATH_AUTO, device=True):
        self.analyze_fn, self.path, self.device = analyze_fn, path, device

    def check(self, test, history, opts):
        from . import _native
        from . import checker as K
        mask = getattr(self.analyze_fn, "analyzers", None)
        history = _indexed(history)
        readers = [bit for bit in (A.CY_WR, A.CY_APPEND, A.CY_MONOTONIC) if mask and mask & bit]
        if not self.device or not mask or len(readers) > 1:       # (each of them reads aux in its own way)
            return check_host(self.analyze_fn, history)
        try:
            cols = encode_append(history) if mask & A.CY_APPEND else encode_map(history) if mask & A.CY_MONOTONIC else \
                encode(history, txns=bool(mask & A.CY_WR))
        except (TypeError, ValueError):
            return check_host(self.analyze_fn, history)
        try:
            ctx = K._ctx()
            res = ctx.check_cycle(cols, mask, self.path)
            if res["valid"] == A.INVALID:
                res = ctx.check_cycle(cols, mask, self.path, edge_cap=sum(res["edge_count"]))
        except _native.JhError as e:
            if e.code != A.JH_EUNSUPPORTED:
                raise
            return check_host(self.analyze_fn, history)
        if res["cause"] in (A.CAUSE_DUPLICATE_APPENDS, A.CAUSE_DUPLICATE_ELEMENTS, A.CAUSE_NO_TOTAL_ORDER):
            return append_map(res, history, cols)
        if res["valid"] == A.UNKNOWN:
            raise_unknown(res, history, cols.keys)
        sccs = res["sccs"]
        if not sccs:
            return {"valid?": True, "scc-count": 0, "cycles": []}
        members = set(v for c in sccs for v in c)
        e = res["edges"]
        e = e[np.isin(e[:, 0], list(members)) & np.isin(e[:, 1], list(members))]
        out = _result(Graph(cols.n, e), _explainer_for(self.analyze_fn, history), sccs, history)
        out["scc-count"] = int(res["scc_count"])
        return out


def checker(analyze_fn, path=A.CY_PATH_AUTO, device=True):
    return CycleChecker(analyze_fn, path, device)


appends_and_reads_graph.analyzers = A.CY_APPEND
