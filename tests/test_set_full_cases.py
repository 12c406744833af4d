"""The two set-full restatements (oracle/set_full.py, the op-map fold pinned by
the reference's known answers, and oracle/set_full_np.py) against each other
over the cases of set_full_cases.py -- the same cases
test_gpu_set_full_edges.py runs on the device -- and the conditions that keep
those cases from degenerating. No GPU.

The numpy restatement finds a read's invocation as "the process' previous
row"; the fold keeps a `reads` map (checker.clj:489-493). Overlapping
readers, :fail and :info reads and renumbered processes are where the two
could part.
"""
import pytest

import set_full_cases as C
from oracle import set_full as SF
from oracle import set_full_np as SN


def flat_worst(m):
    m = dict(m)
    m["worst-stale"] = [(r["element"], r["stable-latency"], r["known"]["index"],
                         r["last-absent"]["index"] if r["last-absent"] else -1) for r in m["worst-stale"]]
    return m


def both(ops, what):
    """The fold's result map (worst-stale flattened), equal to the numpy
    restatement's for either :linearizable?."""
    out = None
    for lin in (False, True):
        a = flat_worst(SF.set_full(ops, linearizable=lin))
        cols, time = C.encode(ops)
        b = SN.set_full_cols(cols, time, linearizable=lin)
        assert a == b, (what, lin, {k: (a[k], b[k]) for k in a if a[k] != b.get(k)})
        out = out or a
    return out


def ok_reads(ops):
    return [o for o in ops if o["type"] == "ok" and o["f"] == "read" and isinstance(o["process"], int)]


def fold_reads(ops, keep_max=True):
    """{element: (last-present, last-absent)} as :index or None, by the
    reference's rule (the invocation of greater :index is kept) or, with
    keep_max false, by "the latest :ok row wins"."""
    elements, reads = {}, {}
    for o in ops:
        if not isinstance(o["process"], int):
            continue
        f, t, v = o["f"], o["type"], o["value"]
        if f == "add" and t == "invoke":
            elements[v] = [None, None]
        elif f == "read" and t == "invoke":
            reads[o["process"]] = o["index"]
        elif f == "read" and t == "ok":
            inv, vs = reads[o["process"]], set(v or ())
            for el, st in elements.items():
                k = 0 if el in vs else 1
                if not keep_max or st[k] is None or st[k] < inv:
                    st[k] = inv
    return {e: tuple(st) for e, st in elements.items()}


# -- the sweep ----------------------------------------------------------------------
@pytest.mark.parametrize("m", C.SF_ELEMS)
def test_sweep_oracles_agree(m):
    """Every shape of the sweep: exactly R :ok reads and M elements, the two
    restatements equal; with M >= 63 and R >= 2 never :unknown, and at least
    one stable, one lost, one never-read and one stale element."""
    for r in C.SF_READS:
        ops = C.sweep_case(m, r)
        res = both(ops, (m, r))
        assert len(ok_reads(ops)) == r and res["attempt-count"] == m
        assert res["stable-count"] + res["lost-count"] + res["never-read-count"] == m
        if m >= 63 and r >= 2:
            assert res["valid?"] != "unknown", (m, r)
            for k in ("stable-count", "lost-count", "never-read-count", "stale-count"):
                assert res[k] > 0, (m, r, k)


def test_sweep_builder_knobs():
    """What the builder promises, on the 65 x 65 case: holes in the element
    window; reads unsorted, with repeats, a value below the smallest element,
    one above the largest, one in a hole and (every other case) a nil; a nil
    and an empty read; :fail and :info reads and adds; nemesis reads and a
    nemesis add outside the client range; a read that holds an element before
    its add is invoked; the last reads completed in descending process order;
    the bases and time steps."""
    ops = C.sweep_case(65, 65)
    client = [o for o in ops if isinstance(o["process"], int)]
    adds = [o for o in client if o["f"] == "add" and o["type"] == "invoke"]
    els = sorted({o["value"] for o in adds})
    assert len(els) == 65 and els[-1] - els[0] + 1 > 65
    reads = ok_reads(ops)
    assert any(o["value"] is None for o in reads) and any(o["value"] == [] for o in reads)
    full = [o["value"] for o in reads if o["value"]]
    ints = [[x for x in v if x is not None] for v in full]
    assert all(v != sorted(v) for v in ints if len(v) > 8)
    assert all(len(set(v)) < len(v) for v in ints)
    assert all(min(v) < els[0] and max(v) > els[-1] for v in ints)
    assert all(any(els[0] < x < els[-1] and x not in els for x in v) for v in ints)
    assert sum(1 for m, r in C.sweep() if any(None in (o["value"] or ()) for o in ok_reads(C.sweep_case(m, r)))) == 24
    for f in ("read", "add"):
        for t in ("fail", "info"):
            assert any(o["f"] == f and o["type"] == t for o in client), (f, t)
    nem = [o for o in ops if o["process"] == "nemesis"]
    assert any(o["f"] == "read" and o["type"] == "ok" and o["value"] for o in nem)
    assert any(o["f"] == "add" and o["type"] == "invoke" and o["value"] > els[-1] + 10 ** 11 for o in nem)
    first_inv = {}
    for o in adds:
        first_inv.setdefault(o["value"], o["index"])
    assert any(x in first_inv and first_inv[x] > o["index"] for o in reads for x in (o["value"] or ()) if x is not None)
    last3 = reads[-3:]
    assert [o["process"] for o in last3] == sorted((o["process"] for o in last3), reverse=True)
    inv_of = fold_invocations(ops)
    assert [inv_of[o["index"]] for o in last3] == sorted((inv_of[o["index"]] for o in last3), reverse=True)
    bases = {min(o["value"] for o in C.sweep_case(m, 2) if o["f"] == "add") >> 39 for m in (63, 64, 65)}
    assert bases == {0, -1, 2}
    assert {C.sweep_case(m, 2)[0]["time"] > 1 << 61 for m in (63, 64)} == {False, True}
    steps = {b["time"] - a["time"] for a, b in zip(ops, ops[1:])}
    assert steps == set(C.STEPS)


def test_sweep_known_from_a_read_before_the_ok_add():
    """In every sweep case with M >= 63 and R >= 63 some element is first held
    by an :ok read while its add is in flight: known is the read's row, not
    the later :ok :add's. And some :ok read's invocation lies more than 64
    rows back (a second round of the device's backward scan)."""
    far = 0
    for m, r in C.sweep():
        ops = C.sweep_case(m, r)
        inv = fold_invocations(ops)
        far = max(far, max(k - v for k, v in inv.items()))
        last_inv, first_read, ok_add = {}, {}, {}
        for o in ops:
            if not isinstance(o["process"], int):
                continue
            if o["f"] == "add" and o["type"] == "invoke":
                last_inv[o["value"]] = o["index"]
                first_read.pop(o["value"], None)
                ok_add.pop(o["value"], None)
            elif o["f"] == "add" and o["type"] == "ok":
                ok_add.setdefault(o["value"], o["index"])
            elif o["f"] == "read" and o["type"] == "ok":
                for x in set(o["value"] or ()):
                    if x in last_inv:
                        first_read.setdefault(x, o["index"])
        n = sum(1 for x in ok_add if x in first_read and first_read[x] < ok_add[x])
        if m >= 63 and r >= 63:
            assert n >= 3, (m, r, n)
    assert far > 64


def fold_invocations(ops):
    """{:index of an :ok read: :index of its invocation} by the reads map."""
    reads, out = {}, {}
    for o in ops:
        if o["f"] == "read" and isinstance(o["process"], int):
            if o["type"] == "invoke":
                reads[o["process"]] = o["index"]
            elif o["type"] == "ok":
                out[o["index"]] = reads[o["process"]]
    return out


# -- the families -----------------------------------------------------------------------
FAMILIES = {
    "overlapping": C.overlapping,
    "reinvoked": C.reinvoked,
    "ignored-rows": C.ignored_rows,
    "sparse-three": lambda: C.sparse("three"),
    "sparse-forty": lambda: C.sparse("forty"),
    "chunk-edges": C.chunk_edges,
    "list-cap": C.list_cap_case,
    "boundary": C.boundary_case,
    "reversed-completion": C.reversed_completion_case,
}


@pytest.mark.parametrize("name", list(FAMILIES))
def test_family_oracles_agree(name):
    res = both(FAMILIES[name](), name)
    assert res["attempt-count"] > 0 and res["valid?"] != "unknown"


def test_overlapping_reads_tell_the_rules_apart():
    """At least one element's last-present and one element's last-absent are
    not what "the latest :ok row wins" gives; and some :ok reads complete in
    the opposite order of their invocations."""
    ops = C.overlapping()
    ref, latest = fold_reads(ops), fold_reads(ops, keep_max=False)
    assert any(ref[e][0] != latest[e][0] for e in ref)
    assert any(ref[e][1] != latest[e][1] for e in ref)
    inv = fold_invocations(ops)
    rows = sorted(inv)
    assert sum(1 for a, b in zip(rows, rows[1:]) if inv[a] > inv[b]) >= 3
    for m, r in C.sweep():
        if m >= 63 and r >= 2:
            o = C.sweep_case(m, r)
            assert fold_reads(o) != fold_reads(o, keep_max=False), (m, r)


def test_reinvoked_adds_shape():
    """Five elements of element word 0 (dense ids below 64) are invoked again
    at different rows between the reads, completed :ok, :info or not at all:
    the word's smallest last invocation is below most lanes' own. One more
    element is invoked again after the last read and comes out never-read,
    known from its new :ok."""
    ops = C.reinvoked()
    res = both(ops, "reinvoked")
    els = sorted({o["value"] for o in ops if o["f"] == "add" and o["type"] == "invoke"})
    last_read = ok_reads(ops)[-1]["index"]
    first_read = ok_reads(ops)[0]["index"]
    inv_rows = {}
    for o in ops:
        if o["f"] == "add" and o["type"] == "invoke":
            inv_rows.setdefault(o["value"], []).append(o["index"])
    again = {els.index(v): rs for v, rs in inv_rows.items() if len(rs) > 1}
    between = {i: rs[-1] for i, rs in again.items() if first_read < rs[-1] < last_read}
    word0 = [i for i in between if i < 64]
    assert len(word0) >= 5 and len({between[i] for i in word0}) == len(word0)
    assert any(i >= 64 for i in between)
    done = set()
    for i in between:
        nxt = [o["type"] for o in ops[between[i] + 1:] if o["f"] == "add" and o["value"] == els[i]]
        done.add(nxt[0] if nxt else "none")
    assert done == {"ok", "info", "none"}
    after = [i for i, rs in again.items() if rs[-1] > last_read]
    assert len(after) == 1 and els[after[0]] in res["never-read"]


def test_chunk_edges_shape():
    ops = C.chunk_edges()
    els = {o["value"] for o in ops if o["f"] == "add"}
    assert len(els) == C.CHUNK_ELEMS
    reads = [o["value"] for o in ok_reads(ops)]
    exact = [v for v in reads if len(set(v)) == len(v) and set(v) <= els]
    assert sorted(len(v) for v in exact) == sorted(C.CHUNK_READ_SIZES + [C.CHUNK_ELEMS])
    assert all(v != sorted(v) for v in exact if len(v) > 8)
    padded = [v for v in reads if not set(v) <= els]
    assert sorted(len(set(v) & els) for v in padded) == [4096, 8192]
    assert sorted(len(v) for v in padded) == [4096 + 7, 8192 + 7]


# -- planned latencies ------------------------------------------------------------------
@pytest.mark.parametrize("c", C.QUANTILE_STABLE)
def test_quantile_family_stable(c):
    """Exactly c stable elements with latencies 0 .. c-1 ms."""
    res = both(C.quantile_case(c, 0), c)
    assert (res["stable-count"], res["stale-count"], res["lost-count"], res["never-read-count"]) == (c, c - 1, 0, 0)
    assert res["stable-latencies"] == SF.frequency_distribution([0, 0.5, 0.95, 0.99, 1], range(c))
    assert [w[1] for w in res["worst-stale"]] == list(range(c - 1, 0, -1))[:8]


@pytest.mark.parametrize("c", C.QUANTILE_LOST)
def test_quantile_family_lost(c):
    res = both(C.quantile_case(3, c), c)
    assert (res["stable-count"], res["lost-count"]) == (3, c)
    assert res["lost-latencies"] == SF.frequency_distribution([0, 0.5, 0.95, 0.99, 1], range(c))
    assert res["lost"] != [] and res["lost"] == sorted(res["lost"])


@pytest.mark.parametrize("s", C.WORST_STALE)
def test_worst_stale_family(s):
    """Exactly s stale elements; with 9 and 30 the three first worst-stale
    entries share the largest latency, the larger element first."""
    res = both(C.worst_stale_case(s), s)
    assert res["stale-count"] == s and res["stable-count"] == s + 2
    w = res["worst-stale"]
    assert len(w) == min(s, 8)
    assert [x[1] for x in w] == sorted((x[1] for x in w), reverse=True)
    if s >= 9:
        assert w[0][1] == w[1][1] == w[2][1] > w[3][1]
        assert w[0][0] > w[1][0] > w[2][0]
    if s == 30:
        lats = sorted(C.worst_stale_lats(s), reverse=True)
        assert lats[7] == lats[8] == lats[9] == w[7][1]            # equal latencies across the cut
        tied = [e for e, lat in stale_latencies(C.worst_stale_case(s)).items() if lat == lats[7]]
        assert len(tied) == 3 and w[7][0] == max(tied)             # the largest of the three makes the cut


def stale_latencies(ops):
    """{element: stable latency} of every stale element, worked out from the
    folds here (worst-stale holds eight at most)."""
    known, reads = fold_known(ops), fold_reads(ops)
    t = {o["index"]: o["time"] for o in ops}
    return {e: max(t[reads[e][1]] + 1 - t[known[e]], 0) // C.MS for e in SF.set_full(ops)["stale"]}


def fold_known(ops):
    """{element: :index of its :known op} (first :ok :add or :ok read holding
    it after its last :invoke :add)."""
    known = {}
    for o in ops:
        if not isinstance(o["process"], int):
            continue
        f, t, v = o["f"], o["type"], o["value"]
        if f == "add" and t == "invoke":
            known[v] = None
        elif f == "add" and t == "ok" and v in known and known[v] is None:
            known[v] = o["index"]
        elif f == "read" and t == "ok":
            for x in set(v or ()):
                if x in known and known[x] is None:
                    known[x] = o["index"]
    return known


def test_list_cap_case_shape():
    res = both(C.list_cap_case(), "list-cap")
    assert (res["lost-count"], res["never-read-count"], res["stale-count"]) == (4, 3, 5)


# -- known answers written out by hand ------------------------------------------------------
def test_boundary_known_answer():
    """time[last-absent] - time[known] = 999 998 / 999 999 / 1 000 000 ns for
    elements 10 / 11 / 12: with the inc, 999 999 / 1 000 000 / 1 000 001 ns =
    0 / 1 / 1 ms. Element 13 is known (row 8) after the invocation (row 6) of
    the read that misses it: max 0. All four are stable (last-present row 10);
    the two of 1 ms are stale, the larger element first in worst-stale."""
    ops = C.boundary_case()
    t = {o["index"]: o["time"] for o in ops}
    assert [t[6] - t[k] for k in (5, 4, 3)] == [999_998, 999_999, 1_000_000] and t[8] > t[6]
    want = {"valid?": True, "attempt-count": 4, "stable-count": 4, "lost-count": 0, "lost": [],
            "never-read-count": 0, "never-read": [], "stale-count": 2, "stale": [11, 12],
            "worst-stale": [(12, 1, 3, 6), (11, 1, 4, 6)],
            "stable-latencies": {0: 0, 0.5: 1, 0.95: 1, 0.99: 1, 1: 1},
            "duplicated-count": 0, "duplicated": {}}
    assert flat_worst(SF.set_full(ops)) == want
    assert SF.set_full(ops, linearizable=True)["valid?"] is False
    cols, time = C.encode(ops)
    assert SN.set_full_cols(cols, time) == want


def test_reversed_completion_known_answer():
    """Reads A, B, C invoked at rows 6, 7, 8 and completed at rows 11, 10, 9;
    times are 2 ms a row.
    1 (in A): last-present 6, last-absent 8 (C, then B must not lower it),
      known row 4 < 8: lost, latency (12 ms + 1 - 8 ms) = 4.
    2 (in C, B): last-present 8 (B must not lower it), last-absent 6, known
      row 5: stable, latency (12 ms + 1 - 10 ms) = 2, stale.
    3 (in C, A): last-present 8 (A must not lower it: with 6 it would be
      below last-absent 7 and the element never-read), known row 9 (the read):
      stable, latency max(14 ms + 1 - 18 ms, 0) = 0.
    4 (in B): last-present 7, last-absent 8 (A must not lower it: with 6 it
      would be stable), known row 10, not before 8: never-read."""
    ops = C.reversed_completion_case()
    want = {"valid?": False, "attempt-count": 4, "stable-count": 2, "lost-count": 1, "lost": [1],
            "never-read-count": 1, "never-read": [4], "stale-count": 1, "stale": [2],
            "worst-stale": [(2, 2, 5, 6)],
            "stable-latencies": {0: 0, 0.5: 2, 0.95: 2, 0.99: 2, 1: 2},
            "lost-latencies": {0: 4, 0.5: 4, 0.95: 4, 0.99: 4, 1: 4},
            "duplicated-count": 0, "duplicated": {}}
    assert flat_worst(SF.set_full(ops)) == want
    cols, time = C.encode(ops)
    assert SN.set_full_cols(cols, time) == want
    assert fold_reads(ops) == {1: (6, 8), 2: (8, 6), 3: (8, 7), 4: (7, 8)}
    assert fold_reads(ops, keep_max=False) == {1: (6, 7), 2: (7, 6), 3: (6, 7), 4: (7, 6)}
