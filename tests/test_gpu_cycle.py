"""jepsen.tests.cycle on the device (jh_scc, jh_check_cycle, jh_cycle.hip)
against the literal transcriptions of tests/cycle_ref.py: labels_out (the whole
partition), the counts, the SCC lists and set(edges_out), exactly. Every case
runs on auto and on both forced tiers where its largest region fits the on-chip
tier. Everything is integer, so every comparison is exact."""
import json
import os
import random

import numpy as np
import pytest

from conftest import GOLD
from jepsen_amd import _abi as A
from jepsen_amd import _native
from jepsen_amd import cycle as CY
import cycle_ref as R
from cycle_cases import (GRAPHS, N, UNKNOWN_CASES, analyzers_of, chain_of_cycles, checker_raises, done, inv, random_history,
                         txn_ops)

pytestmark = pytest.mark.gpu

G = json.load(open(os.path.join(GOLD, "cycle.json")))
ALL = A.CY_PROCESS | A.CY_REALTIME | A.CY_WR


def paths_for(n, edges):
    reg = CY.regions(n, edges)
    big = len(reg) and int((reg[:, 1] - reg[:, 0] + 1).max()) > N
    return (A.CY_PATH_AUTO, A.CY_PATH_GLOBAL) if big else (A.CY_PATH_AUTO, A.CY_PATH_LDS, A.CY_PATH_GLOBAL)


def same_partition(r, want, path):
    assert r["labels"].tolist() == want["labels"], path
    assert (r["valid"], r["scc_count"], r["scc_vertices"]) == (want["valid"], want["scc_count"], want["scc_vertices"]), path
    assert r["sccs"] == want["sccs"], path


def agree_scc(ctx, n, edges):
    edges = list(edges)
    want = R.scc_answer(n, edges)
    reg = CY.regions(n, edges)
    src, dst = [a for a, _ in edges], [b for _, b in edges]
    for path in paths_for(n, edges):
        r = ctx.scc(n, src, dst, path, scc_cap=max(want["scc_count"], 1))
        same_partition(r, want, path)
        assert r["back_edges"] == want["back_edges"] and r["edge_count"] == [0, 0, 0, len(edges)], path
        assert r["regions"] == len(reg) and r["max_region"] == (int((reg[:, 1] - reg[:, 0] + 1).max()) if len(reg) else 0)
        glob = int(((reg[:, 1] - reg[:, 0] + 1) > N).sum()) if path != A.CY_PATH_GLOBAL else len(reg)
        assert r["global_regions"] == glob and r["path"] == (0 if not len(reg) else 2 if glob else 1), path
    return want


def agree(ctx, history, analyzers, extra=None):
    want = R.ref_check(history, analyzers, list(zip(*extra)) if extra else ())
    cols = CY.encode(history, txns=bool(analyzers & A.CY_WR))
    paths = (0, 1, 2) if want["valid"] == A.UNKNOWN else paths_for(len(history), sorted(want["edges"]))
    for path in paths:
        r = ctx.check_cycle(cols, analyzers, path, extra, scc_cap=max(want.get("scc_count", 0), 1), edge_cap=1 << 16)
        assert (r["valid"], r["cause"], r["unknown_row"], r["unknown_rows"]) == \
            (want["valid"], want["cause"], want["unknown_row"], want["unknown_rows"]), path
        if want["valid"] == A.UNKNOWN:
            key = cols.keys[r["unknown_key"]] if r["unknown_key"] != A.NIL else None
            value = None if r["unknown_value"] == A.NIL else r["unknown_value"]
            assert (key, value) == (want["unknown_key"], want["unknown_value"]), path
            continue
        same_partition(r, want, path)
        got = list(map(tuple, r["edges"].tolist()))
        assert set(got) == want["edges"] and r["edge_count"] == want["edge_count"] and len(got) == sum(r["edge_count"]), path
        assert r["back_edges"] == sum(1 for a, b in got if b < a), path
    return want


# -- jh_scc ------------------------------------------------------------------------
@pytest.mark.parametrize("case", G["tarjan"], ids=lambda c: c["name"])
def test_scc_golden_tarjan(ctx, case):
    g = {int(k): v for k, v in case["graph"].items()}
    n = 1 + max(list(g) + [b for s in g.values() for b in s])
    want = agree_scc(ctx, n, [(a, b) for a, s in g.items() for b in s])
    assert sorted(want["sccs"]) == sorted(sorted(c) for c in case["sccs"])


@pytest.mark.parametrize("name", list(GRAPHS))
def test_scc_edge_shapes(ctx, name):
    n, edges = GRAPHS[name]
    want = agree_scc(ctx, n, edges)
    if name.startswith("ring"):
        assert want["sccs"] == [list(range(n))]
    if name == "two-sccs-trivial-between":
        assert want["sccs"] == [[1, 2], [3, 4]] and want["labels"][0] == -1
    if name == "two-cycles-63-64-255-256":
        assert want["sccs"] == [[63, 64], [255, 256]]


@pytest.mark.parametrize("seed", range(6))
def test_scc_random_graphs(ctx, seed):
    rng = random.Random(seed)
    n = rng.choice([1, 2, 50, 700, 3000])
    edges = []
    for _ in range(rng.randint(0, 3 * n)):
        a = rng.randrange(n)
        b = min(n - 1, max(0, a + rng.randint(-6, 30)))
        edges.append((a, b))
    agree_scc(ctx, n, edges)


def test_scc_caps_and_empty(ctx):
    n, edges = GRAPHS["two-cycles-63-64-255-256"]
    src, dst = zip(*edges)
    r = ctx.scc(n, src, dst, scc_cap=1)
    assert r["scc_count"] == 2 and r["sccs"] == [[63, 64]]
    r = ctx.scc(n, src, dst, scc_cap=2, rows_cap=3)
    assert r["scc_count"] == 2 and r["scc_vertices"] == 4 and r["sccs"] == [[63, 64]]
    r = ctx.scc(0, [], [])
    assert (r["valid"], r["scc_count"], r["path"]) == (A.VALID, 0, 0)
    r = ctx.scc(5, [], [])
    assert r["labels"].tolist() == [-1] * 5 and r["regions"] == 0


def test_work_cap(ctx):
    """The back-edge chain of 1000 two-cycles passes JH_CY_WORK_MULT * (V + E)
    (tests/test_cycle_ref.py has the arithmetic); 100 of them do not."""
    for path in (A.CY_PATH_AUTO, A.CY_PATH_GLOBAL):
        with pytest.raises(_native.JhError) as e:
            ctx.scc(2000, *zip(*chain_of_cycles(1000)), path)
        assert e.value.code == A.JH_EUNSUPPORTED
    assert agree_scc(ctx, 200, chain_of_cycles(100))["scc_count"] == 100


# -- realtime and process ------------------------------------------------------------
@pytest.mark.parametrize("case", G["realtime_graph"]["cases"], ids=lambda c: c["name"])
def test_realtime_golden(ctx, case):
    ops = G["realtime_graph"]["ops"]
    h = [ops[name] for name in case["history"]]
    pos = {name: i for i, name in enumerate(case["history"])}
    want = agree(ctx, h, A.CY_REALTIME)
    assert want["edges"] == {(pos[a], pos[b]) for a, succ in case["graph"].items() for b in succ}


def test_empty_history(ctx):
    """n = 0 through jh_check_cycle itself, every analyzer mask and path."""
    for txns, mask in ((False, A.CY_REALTIME), (False, A.CY_PROCESS), (True, A.CY_WR), (True, ALL)):
        cols = CY.encode([], txns=txns)
        assert cols.n == 0
        for path in (A.CY_PATH_AUTO, A.CY_PATH_LDS, A.CY_PATH_GLOBAL):
            r = ctx.check_cycle(cols, mask, path, edge_cap=4)
            assert (r["valid"], r["cause"], r["path"], r["unknown_row"]) == (A.VALID, 0, 0, -1), (mask, path)
            assert (r["scc_count"], r["scc_vertices"], r["back_edges"], r["regions"], r["max_region"], r["global_regions"],
                    r["entries"]) == (0,) * 7
            assert r["edge_count"] == [0, 0, 0, 0] and r["labels"].tolist() == [] and r["sccs"] == []
            assert r["edges"].tolist() == []
    for fn in (CY.realtime_graph, CY.wr_graph):
        assert CY.checker(fn).check({}, [], {}) == {"valid?": True, "scc-count": 0, "cycles": []}


def test_process_golden(ctx):
    want = agree(ctx, G["process_graph"]["history"], A.CY_PROCESS)
    assert want["edges"] == {(0, 3), (1, 2)}


def test_realtime_shapes(ctx):
    a, a2, b, b2 = inv(0), done(0, "ok"), inv(1), done(1, "ok")
    nem = {"process": "nemesis", "type": "info", "f": "start", "value": None}
    # an :ok on the last row; :info and :fail completions as edge targets; nemesis rows between
    agree(ctx, [a, a2, b, b2], A.CY_REALTIME)
    want = agree(ctx, [a, a2, nem, b, inv(2), nem, done(1, "info"), done(2, "fail"), inv(3), done(3, "ok")], A.CY_REALTIME)
    assert {(1, 6), (1, 7), (1, 9)} <= want["edges"]
    # an unmatched invoke before the first :ok is fine, one after it is unknown
    assert agree(ctx, [b, a, a2], A.CY_REALTIME)["valid"] == A.VALID
    for h, cause, row in (([a, a2, b], A.CAUSE_UNMATCHED_INVOKE, 2), ([a, a2, b, a, a2], A.CAUSE_UNMATCHED_INVOKE, 2),
                          ([a, a, a2], A.CAUSE_DOUBLE_INVOKE, 1), ([a, a2, a2], A.CAUSE_ORPHAN, 2),
                          ([a, a2, done(1, "fail")], A.CAUSE_ORPHAN, 2)):
        want = agree(ctx, h, A.CY_REALTIME)
        assert (want["valid"], want["cause"], want["unknown_row"]) == (A.UNKNOWN, cause, row)
    # an :info without an invoke stays unpaired
    assert agree(ctx, [a, a2, done(5, "info"), b, b2], A.CY_REALTIME)["edges"] == {(1, 4)}


@pytest.mark.parametrize("seed", range(12))
def test_realtime_random(ctx, seed):
    rng = random.Random(seed)
    agree(ctx, random_history(seed, rng.randint(1, 6), rng.randint(1, 60)), A.CY_REALTIME | A.CY_PROCESS)


# -- wr ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G["wr_graph"]["cases"], ids=lambda c: c["name"])
def test_wr_golden(ctx, case):
    h = txn_ops(*case["txns"])
    assert (agree(ctx, h, A.CY_WR)["valid"] == A.VALID) is case["valid?"]
    for path in (0, 1, 2):
        got = CY.checker(CY.wr_graph, path=path).check({}, h, {})
        assert got == CY.checker(CY.wr_graph, device=False).check({}, h, {}) and got["valid?"] is case["valid?"]


def test_wr_shapes(ctx):
    # a self-reading txn: a self-loop, kept in the edges, changing nothing
    want = agree(ctx, txn_ops([["r", "x", 1], ["w", "x", 1]]), A.CY_WR)
    assert want["edges"] == {(1, 1)} and want["valid"] == A.VALID
    # nil is a value like any other
    want = agree(ctx, txn_ops([["w", "x", None]], [["r", "x", None]]), A.CY_WR)
    assert want["edges"] == {(1, 3)}
    # a first micro-op that is a write masks a later read; the last write wins
    want = agree(ctx, txn_ops([["w", "x", 1], ["w", "x", 2]], [["w", "y", 5], ["r", "y", 9], ["r", "x", 1]],
                              [["r", "x", 2]], [["w", "y", 9]]), A.CY_WR)
    assert want["edges"] == {(1, 5)}
    # two writers that are read: unknown, every unknown_* field; never read: valid
    t = [[["w", "x", 1]], [["r", "y", 0], ["r", "x", 1]], [["w", "x", 1], ["w", "x", 3], ["w", "x", 1]], [["r", "x", 1]]]
    want = agree(ctx, txn_ops(*t), A.CY_WR)
    assert (want["cause"], want["unknown_row"], want["unknown_key"], want["unknown_value"], want["unknown_rows"]) == \
        (A.CAUSE_MULTIPLE_WRITES, 3, "x", 1, [1, 5])
    assert agree(ctx, txn_ops(t[0], t[2], [["r", "x", 7]]), A.CY_WR)["valid"] == A.VALID


@pytest.mark.parametrize("n_txns,healthy", [(257, True), (257, False), (1025, True), (1025, False)])
def test_wr_random(ctx, n_txns, healthy):
    h = random_history(n_txns, 7, 2 * n_txns, txns=True, healthy=healthy, n_keys=16)
    want = agree(ctx, h, ALL)
    assert want["valid"] != A.UNKNOWN and (want["valid"] == A.VALID) is healthy


def test_wr_and_realtime_combined(ctx):
    w, r = [["w", "x", 1]], [["r", "x", 1]]
    # the reader completes before its writer is invoked: one SCC
    h = [inv(0, r), done(0, "ok", r), inv(1, w), done(1, "ok", w)]
    want = agree(ctx, h, A.CY_WR | A.CY_REALTIME)
    assert want["sccs"] == [[1, 3]]
    got = CY.checker(CY.combine(CY.wr_graph, CY.realtime_graph)).check({}, h, {})
    assert got == CY.checker(CY.combine(CY.wr_graph, CY.realtime_graph), device=False).check({}, h, {})
    assert got["cycles"][0][1::2] == ["which completed before the invocation of", "which wrote :x = 1, which was read by"]
    # the same pair overlapping in time: valid
    assert agree(ctx, [inv(0, r), inv(1, w), done(0, "ok", r), done(1, "ok", w)], A.CY_WR | A.CY_REALTIME)["valid"] == A.VALID


def test_extra_edges(ctx):
    h = [inv(0), done(0, "ok"), inv(1), done(1, "ok")]
    assert agree(ctx, h, A.CY_REALTIME)["valid"] == A.VALID
    assert agree(ctx, h, A.CY_REALTIME, ([3], [1]))["sccs"] == [[1, 3]]
    assert agree(ctx, h, 0, ([3, 1], [1, 3]))["sccs"] == [[1, 3]]


# -- return codes --------------------------------------------------------------------
def code_of(fn):
    with pytest.raises(_native.JhError) as e:
        fn()
    return e.value.code


def test_return_codes(ctx):
    ok = CY.encode(txn_ops([["r", "x", 1], ["w", "y", 2]]))

    def with_(**kw):
        c = CY.encode(txn_ops([["r", "x", 1], ["w", "y", 2]]))
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    assert ctx.check_cycle(ok, A.CY_WR)["valid"] == A.VALID
    # JH_EUNSUPPORTED: another micro-op f; more than JH_CY_MAX_MOPS micro-ops
    assert code_of(lambda: ctx.check_cycle(with_(aux=np.array([7, 0, 1, 1, 1, 2], np.int64)), A.CY_WR)) == A.JH_EUNSUPPORTED
    many = [["w", i, i] for i in range(A.CY_MAX_MOPS + 1)]
    assert ctx.check_cycle(CY.encode(txn_ops(many[:-1])), A.CY_WR)["entries"] == A.CY_MAX_MOPS
    assert code_of(lambda: ctx.check_cycle(CY.encode(txn_ops(many)), A.CY_WR)) == A.JH_EUNSUPPORTED
    # JH_EINVAL: ranges, counts, n_aux, endpoints, no analyzer, forced on-chip path
    for value, value2 in ((1, 2), (0, 3), (-1, 1), (0, -1)):
        c = with_(value=np.array([A.NIL, value], np.int64), value2=np.array([0, value2], np.int64))
        assert code_of(lambda: ctx.check_cycle(c, A.CY_WR)) == A.JH_EINVAL, (value, value2)
    assert code_of(lambda: ctx.check_cycle(with_(aux=np.zeros(7, np.int64)), A.CY_WR)) == A.JH_EINVAL
    for extra in (([2], [0]), ([0], [-1])):
        assert code_of(lambda: ctx.check_cycle(ok, A.CY_WR, extra=extra)) == A.JH_EINVAL
    assert code_of(lambda: ctx.check_cycle(ok, 0)) == A.JH_EINVAL
    assert code_of(lambda: ctx.check_cycle(ok, 8)) == A.JH_EINVAL
    assert code_of(lambda: ctx.check_cycle(ok, A.CY_WR, path=3)) == A.JH_EINVAL
    assert code_of(lambda: ctx.scc(3, [0], [3])) == A.JH_EINVAL
    n, edges = GRAPHS["ring-N+1"]
    assert code_of(lambda: ctx.scc(n, *zip(*edges), A.CY_PATH_LDS)) == A.JH_EINVAL
    # more than 2^31 - 2 vertices: refused before any buffer of that size is made
    assert code_of(lambda: ctx.scc((1 << 31) - 1, [], [], want_labels=False)) == A.JH_EUNSUPPORTED


def test_checker_module_on_device(ctx):
    """The checker's maps through jh_check_cycle equal the host implementation's."""
    for seed in (3, 4, 5):
        h = random_history(seed, 4, 50, txns=True, healthy=False)
        fn = CY.combine(CY.wr_graph, CY.realtime_graph, CY.process_graph)
        want = CY.checker(fn, device=False).check({}, h, {})
        assert want["scc-count"] > 0
        for path in (0, 1, 2):
            assert CY.checker(fn, path=path).check({}, h, {}) == want


@pytest.mark.parametrize("name", list(UNKNOWN_CASES))
def test_unknown_cases_raise_what_the_reference_raises(ctx, name):
    """A JH_UNKNOWN result becomes what the reference raises, through the
    checker on every path: the raw fields first, then the exception."""
    h, names, cause, row, detail = UNKNOWN_CASES[name]
    want = agree(ctx, h, sum(getattr(A, "CY_" + n.upper()) for n in names))
    assert (want["valid"], want["cause"], want["unknown_row"]) == (A.UNKNOWN, cause, row)
    for path in (0, 1, 2):
        checker_raises(CY, CY.checker(analyzers_of(CY, names), path=path), name)
