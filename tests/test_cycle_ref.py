"""jepsen.tests.cycle on the CPU: the literal transcriptions (tests/cycle_ref.py)
against the reference's own test data (tests/golden/cycle.json), and
jepsen_amd.cycle's closed forms, region decomposition and result maps against
the transcriptions. No GPU: the checker runs with device=False."""
import json
import os
import random

import numpy as np
import pytest

from conftest import GOLD
from jepsen_amd import _abi as A
from jepsen_amd import cycle as CY
import cycle_ref as R
from cycle_cases import GRAPHS, UNKNOWN_CASES, analyzers_of, checker_raises, random_history, txn_ops, wr_history

G = json.load(open(os.path.join(GOLD, "cycle.json")))
RT_SEEDS = range(60)
WR_SEEDS = range(40)


def int_graph(g):
    return {int(k): v for k, v in g.items()}


def edges_of(g):
    return {(a, b) for a, succ in g.items() for b in succ}


def edge_set(graph):
    return set(map(tuple, graph.edges.tolist()))


def canon(sccs):
    return sorted(sorted(c) for c in sccs)


@pytest.mark.parametrize("case", G["tarjan"], ids=lambda c: c["name"])
def test_golden_tarjan(case):
    g = int_graph(case["graph"])
    n = 1 + max(list(g) + [b for s in g.values() for b in s])
    want = canon(case["sccs"])
    assert canon(R.sccs_of(R.tarjan(n, edges_of(g)))) == want
    assert canon(CY.tarjan(g)) == want


def test_golden_process_graph():
    case = G["process_graph"]
    want = edges_of(int_graph(case["graph"]))
    assert edges_of(R.process_graph(case["history"])) == want
    assert edge_set(CY.process_graph(case["history"])[0]) == want


@pytest.mark.parametrize("case", G["realtime_graph"]["cases"], ids=lambda c: c["name"])
def test_golden_realtime_graph(case):
    ops = G["realtime_graph"]["ops"]
    h = [ops[name] for name in case["history"]]
    pos = {name: i for i, name in enumerate(case["history"])}
    want = {(pos[a], pos[b]) for a, succ in case["graph"].items() for b in succ}
    assert edges_of(R.realtime_graph(h)) == want
    assert edge_set(CY.realtime_graph(h)[0]) == want


def test_golden_ext_index():
    case = G["ext_index"]
    h = [{"type": "ok", "value": case["txns"][name]} for name in case["history"]]
    want = {k: {int(v): [case["history"].index(o) for o in ops] for v, ops in m.items()} for k, m in case["writes"].items()}
    assert R.ext_index(R.ext_writes, h) == want
    got = CY.ext_index(CY.ext_writes, h)
    assert {k: {v: [h.index(o) for o in ops] for v, ops in m.items()} for k, m in got.items()} == want
    assert R.ext_index(R.ext_writes, []) == {} == CY.ext_index(CY.ext_writes, [])


@pytest.mark.parametrize("case", G["wr_graph"]["cases"], ids=lambda c: c["name"])
def test_golden_wr_graph(case):
    h = txn_ops(*case["txns"])
    assert (R.ref_check(h, A.CY_WR)["valid"] == A.VALID) is case["valid?"]
    got = CY.checker(CY.wr_graph, device=False).check({}, h, {})
    assert got["valid?"] is case["valid?"]
    if case["valid?"]:
        assert got == {"valid?": True, "scc-count": 0, "cycles": []}


def test_golden_path_shells_and_find_cycle():
    case = G["path_shells"]
    g = CY.map_to_graph(int_graph(case["graph"]))
    shells = CY.path_shells(g, case["start"])
    assert [next(shells) for _ in case["shells"]] == case["shells"]
    case = G["find_cycle"]
    g = CY.map_to_graph(int_graph(case["graph"]))
    assert CY.find_cycle(g, range(g.n)) == case["cycle"]


def test_manifest_lists_the_fixture():
    man = json.load(open(os.path.join(GOLD, "manifest_cycle.json")))["reference"][0]
    assert man["file"] == "cycle.json"
    got = {"tarjan": len(G["tarjan"]), "realtime_graph": len(G["realtime_graph"]["cases"]), "wr_graph": len(G["wr_graph"]["cases"])}
    assert {s["name"]: s["cases"] for s in man["sections"] if s["name"] in got} == got


# -- the closed forms against the literal loops ----------------------------------------
@pytest.mark.parametrize("seed", RT_SEEDS)
def test_realtime_and_process_closed_forms(seed):
    rng = random.Random(seed)
    h = random_history(seed, rng.randint(1, 6), rng.randint(0, 40), nemesis=False)
    assert edge_set(CY.realtime_graph(h)[0]) == edges_of(R.realtime_graph(h))
    assert edge_set(CY.process_graph(h)[0]) == edges_of(R.process_graph(h))


def test_realtime_unknown_causes():
    a, a2, b = {"process": 0, "type": "invoke"}, {"process": 0, "type": "ok"}, {"process": 1, "type": "invoke"}
    for h, cause, row in (([a, a, a2], A.CAUSE_DOUBLE_INVOKE, 1), ([a, a2, a2], A.CAUSE_ORPHAN, 2),
                          ([a, a2, b], A.CAUSE_UNMATCHED_INVOKE, 2), ([a, a2, b, a, a2], A.CAUSE_UNMATCHED_INVOKE, 2)):
        want = R.ref_check(h, A.CY_REALTIME)
        assert (want["valid"], want["cause"], want["unknown_row"]) == (A.UNKNOWN, cause, row)
        with pytest.raises(CY.IllegalHistory) as e:
            CY.realtime_graph(h)
        assert (e.value.cause, e.value.row) == (A.CAUSES[cause], row)
    # an unmatched invoke before the first :ok is fine
    h = [b, a, a2]
    assert R.ref_check(h, A.CY_REALTIME)["valid"] == A.VALID and len(CY.realtime_graph(h)[0].edges) == 0


@pytest.mark.parametrize("name", list(UNKNOWN_CASES))
def test_unknown_cases_raise_what_the_reference_raises(name):
    """The hand-written unknown histories through the checker on the host: the
    transcription names the cause, the row and the pair; the checker raises
    wr-graph's IllegalArgumentException or an assert of pair-index / link."""
    h, names, cause, row, detail = UNKNOWN_CASES[name]
    mask = sum(getattr(A, "CY_" + n.upper()) for n in names)
    want = R.ref_check(h, mask)
    assert (want["valid"], want["cause"], want["unknown_row"]) == (A.UNKNOWN, cause, row)
    if detail:
        assert (want["unknown_key"], want["unknown_value"], want["unknown_rows"]) == detail
    checker_raises(CY, CY.checker(analyzers_of(CY, names), device=False), name)


@pytest.mark.parametrize("seed", WR_SEEDS)
def test_wr_closed_form_and_result_maps(seed):
    h = wr_history(seed)
    want = R.ref_check(h, A.CY_WR | A.CY_REALTIME)
    chk = CY.checker(CY.combine(CY.wr_graph, CY.realtime_graph), device=False)
    assert want["valid"] != A.UNKNOWN          # written values are fresh per key: UNKNOWN_CASES covers the rest
    hh = [o for o in h if o["process"] != "nemesis"]
    rows = [i for i, o in enumerate(h) if o["process"] != "nemesis"]
    got_edges = {(rows[a], rows[b]) for a, b in edge_set(CY.wr_graph(hh)[0]) | edge_set(CY.realtime_graph(hh)[0])}
    assert got_edges == want["edges"]
    got = chk.check({}, h, {})
    assert got["valid?"] is (want["valid"] == A.VALID) and got["scc-count"] == want["scc_count"]
    assert len(got["cycles"]) == min(want["scc_count"], 8)
    for cyc, scc in zip(got["cycles"], want["sccs"]):
        ops, whys = cyc[0::2], cyc[1::2]
        assert ops[0] == ops[-1] and ops[0]["index"] == scc[0] and {o["index"] for o in ops} <= set(scc)
        assert all(w.startswith("which wrote") or w == "which completed before the invocation of" for w in whys)
        for a, b in zip(ops, ops[1:]):
            assert (a["index"], b["index"]) in want["edges"]


def test_wr_seeds_cover_valid_and_invalid():
    """Of the random wr cases at least a quarter are invalid and a quarter valid
    by the reference alone."""
    kinds = [R.ref_check(wr_history(s), A.CY_WR | A.CY_REALTIME)["valid"] for s in WR_SEEDS]
    assert kinds.count(A.INVALID) * 4 >= len(kinds), kinds
    assert kinds.count(A.VALID) * 4 >= len(kinds), kinds


# -- regions -----------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(80))
def test_region_decomposition_against_tarjan(seed):
    rng = random.Random(seed)
    n = rng.randint(1, 40)
    m = rng.randint(0, 3 * n)
    # mostly forward edges, some back edges, self-loops and repeats
    edges = []
    for _ in range(m):
        a, b = rng.randrange(n), rng.randrange(n)
        if rng.random() < 0.7:
            a, b = min(a, b), max(a, b)
        edges.append((a, b))
    labels = CY.scc_labels(n, edges)
    assert labels.tolist() == R.tarjan(n, edges)
    reg = CY.regions(n, edges)
    for scc in R.sccs_of(labels.tolist()):
        assert any(a <= scc[0] and scc[-1] <= b for a, b in reg.tolist())
    assert all(b > a for a, b in reg.tolist()) and (reg[1:, 0] > reg[:-1, 1]).all()


@pytest.mark.parametrize("name", list(GRAPHS))
def test_hand_written_graphs(name):
    n, edges = GRAPHS[name]
    assert CY.scc_labels(n, edges).tolist() == R.tarjan(n, edges)


def test_region_shapes():
    assert CY.regions(*GRAPHS["regions-stay-two"]).tolist() == [[0, 3], [4, 7]]
    assert CY.regions(*GRAPHS["regions-merge"]).tolist() == [[0, 7]]
    assert CY.regions(*GRAPHS["nested-intervals"]).tolist() == [[0, 9]]
    assert CY.regions(*GRAPHS["chain-no-back-edge"]).tolist() == []
    assert CY.regions(*GRAPHS["only-self-loops"]).tolist() == []
    assert CY.regions(*GRAPHS["trims-to-nothing"]).tolist() == [[1, 3]]


def test_work_cap_arithmetic():
    """JH_CY_WORK_MULT * (V + E): the back-edge chain of k two-cycles costs about
    1.5 k^2 edge visits against a cap of 64 * 5 k: k = 100 stays below it,
    k = 1000 is past it (tests/test_gpu_cycle.py runs both)."""
    for k, past in ((100, False), (1000, True)):
        v, e = 2 * k, 3 * k - 1
        visits = sum(3 * (k - i) for i in range(k)) // 2           # the backward searches alone, a lower bound
        assert (visits > A.CY_WORK_MULT * (v + e)) is past


# -- the explainers ----------------------------------------------------------------
def test_explanations():
    t1, t2 = [["r", "x", 0], ["w", "y", 1]], [["r", "y", 1], ["w", "x", 0]]
    h = txn_ops(t1, t2)
    got = CY.checker(CY.wr_graph, device=False).check({}, h, {})
    o1, o2 = dict(h[1], index=1), dict(h[3], index=3)
    assert got == {"valid?": False, "scc-count": 1,
                   "cycles": [[o1, "which wrote :y = 1, which was read by", o2, "which wrote :x = 0, which was read by", o1]]}
    # process order against a wr edge: a reads what the later b of the same process wrote
    h = [{"process": 0, "type": "ok", "value": [["r", "x", 1]]}, {"process": 0, "type": "ok", "value": [["w", "x", 1]]}]
    got = CY.checker(CY.combine(CY.wr_graph, CY.process_graph), device=False).check({}, h, {})
    a, b = dict(h[0], index=0), dict(h[1], index=1)
    assert got["cycles"] == [[a, "which process 0 completed before", b, "which wrote :x = 1, which was read by", a]]
    # realtime: with :time the reference's string has no space before the seconds and two after
    ex = CY.RealtimeExplainer([{"process": 0, "type": "ok", "index": 0, "time": 1_000_000_000},
                               {"process": 1, "type": "invoke", "index": 1, "time": 1_500_000_000},
                               {"process": 1, "type": "ok", "index": 2, "time": 2_000_000_000}])
    assert ex.explain_pair(ex.history[0], ex.history[2]) == "which completed0.500 seconds  before the invocation of"
    assert ex.explain_pair(ex.history[2], ex.history[0]) is None
    # a :time of 0 is a time (truthy in Clojure), a missing one is not
    ex = CY.RealtimeExplainer([{"process": 0, "type": "ok", "index": 0, "time": 0},
                               {"process": 1, "type": "invoke", "index": 1, "time": 250_000_000},
                               {"process": 1, "type": "ok", "index": 2}])
    assert ex.explain_pair(ex.history[0], ex.history[2]) == "which completed0.250 seconds  before the invocation of"
    del ex.history[0]["time"]
    assert ex.explain_pair(ex.history[0], ex.history[2]) == "which completed before the invocation of"


def test_synth_history_and_its_twin():
    from jepsen_amd import synth
    for anomalies in (0, 3):
        cols = synth.txn_cycle_history(300, 5, 8, anomalies, 0.05, seed=1)
        ops = synth.txn_cycle_columns_to_ops(cols)
        assert len(ops) == cols.n == 600 and len(cols.aux) % 3 == 0
        want = R.ref_check(ops, A.CY_WR | A.CY_REALTIME)
        assert want["valid"] == (A.INVALID if anomalies else A.VALID)
        again = CY.encode(ops)
        ok = np.asarray(cols.type) == A.TYPE_OK
        assert (again.value2[ok] == cols.value2[ok]).all() and (np.asarray(again.process) == cols.process).all()
        got = CY.checker(CY.combine(CY.wr_graph, CY.realtime_graph), device=False).check({}, ops, {})
        assert got["scc-count"] == want["scc_count"]


def test_ctypes_layout_matches_header(tmp_path):
    import ctypes as C
    import subprocess
    from conftest import ROOT
    prog = tmp_path / "sz.c"
    prog.write_text(f'''#include <stdio.h>
#include <stddef.h>
#include "{os.path.join(ROOT, "include", "jh.h")}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(jh_cycle_opts), sizeof(jh_cycle_result), offsetof(jh_cycle_opts, n_extra),
         offsetof(jh_cycle_result, unknown_rows), offsetof(jh_cycle_result, device_ms), JH_CY_LDS_VERTICES, JH_CY_MAX_MOPS,
         JH_CY_WORK_MULT, JH_CAUSE_UNMATCHED_INVOKE);
  return 0; }}''')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(A.JhCycleOpts), C.sizeof(A.JhCycleResult), A.JhCycleOpts.n_extra.offset,
                   A.JhCycleResult.unknown_rows.offset, A.JhCycleResult.device_ms.offset, A.CY_LDS_VERTICES,
                   A.CY_MAX_MOPS, A.CY_WORK_MULT, A.CAUSE_UNMATCHED_INVOKE]
    assert (A.CY_PROCESS, A.CY_REALTIME, A.CY_WR) == (1, 2, 4)


def test_encode_refuses_what_has_no_encoding():
    with pytest.raises(TypeError):
        CY.encode(txn_ops([["r", "x", "a string"]]))
    with pytest.raises(TypeError):
        CY.encode(txn_ops([["append", "x", 1]]))
    c = CY.encode(txn_ops([["r", "x", None], ["w", "y", 2]]))
    assert c.aux.tolist() == [A.F_READ, 0, A.NIL, A.F_WRITE, 1, 2] and c.value[1] == 0 and c.value2[1] == 2
    assert c.keys == ["x", "y"] and np.asarray(c.process).tolist() == [0, 0]
