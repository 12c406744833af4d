"""monotonic-key-graph on the host: the goldens of the reference's test file
through the naive restatement (tests/cycle_mono_ref.py), through
monotonic_key_graph and through the checker with device=False; the numpy closed
form of jepsen_amd.cycle against the restatement on seeded histories; the
verdicts of healthy and stale histories; the encoding; the ABI constants."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD
from jepsen_amd import _abi as A
from jepsen_amd import cycle as CY
import cycle_mono_ref as R
from cycle_mono_cases import NEM, groups, ok, random_mono_history, row, seeded

G = json.load(open(os.path.join(GOLD, "cycle_mono.json")))
MO, RT, PR = 32, A.CY_REALTIME, A.CY_PROCESS
N_SEEDS = 320
EMPTY = {"valid?": True, "scc-count": 0, "cycles": []}


def hist(case):
    return [dict(op) for op in case["history"]]


def rotations(cycle):
    """[op why op ... op] -> every rotation of the closed walk."""
    steps = list(zip(cycle[0:-1:2], cycle[1::2]))
    out = []
    for i in range(len(steps)):
        rot = steps[i:] + steps[:i]
        out.append([x for s in rot for x in s] + [rot[0][0]])
    return out


def test_manifest_lists_the_fixture():
    man = json.load(open(os.path.join(GOLD, "manifest_cycle_mono.json")))["reference"][0]
    assert man["file"] == "cycle_mono.json"
    assert {s["name"]: s["cases"] for s in man["sections"]} == {"graphs": 2, "checker": 2, "monotonic_process": 1}
    assert all(len(G[s["name"]]) == s["cases"] for s in man["sections"])


@pytest.mark.parametrize("case", G["graphs"], ids=lambda c: c["name"])
def test_golden_graphs(case):
    h = hist(case)
    want = {int(a): succ for a, succ in case["graph"].items()}
    assert {a: sorted(s) for a, s in sorted(R.graph(h).items())} == want
    g, ex = CY.monotonic_key_graph(h)
    assert g.to_map() == want and isinstance(ex, CY.MonotonicKeyExplainer)


@pytest.mark.parametrize("case", G["checker"], ids=lambda c: c["name"])
def test_golden_checker(case):
    h = hist(case)
    assert CY.checker(CY.monotonic_key_graph, device=False).check({}, h, {}) == case["result"]
    assert (R.ref_check_mono(h, MO)["valid"] == A.VALID) is case["result"]["valid?"]
    for ours, theirs in zip(case["result"]["cycles"], case.get("reference_cycles", ())):
        assert theirs in rotations(ours) and theirs != ours


def test_golden_monotonic_and_process():
    case = G["monotonic_process"][0]
    h = hist(case)
    both = CY.combine(CY.monotonic_key_graph, CY.process_graph)
    want = {int(a): succ for a, succ in case["graph"].items()}
    assert both(h)[0].to_map() == want
    assert R.ref_check_mono(h, MO | PR)["edges"] == {(a, b) for a, succ in want.items() for b in succ}
    assert CY.checker(CY.monotonic_key_graph, device=False).check({}, h, {}) == case["monotonic_result"]
    assert CY.checker(CY.process_graph, device=False).check({}, h, {}) == case["process_result"]
    assert CY.checker(both, device=False).check({}, h, {}) == case["combined_result"]
    assert case["reference_cycles"][0] in rotations(case["combined_result"]["cycles"][0])
    assert both.analyzers == MO | PR


def test_explainer():
    ex = CY.MonotonicKeyExplainer()
    a, b = {"value": {"x": 1, "y": None, "z": 2}}, {"value": {"y": 3, "z": 5, "x": 1}}
    assert ex.explain_pair(a, b) == "which observed :z = 2, and a higher value 5 was observed by"
    assert ex.explain_pair(b, a) is None and ex.explain_pair({"value": None}, b) is None
    assert ex.explain_pair({"value": {("x",): 0}}, {"value": {("x",): 7}}) == \
        f"which observed {CY.pr_str(('x',))} = 0, and a higher value 7 was observed by"
    assert CY._explainer_for(CY.monotonic_key_graph, []).__class__ is CY.MonotonicKeyExplainer


def host_edges(h):
    rows = [i for i, op in enumerate(h) if op.get("process") != "nemesis"]
    return sorted((rows[a], rows[b]) for a, b in CY.monotonic_key_edges([h[i] for i in rows]).tolist())


def test_closed_form_against_the_restatement():
    """The same multiset of edges, one per link call, on N_SEEDS seeded histories."""
    n_edges = 0
    for seed in range(N_SEEDS):
        h = seeded(seed)
        rows = [i for i, op in enumerate(h) if op.get("process") != "nemesis"]
        want = sorted((rows[a], rows[b]) for a, b in R.links([h[i] for i in rows]))
        assert host_edges(h) == want, seed
        n_edges += len(want)
    assert n_edges > 10 * N_SEEDS


def test_closed_form_on_hand_shapes():
    for h in (groups(1, 1), groups(3, 2, 4), groups(5), [ok({"x": None}), ok({"x": -3}), ok({"x": None, "y": 2}), ok({"y": 2})],
              [ok({"x": 0, "y": 0}, p=1), row("fail", {"x": 1}), row("info", {"x": 1}), row("invoke", {"x": 1}), ok({"y": 1, "x": 4})],
              [ok(None), ok({})], []):
        assert host_edges(h) == sorted(R.links(h))
    # the same two rows through two keys: twice
    assert host_edges([ok({"x": 0, "y": 0}), ok({"x": 1, "y": 1})]) == [(0, 1), (0, 1)]
    # nil sorts first; a nemesis :ok row is ignored
    assert host_edges([ok({"x": 0}), ok({"x": None}), dict(NEM, type="ok", value={"x": 1})]) == [(1, 0)]
    # values that are no longs: Python's order; a key of mixed types raises
    assert host_edges([ok({"x": "b"}), ok({"x": "a"}), ok({"x": None})]) == [(1, 0), (2, 1)]
    assert host_edges([ok({"x": 1.5}), ok({"x": 1})]) == [(1, 0)]
    with pytest.raises(TypeError):
        CY.monotonic_key_edges([ok({"x": "a"}), ok({"x": 1})])
    with pytest.raises(TypeError):
        CY.monotonic_key_edges([ok([["r", "x", 1]])])


def test_healthy_histories_are_valid_and_stale_ones_are_not():
    stale_invalid = 0
    for seed in range(30):
        healthy, stale = random_mono_history(seed), random_mono_history(seed, stale=0.3)
        for mask, fn in (MO, CY.monotonic_key_graph), (MO | RT, CY.combine(CY.monotonic_key_graph, CY.realtime_graph)):
            want = R.ref_check_mono(healthy, mask)
            assert want["cause"] == 0 and want["valid"] == A.VALID, (seed, mask)
            assert CY.checker(fn, device=False).check({}, healthy, {}) == EMPTY, (seed, mask)
        want = R.ref_check_mono(stale, MO | RT)
        got = CY.checker(CY.combine(CY.monotonic_key_graph, CY.realtime_graph), device=False).check({}, stale, {})
        assert got["valid?"] is (want["valid"] == A.VALID) and got["scc-count"] == want["scc_count"], seed
        stale_invalid += want["valid"] == A.INVALID
    assert stale_invalid >= 10


def test_encode_map_round_trip_and_refusals():
    h = [dict(NEM), row("invoke", None, f="inc"), ok({"x": 3}), ok(None), ok({}), ok({("x", "y"): None, "x": -7}), row("fail", {"x": 1}),
         row("info", [1, 2]), dict(NEM, type="ok", value={"x": 9})]
    c = CY.encode_map(h)
    assert c.n == 9 and c.keys == ["x", ("x", "y")] and len(c.aux) == 6
    assert c.value2.tolist() == [0, 0, 1, 0, 0, 2, 0, 0, 0] and c.value[2] == 0 and c.value[5] == 1
    assert c.aux.tolist() == [0, 3, 1, A.NIL, 0, -7]
    back = [{c.keys[k]: (None if v == A.NIL else v) for k, v in c.aux[2 * c.value[i]:2 * (c.value[i] + c.value2[i])].reshape(-1, 2).tolist()}
            for i in range(c.n) if c.value2[i]]
    assert back == [h[2]["value"], h[5]["value"]]
    e = CY.encode_map([])
    assert e.n == 0 and len(e.aux) == 0
    for bad in ([["r", "x", 1]], 5, "s", {"x": "s"}, {"x": 1.5}, {"x": A.NIL}, {"x": 1 << 63}):
        with pytest.raises(TypeError):
            CY.encode_map([ok(bad)])
    from jepsen_amd import synth
    cols = synth.monotonic_history(300, 5, 3, 0.5, 0.0, 0.05, seed=3)
    ops = synth.monotonic_columns_to_ops(cols)
    c2 = CY.encode_map(ops)
    assert sorted(map(tuple, CY.map_edges(cols).tolist())) == sorted(map(tuple, CY.map_edges(c2).tolist())) == sorted(R.links(ops))
    # (encode_map interns the keys in first-appearance order, the generator numbers them: the maps are the same)
    assert [op["value"] for op in synth.monotonic_columns_to_ops(c2)] == [op["value"] for op in ops]
    assert c2.value2.tolist() == np.asarray(cols.value2).tolist() and len(c2.aux) == len(cols.aux)
    assert c2.process.tolist() == np.asarray(cols.process).tolist() and c2.type.tolist() == np.asarray(cols.type).tolist()


def test_synth_monotonic_history():
    """Healthy histories are valid under every combination, stale ones are not,
    every invoke is completed, and p_read gives the chain and the wide shapes."""
    from jepsen_amd import synth
    for stale in (0.0, 0.3):
        ops = synth.monotonic_columns_to_ops(synth.monotonic_history(400, 5, 3, 0.5, stale, 0.05, seed=2))
        assert sum(op["type"] == "invoke" for op in ops) == 400 == len(ops) // 2 and any(op["type"] == "info" for op in ops)
        for mask in (MO, MO | RT, MO | RT | PR):
            want = R.ref_check_mono(ops, mask)
            assert want["cause"] == 0 and (stale or want["valid"] == A.VALID), (stale, mask)
            assert not stale or mask == MO or want["valid"] == A.INVALID, mask
    chain = synth.monotonic_columns_to_ops(synth.monotonic_history(200, 4, 2, 0.0, 0.0, 0.0, seed=1))
    assert len(CY.monotonic_key_edges(chain)) == 200 - 2
    wide = synth.monotonic_columns_to_ops(synth.monotonic_history(400, 4, 1, 0.98, 0.0, 0.0, seed=1))
    assert len(CY.monotonic_key_edges(wide)) > 20 * 400


def test_memory_error_before_any_allocation():
    """Two groups of 46 341 rows: 46 341^2 = 2 147 488 281 > 2^31 - 2 link calls."""
    import tracemalloc
    h = [ok({"x": 0})] * 46341 + [ok({"x": 1})] * 46341
    tracemalloc.start()
    with pytest.raises(MemoryError) as e:
        CY.monotonic_key_edges(h)
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    assert "2147488281" in str(e.value)
    assert peak < 64 << 20                      # the edges alone would be 34 GB


def test_abi_constants_and_struct_sizes(tmp_path):
    """JH_CY_MONOTONIC and its neighbours equal _abi's; the structs keep their sizes and offsets; the ABI stays 8."""
    from conftest import ROOT
    prog = tmp_path / "sz.c"
    prog.write_text(f'''#include <stdio.h>
#include <stddef.h>
#include "{os.path.join(ROOT, "include", "jh.h")}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %d %d %d %d %d %d %d\\n", sizeof(jh_cycle_opts), sizeof(jh_cycle_result),
         offsetof(jh_cycle_opts, n_extra), offsetof(jh_cycle_result, edge_count), offsetof(jh_cycle_result, entries),
         JH_CY_MONOTONIC, JH_CY_APPEND, JH_CY_WR, JH_CY_REALTIME, JH_CY_PROCESS, JH_CY_MAX_MOPS, JH_ABI_VERSION);
  return 0; }}''')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(A.JhCycleOpts), C.sizeof(A.JhCycleResult), A.JhCycleOpts.n_extra.offset,
                   A.JhCycleResult.edge_count.offset, A.JhCycleResult.entries.offset, A.CY_MONOTONIC, A.CY_APPEND, A.CY_WR,
                   A.CY_REALTIME, A.CY_PROCESS, A.CY_MAX_MOPS, 8]
    assert got[:2] == [64, 152] and A.CY_MONOTONIC == 32 and CY.monotonic_key_graph.analyzers == 32


def test_checker_routes_without_a_device(monkeypatch):
    """MONOTONIC with WR or APPEND goes to the host, as does device=False and a map that does not encode."""
    from jepsen_amd import checker as K

    def no_device():
        raise AssertionError("the device was asked")
    monkeypatch.setattr(K, "_ctx", no_device)
    h = [ok({"x": 1}), ok({"x": 0})]
    for other in (CY.wr_graph, CY.appends_and_reads_graph):
        both = CY.combine(CY.monotonic_key_graph, other)
        assert both.analyzers & MO and both.analyzers & (A.CY_WR | A.CY_APPEND)
        assert CY.checker(both).check({}, [ok(None), ok(None, p=1)], {}) == EMPTY
    assert CY.checker(CY.monotonic_key_graph, device=False).check({}, h, {}) == EMPTY
    out = CY.checker(CY.combine(CY.monotonic_key_graph, CY.process_graph)).check({}, [ok({"x": "b"}), ok({"x": "a"})], {})
    assert out["valid?"] is False and out["cycles"][0][1::2] == ["which process 0 completed before",
                                                                 "which observed :x = :a, and a higher value :b was observed by"]
    with pytest.raises(AssertionError):
        CY.checker(CY.monotonic_key_graph).check({}, h, {})
