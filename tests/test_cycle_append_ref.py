"""appends-and-reads-graph on the host: the goldens of the reference's test file
through the literal transcription (tests/cycle_append_ref.py) and through the
checker with device=False; the numpy closed forms of jepsen_amd.cycle against
the transcription on seeded histories that reach every cause; the encoding."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD
from jepsen_amd import _abi as A
from jepsen_amd import cycle as CY
import cycle_append_ref as R
from cycle_append_cases import NEM, all_causes, ap, long_read_history, ok, r, row, seeded

G = json.load(open(os.path.join(GOLD, "cycle_append.json")))
N_SEEDS = 360


def named(case):
    return [dict(G["ops"][name]) for name in case["history"]]


def test_manifest_lists_the_fixture():
    man = json.load(open(os.path.join(GOLD, "manifest_cycle_append.json")))["reference"][0]
    assert man["file"] == "cycle_append.json"
    for sec in man["sections"]:
        assert len(G[sec["name"]]) == sec["cases"] if sec["name"] != "checker" else sec["cases"] == 1
    assert len(G["cases"]) == 10 and len(G["errors"]) == 3


@pytest.mark.parametrize("case", G["cases"], ids=lambda c: c["name"])
def test_golden_graphs(case):
    h = named(case)
    pos = {name: i for i, name in enumerate(case["history"])}
    want = {pos[a]: sorted(pos[b] for b in succ) for a, succ in case["graph"].items()}
    assert {a: sorted(s) for a, s in R.graph(h).items()} == want
    g, ex = CY.appends_and_reads_graph(h)
    assert g.to_map() == want and ex.explain_pair(None, None) == "something something"


def golden_error(case):
    want = {k: case[k] for k in ("type", "op", "key", "value", "errors") if k in case}
    if "duplicates" in case:
        want["duplicates"] = {int(k): v for k, v in case["duplicates"].items()}
    return want


@pytest.mark.parametrize("case", G["errors"], ids=lambda c: c["name"])
def test_golden_errors(case):
    h = [dict(op) for op in case["history"]]
    hi = [op if "index" in op else dict(op, index=i) for i, op in enumerate(h)]
    want = golden_error(case)
    with pytest.raises(R.Thrown) as e:
        R.graph(hi)
    assert {k: e.value.m[k] for k in want} == want
    with pytest.raises(CY.AnalysisMap) as e2:
        CY.appends_and_reads_graph(hi)
    assert {k: e2.value.map[k] for k in want} == want and e2.value.map == e.value.m


def test_golden_checker_map():
    h = [dict(op) for op in G["checker"]["history"]]
    assert CY.checker(CY.appends_and_reads_graph, device=False).check({}, h, {}) == G["checker"]["result"]


def host_answer(h, analyzers=None):
    """What the numpy closed forms give, in ref_check_append's terms."""
    rows = [i for i, op in enumerate(h) if op.get("process") != "nemesis"]
    hh = [h[i] for i in rows]
    try:
        g, _ = CY.appends_and_reads_graph(hh)
    except CY.AnalysisMap as e:
        return {"map": e.map}
    except CY.IllegalHistory as e:
        return {"cause": A.CAUSE_NO_WRITER, "unknown_row": rows[e.row], "mop": e.mop, "value": e.value}
    return {"edges": sorted((rows[a], rows[b]) for a, b in g.edges.tolist())}


def test_closed_forms_against_the_transcription():
    """Identical edge multisets and identical first failures on N_SEEDS seeded
    histories (healthy, stale, mutated); every cause 13-16 is reached."""
    reached = {}
    for seed in range(N_SEEDS):
        h = seeded(seed)
        want, got = R.ref_check_append(h, A.CY_APPEND), host_answer(h)
        reached[want["cause"]] = reached.get(want["cause"], 0) + 1
        if want["cause"] == A.CAUSE_NO_WRITER:
            assert (got["cause"], got["unknown_row"], got["mop"]) == (want["cause"], want["unknown_row"], want["unknown_rows"][0]), seed
            assert got["value"] == want["unknown_value"], seed
        elif want["cause"]:
            assert got["map"] == want["map"], seed
        else:
            # the multiset: one edge per link call
            rows = [i for i, op in enumerate(h) if op.get("process") != "nemesis"]
            links = []
            R.graph([h[i] for i in rows], links)
            assert set(got["edges"]) == want["edges"] and len(got["edges"]) == links[0] == want["edge_count"][2], seed
            chk = CY.checker(CY.appends_and_reads_graph, device=False).check({}, h, {})
            assert chk["valid?"] is (want["valid"] == A.VALID) and chk["scc-count"] == want["scc_count"], seed
    assert all(reached.get(c, 0) >= 3 for c in (0, 13, 14, 15, 16)), reached


def test_stale_reads_give_cycles_and_healthy_ones_none():
    healthy = [R.ref_check_append(seeded(s), A.CY_APPEND)["valid"] for s in range(0, 60, 3)]
    stale = [R.ref_check_append(seeded(s), A.CY_APPEND) for s in range(1, 60, 3)]
    assert set(healthy) == {A.VALID}
    assert sum(w["valid"] == A.INVALID and w["cause"] == 0 for w in stale) >= 5


def test_priority_of_the_causes():
    parts = all_causes()
    for gone, cause in ((), 13), ((13,), 14), ((13, 14), 15), ((13, 14, 15), 16), ((14,), 13), ((15,), 13), ((16,), 13), ((13, 15), 14):
        h = [op for c, ops in parts.items() if c not in gone for op in ops]
        assert R.ref_check_append(h, A.CY_APPEND)["cause"] == cause
        got = host_answer(h)
        names = {v: k for k, v in A.CAUSES.items()}
        assert (got["cause"] if "cause" in got else names[got["map"]["type"]]) == cause


def test_checker_returns_maps_and_raises_for_a_missing_writer():
    chk = CY.checker(CY.appends_and_reads_graph, device=False)
    out = chk.check({}, [dict(NEM), ok(r("x", [1, 2, 1]))], {})
    assert out["type"] == "duplicate-elements" and out["duplicates"] == {1: 2} and out["op"]["index"] == 1
    out = chk.check({}, [ok(["w", "x", 1])], {})
    assert out["valid?"] == "unknown" and out["type"] == "unexpected-txn-micro-op-types" and len(out["examples"]) == 1
    with pytest.raises(CY.IllegalHistory) as e:
        chk.check({}, [dict(NEM), row("fail", ap("x", 1)), ok(r("x", [1]))], {})
    assert (e.value.cause, e.value.row) == ("no-writer", 2)
    # elements that are no longs stay on the host and compare by equality
    out = chk.check({}, [ok(ap("x", "a")), ok(r("x", ["a"]))], {})
    assert out == {"valid?": True, "scc-count": 0, "cycles": []}
    # G2 with its explanation
    h = [dict(G["ops"][n]) for n in ("rxay1", "ryax1", "rx1ry1")]
    out = chk.check({}, h, {})
    assert out["valid?"] is False and out["cycles"][0][1::2] == ["something something"] * 2
    # combined with wr-graph: on the host
    both = CY.checker(CY.combine(CY.appends_and_reads_graph, CY.wr_graph)).check({}, h[:2], {})
    assert both == {"valid?": True, "scc-count": 0, "cycles": []}


def test_encode_append_round_trip_and_refusals():
    h = [dict(NEM), row("invoke", ap("x", 1), r("y", None)), ok(ap("x", 1), r("y", [])), row("fail", r("x", [1, 2, 3]), ap("y", 7)),
         {"process": 1, "type": "info", "f": "txn", "value": None}]
    c = CY.encode_append(h)
    assert c.n == 5 and c.n_keys == 2 and c.keys == ["x", "y"]
    assert c.value.tolist() == [A.NIL, 0, 8, 16, A.NIL] and c.value2.tolist() == [0, 2, 2, 2, 0]
    w = c.aux[:24].reshape(-1, 4).tolist()
    assert w == [[A.F_APPEND, 0, 1, 0], [A.F_READ, 1, 24, 0], [A.F_APPEND, 0, 1, 0], [A.F_READ, 1, 24, 0],
                 [A.F_READ, 0, 24, 3], [A.F_APPEND, 1, 7, 0]]
    assert c.aux[24:].tolist() == [1, 2, 3]
    # back to op maps
    back = []
    for i in range(c.n):
        if c.value2[i] == 0:
            continue
        txn = []
        for f, k, a, b in c.aux[c.value[i]:c.value[i] + 4 * c.value2[i]].reshape(-1, 4).tolist():
            txn.append(["r", c.keys[k], c.aux[a:a + b].tolist()] if f == A.F_READ else ["append", c.keys[k], a])
        back.append(txn)
    assert back == [[m[:2] + [m[2] or []] if m[0] == "r" else m for m in op["value"]] for op in h[1:4]]
    assert CY.encode_append([]).n == 0
    for bad in (ap("x", None), ap("x", "s"), ap("x", 1.5), ap("x", A.NIL), r("x", [1, None]), r("x", ["s"]), r("x", 5), ["w", "x", 1],
                ["cas", "x", [1, 2]]):
        with pytest.raises(TypeError):
            CY.encode_append([ok(bad)])
    with pytest.raises(TypeError):
        CY.encode([ok(ap("x", 1))])
    assert CY.appends_and_reads_graph.analyzers == A.CY_APPEND == 16
    assert CY.combine(CY.appends_and_reads_graph, CY.realtime_graph).analyzers == A.CY_APPEND | A.CY_REALTIME


def test_long_reads_on_the_host():
    h = long_read_history(257, [0, 1, 63, 64, 65, 255, 256, 257])
    want = R.ref_check_append(h, A.CY_APPEND)
    assert want["valid"] == A.VALID and set(host_answer(h)["edges"]) == want["edges"]


def test_abi_constants_and_struct_sizes(tmp_path):
    """The header's new constants equal _abi's; the structs keep their sizes and offsets."""
    from conftest import ROOT
    prog = tmp_path / "sz.c"
    prog.write_text(f'''#include <stdio.h>
#include <stddef.h>
#include "{os.path.join(ROOT, "include", "jh.h")}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d\\n", sizeof(jh_cycle_opts), sizeof(jh_cycle_result),
         offsetof(jh_cycle_opts, n_extra), offsetof(jh_cycle_result, unknown_rows), offsetof(jh_cycle_result, device_ms),
         JH_CY_APPEND, JH_F_APPEND, JH_CY_AP_DIRECT_READ, JH_CAUSE_DUPLICATE_APPENDS, JH_CAUSE_DUPLICATE_ELEMENTS,
         JH_CAUSE_NO_TOTAL_ORDER, JH_CAUSE_NO_WRITER, JH_CY_MAX_MOPS);
  return 0; }}''')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(A.JhCycleOpts), C.sizeof(A.JhCycleResult), A.JhCycleOpts.n_extra.offset,
                   A.JhCycleResult.unknown_rows.offset, A.JhCycleResult.device_ms.offset, A.CY_APPEND, A.F_APPEND,
                   A.CY_AP_DIRECT_READ, A.CAUSE_DUPLICATE_APPENDS, A.CAUSE_DUPLICATE_ELEMENTS, A.CAUSE_NO_TOTAL_ORDER,
                   A.CAUSE_NO_WRITER, A.CY_MAX_MOPS]
    assert got[:2] == [64, 152] and (A.CY_PROCESS, A.CY_REALTIME, A.CY_WR, A.CY_APPEND) == (1, 2, 4, 16)
    assert [A.CAUSES[c] for c in (13, 14, 15, 16)] == ["duplicate-appends", "duplicate-elements", "no-total-state-order", "no-writer"]


def test_synth_append_history():
    """synth.append_history: the serial schedule is valid with and without the
    realtime edges, stale reads give SCCs, reads stay below max_len, and the
    columns are what encode_append makes of their op maps."""
    from jepsen_amd import synth
    for anomalies in (0, 6):
        cols = synth.append_history(300, 5, 4, anomalies, 0.05, seed=1, max_len=8)
        ops = synth.append_columns_to_ops(cols)
        assert cols.n == len(ops) == 600 and cols.n_keys > 4 and (np.asarray(cols.type) == A.TYPE_INFO).any()
        assert max(len(m[2] or ()) for op in ops for m in op["value"] if m[0] == "r") < 8
        for mask in (A.CY_APPEND, A.CY_APPEND | A.CY_REALTIME | A.CY_PROCESS):
            want = R.ref_check_append(ops, mask)
            assert want["cause"] == 0 and (want["scc_count"] > 0) is bool(anomalies), (anomalies, mask)
        m, m2 = CY._Mops(cols), CY._Mops(CY.encode_append(ops))
        assert m.entries == m2.entries == want["entries"]
        edges = CY.append_edges(m)
        assert sorted(map(tuple, edges.tolist())) == sorted(map(tuple, CY.append_edges(m2).tolist()))
        assert len(edges) == want["edge_count"][2]
