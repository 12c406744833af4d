"""appends-and-reads-graph on the device (jh_check_cycle with JH_CY_APPEND,
jh_cycle_append.hip) against the literal transcription of
tests/cycle_append_ref.py: the cause and every unknown_* field, or labels_out,
the counts, the SCC lists, set(edges_out) and edge_count, exactly, on auto and on
both forced tiers where the largest region fits the on-chip tier. Everything is
integer, so every comparison is exact."""
import json
import os

import numpy as np
import pytest

from conftest import GOLD
from jepsen_amd import _abi as A
from jepsen_amd import _native
from jepsen_amd import cycle as CY
import cycle_append_ref as R
from cycle_append_cases import NEM, all_causes, ap, appends_of, long_read_history, ok, r, random_append_history, row

pytestmark = pytest.mark.gpu

G = json.load(open(os.path.join(GOLD, "cycle_append.json")))
AP, RT, PR = A.CY_APPEND, A.CY_REALTIME, A.CY_PROCESS
D = A.CY_AP_DIRECT_READ


def paths_for(n, edges):
    reg = CY.regions(n, edges)
    big = len(reg) and int((reg[:, 1] - reg[:, 0] + 1).max()) > A.CY_LDS_VERTICES
    return (A.CY_PATH_AUTO, A.CY_PATH_GLOBAL) if big else (A.CY_PATH_AUTO, A.CY_PATH_LDS, A.CY_PATH_GLOBAL)


def same_partition(got, want, path):
    assert got["labels"].tolist() == want["labels"], path
    assert (got["valid"], got["scc_count"], got["scc_vertices"]) == (want["valid"], want["scc_count"], want["scc_vertices"]), path
    assert got["sccs"] == want["sccs"], path


def code_of(fn):
    with pytest.raises(_native.JhError) as e:
        fn()
    return e.value.code


def agree(ctx, history, analyzers=AP, extra=None):
    want = R.ref_check_append(history, analyzers, list(zip(*extra)) if extra else ())
    cols = CY.encode_append(history)
    paths = (0, 1, 2) if want["cause"] else paths_for(len(history), sorted(want["edges"]))
    for path in paths:
        got = ctx.check_cycle(cols, analyzers, path, extra, scc_cap=max(want.get("scc_count", 0), 1), edge_cap=1 << 17)
        assert (got["valid"], got["cause"], got["unknown_row"], got["unknown_rows"]) == \
            (want["valid"], want["cause"], want["unknown_row"], want["unknown_rows"]), path
        if want["cause"] not in (A.CAUSE_DOUBLE_INVOKE, A.CAUSE_ORPHAN, A.CAUSE_UNMATCHED_INVOKE):    # (those return before the txns are read)
            assert got["entries"] == want["entries"], path
        if want["cause"]:
            key = cols.keys[got["unknown_key"]] if got["unknown_key"] != A.NIL else None
            value = None if got["unknown_value"] == A.NIL else got["unknown_value"]
            assert (key, value) == (want["unknown_key"], want["unknown_value"]), path
            assert got["scc_count"] == 0 and got["labels"].tolist() == [-1] * len(history) and got["sccs"] == [], path
            continue
        same_partition(got, want, path)
        edges = list(map(tuple, got["edges"].tolist()))
        assert set(edges) == want["edges"] and got["edge_count"] == want["edge_count"] and len(edges) == sum(got["edge_count"]), path
        assert got["back_edges"] == sum(1 for a, b in edges if b < a), path
    return want


def caused(want):
    return want["cause"], want["unknown_row"], want["unknown_rows"][0], want["unknown_key"], want["unknown_value"]


# -- goldens -------------------------------------------------------------------------
@pytest.mark.parametrize("case", G["cases"], ids=lambda c: c["name"])
def test_golden_graphs(ctx, case):
    h = [dict(G["ops"][name]) for name in case["history"]]
    pos = {name: i for i, name in enumerate(case["history"])}
    want = agree(ctx, h)
    assert want["edges"] == {(pos[a], pos[b]) for a, succ in case["graph"].items() for b in succ}


def test_golden_errors(ctx):
    dup_read, dup_append, order = [[dict(op) for op in c["history"]] for c in G["errors"]]
    assert caused(agree(ctx, dup_read)) == (A.CAUSE_DUPLICATE_ELEMENTS, 0, 0, "x", 1)
    assert caused(agree(ctx, dup_append)) == (A.CAUSE_DUPLICATE_APPENDS, 1, 1, "x", 1)
    assert caused(agree(ctx, order)) == (A.CAUSE_NO_TOTAL_ORDER, 0, 1, "x", None)


# -- the prefix compare ------------------------------------------------------------
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257]


@pytest.mark.parametrize("longest", [257, 4097])
def test_read_lengths_against_a_long_read(ctx, longest):
    want = agree(ctx, long_read_history(longest, LENGTHS))
    assert want["valid"] == A.VALID
    # the read of length c hangs between the appenders of c and of c + 1 (rows c - 1 and c)
    reader = {c: longest + 1 + i for i, c in enumerate(LENGTHS)}
    assert {(62, reader[63]), (reader[63], 63), (reader[0], 0), (255, reader[256]), (reader[256], 256)} <= want["edges"]


@pytest.mark.parametrize("longest", [257, 4097])
@pytest.mark.parametrize("at", [0, 63, 64, 256])
def test_a_mismatch_at(ctx, longest, at):
    """In the first element, at a tile boundary and in the last one of a read of 257."""
    h = long_read_history(longest, [1, 64])
    bad = list(range(1, 258))
    bad[at] = 9999
    h.append(ok(r("x", bad)))
    assert caused(agree(ctx, h)) == (A.CAUSE_NO_TOTAL_ORDER, len(h) - 1, 1, "x", None)


def test_two_different_reads_of_maximal_length(ctx):
    h = [ok(r("x", [1, 2, 3])), ok(r("y", [1])), ok(r("x", [1, 2, 4])), ok(r("x", [1, 2]))]
    assert caused(agree(ctx, h)) == (A.CAUSE_NO_TOTAL_ORDER, 2, 1, "x", None)
    # the first of them is L_k: a later shorter read that fits only the second is bad as well
    h = appends_of("x", [1, 2, 3, 4]) + [ok(r("x", [1, 2, 3])), ok(r("x", [1, 2, 4])), ok(r("y", [7, 8])), ok(r("y", [8]))]
    assert caused(agree(ctx, h)) == (A.CAUSE_NO_TOTAL_ORDER, 5, 2, "x", None)


def test_nil_and_empty_reads(ctx):
    h = [ok(r("x", None)), ok(r("x", [])), ok(ap("x", 1)), ok(r("x", [1]))]
    assert agree(ctx, h)["edges"] == {(0, 2), (1, 2), (2, 3)}
    assert agree(ctx, [ok(r("x", None)), ok(r("x", []))])["edges"] == set()
    assert agree(ctx, [{"process": 0, "type": "ok", "f": "txn", "value": None}, ok()])["entries"] == 0


# -- edges -----------------------------------------------------------------------------
def test_appends_that_nobody_reads(ctx):
    # a key appended but never read; an append never read (its key is)
    want = agree(ctx, [ok(ap("y", 1)), ok(ap("x", 1)), ok(ap("x", 2)), ok(r("x", [1]))])
    assert want["edges"] == {(1, 3)}


def test_self_pairs_are_excluded(ctx):
    # a txn that reads its own append; one that reads the previous state and appends
    want = agree(ctx, [ok(ap("x", 1), r("x", [1])), ok(r("x", [1]), ap("x", 2)), ok(r("x", [1, 2]))])
    assert want["edges"] == {(0, 1), (1, 2)} and want["edge_count"][2] == 4      # wr, ww and rw 0->1, wr 1->2


def test_two_readers_of_one_length(ctx):
    want = agree(ctx, [ok(r("x", None)), ok(r("x", [])), ok(ap("x", 1)), ok(r("x", [1])), ok(r("x", [1]))])
    assert want["edges"] == {(0, 2), (1, 2), (2, 3), (2, 4)}


def test_the_same_read_twice_in_one_txn(ctx):
    want = agree(ctx, [ok(r("x", None), r("x", None)), ok(ap("x", 1)), ok(r("x", [1]), r("x", [1]))])
    assert want["edges"] == {(0, 1), (1, 2)} and want["edge_count"][2] == 4


def test_writers(ctx):
    # an :info writer
    assert agree(ctx, [row("info", ap("x", 1)), ok(r("x", [1]))])["edges"] == {(0, 1)}
    # a :fail writer that is read: on a wr slot, and on a ww slot
    assert caused(agree(ctx, [row("fail", ap("x", 1)), ok(ap("y", 3)), ok(r("y", [3]), r("x", [1]))])) == \
        (A.CAUSE_NO_WRITER, 2, 1, "x", 1)
    h = [row("fail", ap("x", 1)), ok(ap("x", 2)), ok(r("z", None), ap("x", 3)), ok(ap("x", 4))]
    assert caused(agree(ctx, h + [row("fail", r("x", [1, 2, 3, 4])), row("info", r("x", [1, 2, 3]))])) == \
        (A.CAUSE_NO_WRITER, 1, 0, "x", 1)                                      # only the :info read counts; the ww slot of 2
    assert caused(agree(ctx, [row("fail", ap("x", 1)), ok(r("z", None), ap("x", 2)), ok(r("q", [])), ok(r("x", [1, 2]))])) == \
        (A.CAUSE_NO_WRITER, 1, 1, "x", 1)                                      # the ww slot of the append of 2
    # two :ok appends of one (k, v) and no invoke rows: the later one is the writer
    assert agree(ctx, [ok(ap("x", 1)), ok(ap("x", 1)), ok(r("x", [1]))])["edges"] == {(1, 2)}


def test_duplicate_appends(ctx):
    i1, i2 = row("invoke", ap("x", 1), r("y", None)), row("invoke", ap("y", 2), ap("x", 1))
    # inside one txn and across txns: the earliest is named
    assert caused(agree(ctx, [i1, row("invoke", r("y", None), ap("z", 5), ap("z", 5)), i2])) == (A.CAUSE_DUPLICATE_APPENDS, 1, 2, "z", 5)
    assert caused(agree(ctx, [i1, i2, row("invoke", ap("z", 5), ap("z", 5))])) == (A.CAUSE_DUPLICATE_APPENDS, 1, 1, "x", 1)
    # an invoke-only duplicate whose completion failed
    assert caused(agree(ctx, [i1, ok(ap("x", 1), r("y", [])), i2, row("fail", ap("y", 2), ap("x", 1))])) == \
        (A.CAUSE_DUPLICATE_APPENDS, 2, 1, "x", 1)
    # completions alone are no duplicates
    assert agree(ctx, [i1, ok(ap("x", 1), r("y", [])), row("info", ap("x", 1))])["cause"] == 0


def test_duplicate_elements(ctx):
    # in L_k at the last position: the shorter prefix reads hold none, L_k itself does
    h = appends_of("x", range(1, 70)) + [ok(r("x", list(range(1, 70)))), ok(r("x", list(range(1, 70)) + [5]))]
    assert caused(agree(ctx, h)) == (A.CAUSE_DUPLICATE_ELEMENTS, len(h) - 1, 0, "x", 5)
    # a later prefix read past the duplicate's place is named when it stands first
    h = [ok(r("x", [1, 2])), ok(r("y", None), r("x", [1, 2, 1])), ok(r("x", [1, 2, 1, 3]))]
    assert caused(agree(ctx, h)) == (A.CAUSE_DUPLICATE_ELEMENTS, 1, 1, "x", 1)
    # in a non-prefix read (cause 14 goes before cause 15)
    h = [ok(r("x", [1, 2, 3, 4])), ok(r("x", [2, 7, 7, 2]))]
    assert caused(agree(ctx, h)) == (A.CAUSE_DUPLICATE_ELEMENTS, 1, 0, "x", 7)
    # in an :invoke row's and in a :fail row's read
    assert caused(agree(ctx, [row("invoke", r("x", [4, 4])), ok(r("x", None))])) == (A.CAUSE_DUPLICATE_ELEMENTS, 0, 0, "x", 4)
    assert caused(agree(ctx, [ok(r("x", None)), row("fail", ap("x", 1), r("x", [3, 4, 3]))])) == (A.CAUSE_DUPLICATE_ELEMENTS, 1, 1, "x", 3)


def test_the_direct_check_at_its_cap(ctx):
    full = list(range(1, D + 1))
    h = [row("fail", r("x", full[:-1] + [1]))]
    assert caused(agree(ctx, h)) == (A.CAUSE_DUPLICATE_ELEMENTS, 0, 0, "x", 1)
    assert agree(ctx, [row("fail", r("x", full))])["valid"] == A.VALID
    cols = CY.encode_append([row("fail", r("x", full + [D + 1]))])
    assert code_of(lambda: ctx.check_cycle(cols, AP)) == A.JH_EUNSUPPORTED
    # through the checker: the host answers
    chk = CY.checker(CY.appends_and_reads_graph)
    assert chk.check({}, [row("fail", r("x", full + [1]))], {})["type"] == "duplicate-elements"


def test_priority_of_the_causes(ctx):
    parts = all_causes()
    for gone, cause in ((), 13), ((13,), 14), ((13, 14), 15), ((13, 14, 15), 16), ((14,), 13), ((15,), 13), ((16,), 13), ((13, 15), 14):
        h = [op for c, ops in parts.items() if c not in gone for op in ops]
        assert agree(ctx, h)["cause"] == cause
    # the pairing causes go first
    h = [row("invoke", ap("x", 1)), row("invoke", ap("x", 1))]
    assert agree(ctx, h, AP | RT)["cause"] == A.CAUSE_DOUBLE_INVOKE and agree(ctx, h)["cause"] == A.CAUSE_DUPLICATE_APPENDS


# -- sizes ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [1, 300])
def test_keys(ctx, n_keys):
    h = [ok(*[ap(k, 1) for k in range(i, min(i + 50, n_keys))]) for i in range(0, n_keys, 50)]
    h += [ok(*[r(k, [1]) for k in range(i, min(i + 50, n_keys))]) for i in range(0, n_keys, 50)]
    h += [ok(ap(0, 2)), ok(r(0, [1, 2]))]
    want = agree(ctx, h)
    assert want["valid"] == A.VALID and want["edge_count"][2] >= n_keys


def test_micro_op_counts(ctx):
    many = [ap("x", i + 1) for i in range(A.CY_MAX_MOPS + 1)]
    h = [ok(*many[:-1]), ok(r("x", list(range(1, A.CY_MAX_MOPS + 1))))]
    assert agree(ctx, h)["edges"] == {(0, 1)}
    assert code_of(lambda: ctx.check_cycle(CY.encode_append([ok(*many)]), AP)) == A.JH_EUNSUPPORTED


def test_empty_history(ctx):
    cols = CY.encode_append([])
    for mask in (AP, AP | RT | PR):
        for path in (0, 1, 2):
            got = ctx.check_cycle(cols, mask, path, edge_cap=4)
            assert (got["valid"], got["cause"], got["path"], got["unknown_row"], got["entries"]) == (A.VALID, 0, 0, -1, 0)
            assert got["edge_count"] == [0, 0, 0, 0] and got["labels"].tolist() == [] and got["sccs"] == []
    assert CY.checker(CY.appends_and_reads_graph).check({}, [], {}) == {"valid?": True, "scc-count": 0, "cycles": []}
    assert agree(ctx, [dict(NEM)])["valid"] == A.VALID


def test_nemesis_rows_in_between(ctx):
    h = [dict(NEM), ok(r("x", None)), dict(NEM), dict(NEM), ok(ap("x", 1)), dict(NEM), ok(r("x", [1])), dict(NEM)]
    assert agree(ctx, h)["edges"] == {(1, 4), (4, 6)}


def test_g2_needs_the_other_analyzers_too(ctx):
    """Two txns that each read the empty state of the key the other appends to,
    one after the other in real time and on one process."""
    t1, t2 = [r("x", None), ap("y", 1)], [r("y", None), ap("x", 1)]
    h = [row("invoke", *t1), ok(*t1), row("invoke", *t2), ok(*t2), row("invoke", r("x", None), r("y", None)),
         ok(r("x", [1]), r("y", [1]))]
    want = agree(ctx, h, AP | RT | PR)
    assert want["sccs"] == [[1, 3]] and want["edge_count"][0] == 2 and want["edge_count"][1] == 2
    assert agree(ctx, h, AP)["sccs"] == [[1, 3]]
    # extra edges travel along
    assert agree(ctx, h[:2], AP, ([1], [0]))["valid"] == A.VALID


def test_return_codes(ctx):
    good = [ok(ap("x", 1), r("x", [1, 2]))]

    def with_(**kw):
        c = CY.encode_append(good)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def aux_with(at, v):
        a = CY.encode_append(good).aux.copy()
        a[at] = v
        return a
    assert ctx.check_cycle(with_(), AP)["cause"] == A.CAUSE_NO_WRITER
    assert code_of(lambda: ctx.check_cycle(with_(), AP | A.CY_WR)) == A.JH_EINVAL
    assert code_of(lambda: ctx.check_cycle(with_(), 8)) == A.JH_EINVAL
    assert code_of(lambda: ctx.check_cycle(with_(n_keys=0), AP)) == A.JH_EINVAL                  # a key outside [0, n_keys)
    assert code_of(lambda: ctx.check_cycle(with_(aux=aux_with(1, -1)), AP)) == A.JH_EINVAL
    assert code_of(lambda: ctx.check_cycle(with_(aux=aux_with(9, A.NIL)), AP)) == A.JH_EINVAL     # an element of the read
    assert code_of(lambda: ctx.check_cycle(with_(aux=aux_with(2, A.NIL)), AP)) == A.JH_EINVAL     # the appended element
    for at, v in ((6, 9), (6, -1), (7, 3), (7, -1), (6, 1 << 40)):                                # the read's range
        assert code_of(lambda: ctx.check_cycle(with_(aux=aux_with(at, v)), AP)) == A.JH_EINVAL, (at, v)
    for value, value2 in ((4, 2), (0, 3), (-1, 1), (0, -1)):                                     # the txn's range
        c = with_(value=np.array([value], np.int64), value2=np.array([value2], np.int64))
        assert code_of(lambda: ctx.check_cycle(c, AP)) == A.JH_EINVAL, (value, value2)
    assert code_of(lambda: ctx.check_cycle(with_(aux=aux_with(0, A.F_WRITE)), AP)) == A.JH_EUNSUPPORTED


# -- random histories ----------------------------------------------------------------
# (seed, txns, stale): chosen with the transcription alone, which finds the healthy ones valid and SCCs in the stale ones
SEEDS = [(1, 1025, 0.0), (2, 257, 0.0), (3, 600, 0.0), (4, 1000, 0.0), (11, 1025, 0.3), (12, 257, 0.3), (13, 600, 0.3), (14, 1000, 0.3)]


@pytest.mark.parametrize("seed,n_txns,stale", SEEDS)
def test_random_histories(ctx, seed, n_txns, stale):
    h = random_append_history(seed, n_txns, n_procs=7, n_keys=6, stale=stale, max_len=40)
    want = agree(ctx, h, AP | RT | PR)
    assert want["cause"] == 0 and ((want["valid"] == A.VALID) if not stale else want["scc_count"] > 0)


# -- the checker module ----------------------------------------------------------------
def test_checker_module_on_device(ctx):
    fn = CY.appends_and_reads_graph
    maps = [[dict(op) for op in c["history"]] for c in G["errors"]]
    stale = random_append_history(12, 120, n_procs=4, n_keys=3, stale=0.4)
    g2 = [dict(G["ops"][n]) for n in ("rxay1", "ryax1", "rx1ry1")]
    for h in maps + [stale, g2, [dict(NEM)] + g2]:
        want = CY.checker(fn, device=False).check({}, h, {})
        for path in (0, 1, 2):
            assert CY.checker(fn, path=path).check({}, h, {}) == want
    assert [m["type"] for m in (CY.checker(fn).check({}, h, {}) for h in maps)] == \
        ["duplicate-elements", "duplicate-appends", "no-total-state-order"]
    out = CY.checker(fn).check({}, g2, {})
    assert out["valid?"] is False and out["cycles"][0][1::2] == ["something something"] * 2
    assert CY.checker(fn, device=False).check({}, stale, {})["scc-count"] > 0
    both = CY.combine(fn, CY.realtime_graph)
    assert CY.checker(both).check({}, stale, {}) == CY.checker(both, device=False).check({}, stale, {})
    with pytest.raises(CY.IllegalHistory) as e:
        CY.checker(fn).check({}, [dict(NEM), row("fail", ap("x", 1)), ok(r("x", [1]))], {})
    assert (e.value.cause, e.value.row) == ("no-writer", 2)
