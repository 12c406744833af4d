"""monotonic-key-graph on the device (jh_check_cycle with JH_CY_MONOTONIC,
jh_cycle_mono.hip) against the naive restatement of tests/cycle_mono_ref.py:
valid, cause, edge_count, entries, set(edges_out) with len(edges_out) ==
sum(edge_count), back_edges, labels_out, the SCC lists and scc_count, exactly, on
auto and on both forced tiers where the largest region fits the on-chip tier.
Everything is integer, so every comparison is exact."""
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLD
from jepsen_amd import _abi as A
from jepsen_amd import _native
from jepsen_amd import cycle as CY
from jepsen_amd import history as H
import cycle_mono_ref as R
from cycle_mono_cases import NEM, chain, groups, interleaved_chains, ok, random_mono_history, row

pytestmark = pytest.mark.gpu

G = json.load(open(os.path.join(GOLD, "cycle_mono.json")))
MO, RT, PR = 32, A.CY_REALTIME, A.CY_PROCESS
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)


def paths_for(n, edges):
    reg = CY.regions(n, edges)
    big = len(reg) and int((reg[:, 1] - reg[:, 0] + 1).max()) > A.CY_LDS_VERTICES
    return (A.CY_PATH_AUTO, A.CY_PATH_GLOBAL) if big else (A.CY_PATH_AUTO, A.CY_PATH_LDS, A.CY_PATH_GLOBAL)


def code_of(fn):
    with pytest.raises(_native.JhError) as e:
        fn()
    return e.value.code


def raw_cols(h, order=None, gap=0):
    """Columns of op maps whose keys are int64 themselves (nothing is interned)
    and whose rows of every type carry their map. order: the rows whose pair
    ranges are laid out first, in that order; gap: garbage pairs between ranges."""
    proc, typ = CY._encode_rows(h)
    n = len(h)
    val, val2, aux = np.full(n, A.NIL, np.int64), np.zeros(n, np.int64), []
    rows = list(order or ()) + [i for i in range(n) if i not in (order or ())]
    for i in rows:
        v = h[i].get("value")
        if isinstance(v, dict) and v:
            aux += [77, 77] * gap
            val[i], val2[i] = len(aux) // 2, len(v)
            for k, x in v.items():
                aux += [k, A.NIL if x is None else x]
    return H.Columns(n=n, process=proc, type=typ, f=np.full(n, A.F_FIRST_INTERNED, np.int64), key=None, value=val, value2=val2,
                     n_keys=0, aux=np.asarray(aux + [0, 0], np.int64)[:len(aux)], keys=[])


def agree(ctx, history, analyzers=MO, extra=None, cols=None):
    want = R.ref_check_mono(history, analyzers, list(zip(*extra)) if extra else ())
    cols = CY.encode_map(history) if cols is None else cols
    paths = (0, 1, 2) if want["cause"] else paths_for(len(history), sorted(want["edges"]))
    for path in paths:
        got = ctx.check_cycle(cols, analyzers, path, extra, scc_cap=max(want.get("scc_count", 0), 1), edge_cap=1 << 21)
        assert (got["valid"], got["cause"], got["unknown_row"]) == (want["valid"], want["cause"], want["unknown_row"]), path
        if want["cause"]:
            continue
        assert got["entries"] == want["entries"], path
        assert got["labels"].tolist() == want["labels"], path
        assert (got["scc_count"], got["scc_vertices"]) == (want["scc_count"], want["scc_vertices"]) and got["sccs"] == want["sccs"], path
        edges = list(map(tuple, got["edges"].tolist()))
        assert got["edge_count"] == want["edge_count"] and len(edges) == sum(got["edge_count"]) and set(edges) == want["edges"], path
        assert got["back_edges"] == want["back_edges"] == sum(1 for a, b in edges if b < a), path
    return want


# -- goldens -------------------------------------------------------------------------
def test_golden_graphs(ctx):
    for case in G["graphs"]:
        want = agree(ctx, [dict(op) for op in case["history"]])
        assert want["edges"] == {(int(a), b) for a, succ in case["graph"].items() for b in succ}


def test_checker_module_on_device(ctx):
    fn = CY.monotonic_key_graph
    both = CY.combine(fn, CY.process_graph)
    cases = [(fn, [dict(op) for op in c["history"]], c["result"]) for c in G["checker"]]
    mp = G["monotonic_process"][0]
    h = [dict(op) for op in mp["history"]]
    cases += [(fn, h, mp["monotonic_result"]), (both, h, mp["combined_result"]), (both, [dict(NEM)] + h, None)]
    stale = random_mono_history(3, 120, stale=0.3)
    cases += [(CY.combine(fn, CY.realtime_graph), stale, None), (CY.combine(fn, CY.realtime_graph, CY.process_graph), stale, None)]
    for an, h, result in cases:
        want = CY.checker(an, device=False).check({}, h, {})
        assert result is None or want == result
        for path in (0, 1, 2):
            assert CY.checker(an, path=path).check({}, h, {}) == want
    assert CY.checker(CY.combine(fn, CY.realtime_graph), device=False).check({}, stale, {})["valid?"] is False
    # values that do not encode: the host answers
    assert CY.checker(fn).check({}, [ok({"x": "a"}), ok({"x": "b"})], {}) == {"valid?": True, "scc-count": 0, "cycles": []}


# -- group shapes, one key -----------------------------------------------------------
SHAPES = {"no group": (), "one group": (5,), "1x1": (1, 1), "1x65": (1, 65), "65x1": (65, 1), "63x64": (63, 64), "257x3": (257, 3),
          "3x257": (3, 257), "257x3x130": (257, 3, 130)}


@pytest.mark.parametrize("name", SHAPES)
def test_group_shapes(ctx, name):
    sizes = SHAPES[name]
    want = agree(ctx, groups(*sizes))
    assert want["valid"] == A.VALID
    assert want["edge_count"][2] == sum(a * b for a, b in zip(sizes, sizes[1:])) and want["entries"] == sum(sizes)


def test_a_chain_of_1000_unique_values(ctx):
    want = agree(ctx, chain(1000))
    assert want["valid"] == A.VALID and want["edge_count"] == [0, 0, 999, 0]


def test_a_chain_and_wide_groups_in_one_tile(ctx):
    """A chain of single rows that runs into groups of hundreds: tiles of the fill
    that hold many sources and tiles that hold a few."""
    h = chain(3000) + [ok({"x": 3000 + j // 300}) for j in range(1500)]
    want = agree(ctx, h)
    assert want["valid"] == A.VALID and want["edge_count"][2] == 2999 + 300 + 4 * 300 * 300


def test_three_interleaved_chains_of_10000_rows(ctx):
    h = interleaved_chains(10000)
    want = agree(ctx, h)
    assert want["valid"] == A.VALID and want["edge_count"][2] > 2000
    assert agree(ctx, h, MO | RT)["valid"] == A.VALID


# -- values --------------------------------------------------------------------------
def test_values(ctx):
    # negative, 0, the extremes; nil sorts first and links to the next group
    h = [ok({"x": 0}), ok({"x": I64_MAX}), ok({"x": -5}), ok({"x": I64_MIN + 1}), ok({"x": None}), ok({"x": None})]
    assert agree(ctx, h)["edges"] == {(4, 3), (5, 3), (3, 2), (2, 0), (0, 1)}
    # equal low words, equal high words
    h = [ok({"x": (7 << 32) + 3}), ok({"x": (2 << 32) + 3}), ok({"x": (2 << 32) + 9}), ok({"x": (2 << 32) + 1})]
    assert agree(ctx, h)["edges"] == {(3, 1), (1, 2), (2, 0)}
    # values need not be adjacent
    assert agree(ctx, [ok({"x": 4}), ok({"x": 0}), ok({"x": 1})])["edges"] == {(1, 2), (2, 0)}
    # keys 0 and 2^40, not interned
    h = [ok({0: 1, 1 << 40: 2}), ok({1 << 40: 1}), ok({0: 0}), ok({(1 << 40) + 1: 0, -3: 0})]
    assert agree(ctx, h, cols=raw_cols(h))["edges"] == {(2, 0), (1, 0)}


# -- rows ----------------------------------------------------------------------------
def test_two_rows_linked_by_two_keys_count_twice(ctx):
    want = agree(ctx, [ok({"x": 0, "y": 0}), ok({"x": 1, "y": 1})])
    assert want["edges"] == {(0, 1)} and want["edge_count"][2] == 2 and want["entries"] == 4


def test_pairs_out_of_order_and_apart_in_aux(ctx):
    h = groups(3, 4, 2) + [ok({"x": 1, "y": 0}), ok({"y": 1, "x": 0})]
    want = agree(ctx, h, cols=raw_cols([dict(op, value={{"x": 0, "y": 1}[k]: v for k, v in op["value"].items()}) for op in h],
                                       order=[10, 3, 0, 7], gap=3))
    assert want["edge_count"][2] == 4 * 5 + 5 * 2 + 1


def test_rows_that_are_ignored(ctx):
    # rows of other types carrying maps; an :ok row of process -1; nemesis rows in between
    h = [dict(NEM), ok({0: 0}), row("invoke", {0: 5}), row("fail", {0: 1}), dict(NEM), row("info", {0: 1}),
         dict(NEM, type="ok", value={0: 1}), ok({0: 2}), dict(NEM)]
    want = agree(ctx, h, cols=raw_cols(h))
    assert want["edges"] == {(1, 7)} and want["entries"] == 2
    for an in (MO, MO | RT, MO | PR):
        # an empty history; a history with no :ok row
        got = ctx.check_cycle(CY.encode_map([]), an, edge_cap=4)
        assert (got["valid"], got["cause"], got["entries"], got["edge_count"]) == (A.VALID, 0, 0, [0, 0, 0, 0])
        assert got["labels"].tolist() == [] and got["sccs"] == []
    assert agree(ctx, [row("invoke", None), row("info", {"x": 1})])["edge_count"] == [0, 0, 0, 0]
    assert agree(ctx, [dict(NEM)])["valid"] == A.VALID
    # value2 = 0 with a garbage value
    cols = CY.encode_map([ok(None), ok({"x": 1}), ok({}), ok({"x": 2})])
    cols.value = np.array([1 << 50, 0, -7, 1], np.int64)
    assert agree(ctx, [ok(None), ok({"x": 1}), ok({}), ok({"x": 2})], cols=cols)["edges"] == {(1, 3)}


# -- combinations --------------------------------------------------------------------
def test_monotonic_and_process_on_the_reference_case(ctx):
    h = [dict(op) for op in G["monotonic_process"][0]["history"]]
    assert agree(ctx, h)["valid"] == A.VALID and agree(ctx, h, PR)["valid"] == A.VALID
    want = agree(ctx, h, MO | PR)
    assert want["sccs"] == [[0, 1]] and want["edge_count"] == [1, 0, 1, 0]


SEEDS = [(seed, 40 + 9 * seed, 0.3 * (seed % 2)) for seed in range(40)]


@functools.lru_cache(maxsize=None)
def seeded_reference(seed, n_ops, stale, mask):
    return R.ref_check_mono(random_mono_history(seed, n_ops, n_procs=5, stale=stale), mask)


@pytest.mark.parametrize("seed,n_ops,stale", SEEDS)
def test_seeded_histories_with_realtime_and_process(ctx, seed, n_ops, stale):
    h = random_mono_history(seed, n_ops, n_procs=5, stale=stale)
    for mask in (MO | RT, MO | RT | PR):
        want = agree(ctx, h, mask)
        assert want == seeded_reference(seed, n_ops, stale, mask) and want["cause"] == 0
        assert stale or want["valid"] == A.VALID


def test_seeded_histories_reach_both_verdicts():
    for mask in (MO | RT, MO | RT | PR):
        verdicts = [seeded_reference(*s, mask)["valid"] for s in SEEDS]
        assert verdicts.count(A.VALID) >= 5 and verdicts.count(A.INVALID) >= 5


def test_extra_edges_with_the_builder(ctx):
    h = [ok({"x": 0}), ok({"x": 1}), ok({"x": 2})]
    want = agree(ctx, h, MO, ([2, 0], [0, 0]))
    assert want["sccs"] == [[0, 1, 2]] and want["edge_count"] == [0, 0, 2, 2]
    assert agree(ctx, h, MO | PR, ([1], [2]))["valid"] == A.VALID


def test_a_region_of_more_than_2048_rows(ctx):
    """One stale row at the end observes a value between the first two of a chain
    of 3 000 and a y above the chain's last row's: an SCC of all but row 0."""
    h = [ok({"x": 2 * v}) for v in range(2999)] + [ok({"x": 2 * 2999, "y": 5}), ok({"x": 1, "y": 10})]
    want = agree(ctx, h)
    assert want["scc_count"] == 1 and len(want["sccs"][0]) == 3000
    got = ctx.check_cycle(CY.encode_map(h), MO)
    assert got["path"] == 2 and got["global_regions"] == 1 and got["max_region"] == 3000
    assert code_of(lambda: ctx.check_cycle(CY.encode_map(h), MO, A.CY_PATH_LDS)) == A.JH_EINVAL


# -- return codes --------------------------------------------------------------------
def test_return_codes(ctx):
    good = [ok({"x": 1, "y": 2}), ok({"x": 2})]

    def with_(**kw):
        c = CY.encode_map(good)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    assert ctx.check_cycle(with_(), MO)["edge_count"] == [0, 0, 1, 0]
    assert code_of(lambda: ctx.check_cycle(with_(), MO | A.CY_WR)) == A.JH_EINVAL
    assert code_of(lambda: ctx.check_cycle(with_(), MO | A.CY_APPEND)) == A.JH_EINVAL
    assert code_of(lambda: ctx.check_cycle(with_(), MO | 8)) == A.JH_EINVAL
    assert code_of(lambda: ctx.check_cycle(with_(aux=np.arange(7, dtype=np.int64)), MO)) == A.JH_EINVAL             # an odd n_aux
    for value, value2 in (([0, 2], [2, 2]), ([3, 0], [1, 1]), ([-1, 2], [2, 1]), ([0, 1 << 62], [2, 1]), ([0, 2], [2, 1 << 62])):   # a range past aux
        c = with_(value=np.array(value, np.int64), value2=np.array(value2, np.int64))
        assert code_of(lambda: ctx.check_cycle(c, MO)) == A.JH_EINVAL, (value, value2)
    c = with_(value2=np.array([2, -1], np.int64))                                                                 # a negative count
    assert code_of(lambda: ctx.check_cycle(c, MO)) == A.JH_EINVAL
    c = with_(aux=np.array([0, 1, 0, 2, 0, 2], np.int64))                                                          # a key twice in a row
    assert code_of(lambda: ctx.check_cycle(c, MO)) == A.JH_EINVAL
    # the same ranges on rows that are not read are fine
    c = with_(type=np.array([A.TYPE_OK, A.TYPE_FAIL], np.int64), value=np.array([0, 99], np.int64), value2=np.array([2, -4], np.int64))
    assert ctx.check_cycle(c, MO)["entries"] == 2


def test_pairs_per_row(ctx):
    many = {k: k for k in range(A.CY_MAX_MOPS + 1)}
    full = dict(list(many.items())[:-1])
    want = agree(ctx, [ok(full), ok({k: v + 1 for k, v in full.items()})])
    assert want["edge_count"][2] == 64 and want["edges"] == {(0, 1)}
    assert code_of(lambda: ctx.check_cycle(CY.encode_map([ok(many)]), MO)) == A.JH_EUNSUPPORTED
    # through the checker: the host answers
    assert CY.checker(CY.monotonic_key_graph).check({}, [ok(many)], {})["valid?"] is True


def test_an_edge_count_past_the_cap_is_refused_from_the_64_bit_count(ctx):
    """Two groups of 46 341 rows: 46 341^2 = 2 147 488 281 link calls, which a 32-bit count would wrap."""
    typ = np.full(2 * 46341, A.TYPE_OK, np.int64)
    n = len(typ)
    aux = np.zeros(2 * n, np.int64)
    aux[1::2] = np.arange(n) >= 46341
    cols = H.Columns(n=n, process=np.arange(n, dtype=np.int64) % 5, type=typ, f=np.full(n, A.F_FIRST_INTERNED, np.int64), key=None,
                     value=np.arange(n, dtype=np.int64), value2=np.ones(n, np.int64), n_keys=0, aux=aux, keys=["x"])
    with pytest.raises(_native.JhError) as e:
        ctx.check_cycle(cols, MO, edge_cap=16)
    assert e.value.code == A.JH_EUNSUPPORTED and "2^31 - 2" in str(e.value)


def test_edge_cap(ctx):
    h = groups(4, 5, 3)
    want = R.ref_check_mono(h, MO | PR)
    for cap in (0, 7):
        got = ctx.check_cycle(CY.encode_map(h), MO | PR, edge_cap=cap)
        assert got["edge_count"] == want["edge_count"] and sum(got["edge_count"]) > 7
        edges = list(map(tuple, got["edges"].tolist()))
        assert len(edges) == cap and set(edges) <= want["edges"]
        assert (got["valid"], got["scc_count"], got["back_edges"]) == (want["valid"], want["scc_count"], want["back_edges"])
