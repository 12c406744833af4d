"""checker/perf on the device (jh_perf, jh_perf.hip) against the numpy closed
form of tests/perf_ref.py. The raw tests call Context.perf, never the
falling-back checker, so a JH_EUNSUPPORTED on these inputs fails the test.
Every comparison of the raw outputs is integer and exact; the end-to-end tests
compare the plot maps of the device path and of the literal host path with ==,
doubles included."""
import numpy as np
import pytest

from jepsen_amd import _abi as A
from jepsen_amd import _native, checker, perf as P, synth
from jepsen_amd.history import Columns
from perf_cases import CASES, EXPECT, reference_cases, series_of
from perf_ref import LISTS, SCALARS, bucket, ref_cols

pytestmark = pytest.mark.gpu

T = A.PERF_TILE
S = 10 ** 9
F_COUNT = 19


def columns(proc, typ, f, names=()):
    n = len(proc)
    z = np.zeros(n, np.int64)
    return Columns(n=n, process=np.asarray(proc, np.int64), type=np.asarray(typ, np.int64), f=np.asarray(f, np.int64),
                   key=z, value=z, value2=z, n_keys=0, aux=np.zeros(1, np.int64), f_names=list(names))


def same(got, want, what=""):
    assert want["rc"] == A.JH_OK
    assert {k: got[k] for k in SCALARS} == {k: want[k] for k in SCALARS}, what
    for k in LISTS:
        assert got[k].tolist() == want[k].tolist(), (what, k)


def agree(ctx, cols, t, **kw):
    kw.setdefault("f_count", F_COUNT)
    want = ref_cols(cols, t, **kw)
    same(ctx.perf(cols, np.asarray(t, np.int64), **kw), want)
    return want


def on_device(ctx, cols, t, **kw):
    from hipcols import DevCols
    kw.setdefault("f_count", F_COUNT)
    d = DevCols(cols, 0)
    dt = DevCols(columns(t, t, t), 0)                 # the time column rides as a column of its own
    return ctx.perf(d, dt.process, on_device=True, **kw)


def paired(n, layout, seed=0):
    """n rows of invoke / completion pairs (an odd n ends on a lone invoke):
    one process; every op a process of its own; 5 processes round-robin, five
    invokes then their five completions."""
    rng = np.random.default_rng(seed + n)
    n_ops = (n + 1) // 2
    if layout == "rr5":
        blk = np.arange(n_ops) // 5
        within = np.arange(n_ops) % 5
        size = np.minimum(5, n_ops - blk * 5)
        inv_row, cmp_row = blk * 10 + within, blk * 10 + size + within
        proc_op = within
    else:
        inv_row, cmp_row = 2 * np.arange(n_ops), 2 * np.arange(n_ops) + 1
        proc_op = np.zeros(n_ops, np.int64) if layout == "one" else np.arange(n_ops)
    m = 2 * n_ops
    proc, typ, f = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64)
    proc[inv_row] = proc[cmp_row] = proc_op
    typ[cmp_row] = rng.integers(1, 4, n_ops)
    f[inv_row] = f[cmp_row] = rng.integers(0, 3, n_ops)
    t = np.arange(m, dtype=np.int64) * 700_000_000 + rng.integers(0, 1000, m)
    keep = np.ones(m, bool)
    if n % 2:
        keep[cmp_row[-1]] = False                      # the last op never completes
    return columns(proc[keep], typ[keep], f[keep]), t[keep]


# -- the hand-written cases ---------------------------------------------------
@pytest.mark.parametrize("name", list(CASES) + ["history21"])
def test_hand_written_cases_host_and_device_pointers(ctx, name):
    h = reference_cases()["history21"]["ops"] if name == "history21" else CASES[name]
    cols, t = P.encode_rows(h), P.time_column(h)
    fc = A.F_FIRST_INTERNED + len(cols.f_names)
    want = agree(ctx, cols, t, f_count=fc)
    same(on_device(ctx, cols, t, f_count=fc), want, "device pointers")
    if name == "history21":
        ref = reference_cases()["history21"]
        assert want["pair"].tolist() == ref["pair"]
        lat = t[want["pair"]] - t
        assert {int(k): v for k, v in ref["latency_of_invoke"].items()} == \
            {i: int(lat[i]) for i in range(len(h)) if h[i]["type"] == "invoke"}


@pytest.mark.parametrize("name", list(CASES))
def test_hand_written_cases_through_the_checker(ctx, name):
    h = CASES[name]
    dev, host = checker.perf(), checker.perf(force_host=True)
    rd, rh = dev.check({"name": "t"}, h, {}), host.check({"name": "t"}, h, {})
    assert {k: (v if k == "valid?" else v["valid?"]) for k, v in rd.items()} == \
        {k: (v if k == "valid?" else v["valid?"]) for k, v in rh.items()}
    for key in ("latency-graph", "rate-graph"):
        assert dev.checker_map[key].last_path == "device" and host.checker_map[key].last_path == "host"
        assert dev.checker_map[key].last_plots == host.checker_map[key].last_plots, key
    plots = dict(dev.checker_map["latency-graph"].last_plots, **dev.checker_map["rate-graph"].last_plots)
    for plot, want in EXPECT[name].items():
        if isinstance(want, type):
            assert plot not in plots and want.__name__ in rd["latency-graph"]["error"]
            assert "index 0 " in rd["latency-graph"]["error"]      # first_unpaired_invoke
        else:
            assert series_of(plots[plot]) == want, plot


# -- sizes and process layouts --------------------------------------------------
@pytest.mark.parametrize("layout", ["one", "own", "rr5"])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1])
def test_rows_and_process_layouts(ctx, n, layout):
    cols, t = paired(n, layout)
    assert cols.n == n
    want = agree(ctx, cols, t)
    assert want["n_invokes"] == (n + 1) // 2 and want["n_unpaired_invokes"] == n % 2
    assert want["has_quantiles"] == (0 if n % 2 or n == 0 else 1)


@pytest.mark.parametrize("other", [0, 1])
def test_pair_across_a_tile_edge(ctx, other):
    """Process 7's run in the per-process order: an orphan completion in slot
    0, then pairs, so that slot T - 1 is an invoke and slot T its completion.
    other: rows of process 9 stand between them in history order."""
    n7 = T + 5
    typ7 = np.where(np.arange(n7) % 2 == 1, A.TYPE_INVOKE, A.TYPE_OK)
    proc, typ = [], []
    for i in range(n7):
        proc.append(7)
        typ.append(int(typ7[i]))
        if other:
            proc.append(9)
            typ.append(A.TYPE_INVOKE if i % 2 == 0 and i + 1 < n7 else A.TYPE_FAIL)
    cols = columns(proc, typ, np.arange(len(proc)) % 2)
    t = np.arange(len(proc), dtype=np.int64) * 1000
    want = agree(ctx, cols, t)
    rows7 = np.nonzero(cols.process == 7)[0]
    assert typ7[T - 1] == A.TYPE_INVOKE and want["pair"][rows7[T - 1]] == rows7[T] and want["pair"][rows7[T]] == rows7[T - 1]
    assert want["pair"][rows7[0]] == -1 and want["n_unpaired_invokes"] == 0


def test_processes_of_63_bits_and_a_negative_latency(ctx):
    procs = np.asarray([-(1 << 62), (1 << 62) + 5, -2, -1, 0, 2 ** 40], np.int64)
    proc = np.tile(np.repeat(procs, 1), 40)
    typ = np.repeat(np.tile([A.TYPE_INVOKE, A.TYPE_INFO], 20), len(procs))
    rng = np.random.default_rng(3)
    t = rng.integers(0, 50 * S, len(proc))              # times wander: about half the latencies are negative
    want = agree(ctx, columns(proc, typ, proc % 3), t)
    assert want["n_paired"] == 20 * len(procs) and (t[want["pair"]] - t)[typ == A.TYPE_INVOKE].min() < 0
    assert want["cells"][:, 3].sum() == 60                # the three processes >= 0 only


# -- quantile groups ------------------------------------------------------------
SIZES = [1, 2, 19, 20, 21, 63, 64, 65, 99, 100, 101, 255, 256, 257]


def group_history(groups, seed=1):
    """groups: (f, bucket, size). Every op has a process of its own, invokes at
    bucket * 30 s + a few ns, latencies a shuffled permutation of 1000, 2000,
    ... over the whole history, so every pick is distinguishable. Rows: the
    groups' invokes interleaved round-robin, then the completions."""
    rng = np.random.default_rng(seed)
    n_ops = sum(s for _, _, s in groups)
    lat = (rng.permutation(n_ops) + 1) * 1000
    f_op = np.concatenate([np.full(s, f) for f, _, s in groups])
    b_op = np.concatenate([np.full(s, b) for _, b, s in groups])
    k_op = np.concatenate([np.arange(s) for _, _, s in groups])
    order = np.lexsort((np.arange(n_ops), k_op))        # round-robin over the groups
    f_op, b_op = f_op[order], b_op[order]
    t_inv = b_op * 30 * S + np.arange(n_ops)
    proc = np.concatenate([np.arange(n_ops), np.arange(n_ops)])
    typ = np.concatenate([np.zeros(n_ops, np.int64), np.full(n_ops, A.TYPE_OK)])
    return columns(proc, typ, np.concatenate([f_op, f_op])), np.concatenate([t_inv, t_inv + lat])


@pytest.mark.parametrize("size", SIZES)
def test_one_quantile_group(ctx, size):
    cols, t = group_history([(2, 0, size)])
    want = agree(ctx, cols, t)
    lat = np.sort(t[size:] - t[:size])
    idx = [min(size - 1, int(np.floor(size * q))) for q in (0.5, 0.95, 0.99, 1.0)]
    assert want["groups"].tolist() == [[2, 0, size] + lat[idx].tolist()]


def test_groups_as_consecutive_buckets_and_interleaved_fs(ctx):
    want = agree(ctx, *group_history([(2, b, s) for b, s in enumerate(SIZES)]))
    assert want["groups"][:, :3].tolist() == [[2, b, s] for b, s in enumerate(SIZES)]
    two = [(1 + (i % 2) * 4, i // 2, s) for i, s in enumerate(SIZES)]
    want = agree(ctx, *group_history(two, seed=2))
    assert want["groups"][:, :3].tolist() == sorted([f, b, s] for f, b, s in two)


def test_bucket_boundaries(ctx):
    ts = [k * dt * S + d for dt in (30, 10) for k in (1, 2, 3, 1000, 333333) for d in (-1, 0, 1)]
    n = len(ts)
    t = np.asarray(ts + ts, np.int64)                   # invoke and completion at the same time
    cols = columns(np.concatenate([np.arange(n), np.arange(n)]),
                   np.concatenate([np.zeros(n, np.int64), np.full(n, A.TYPE_OK)]), np.zeros(2 * n, np.int64))
    want = agree(ctx, cols, t)
    two_div = lambda dt: sorted(set((np.asarray(ts, np.float64) / 1e9 / float(dt)).astype(np.int64).tolist()))   # noqa: E731
    assert sorted(want["groups"][:, 1].tolist()) == two_div(30) == sorted(set(bucket(ts, 30).tolist()))
    assert sorted(want["cells"][:, 2].tolist()) == two_div(10)
    assert want["groups"][:, 2].sum() == n and want["cells"][:, 3].sum() == n
    other = agree(ctx, cols, t, dt_quantiles=7, dt_rate=3)
    assert sorted(other["groups"][:, 1].tolist()) == two_div(7) and sorted(other["cells"][:, 2].tolist()) == two_div(3)


# -- caps, masks, limits -----------------------------------------------------------
def test_caps(ctx):
    cols = synth.perf_history(3000, 6, seed=4, nemesis_every=400, mean_think_ms=150.0)
    want = ref_cols(cols, cols.time, f_count=F_COUNT)
    count = {"pair": cols.n, "pt_row": want["n_paired"], "series": want["n_series"], "groups": want["n_groups"],
             "cells": want["n_cells"]}
    assert all(c > 2 for c in count.values())
    for mode in ("zero", "one", "less"):
        caps = {k: {"zero": 0, "one": 1, "less": c - 1}[mode] for k, c in count.items()}
        got = ctx.perf(cols, cols.time, f_count=F_COUNT, pair_cap=caps["pair"], pt_cap=caps["pt_row"],
                       series_cap=caps["series"], group_cap=caps["groups"], cell_cap=caps["cells"])
        assert {k: got[k] for k in SCALARS} == {k: want[k] for k in SCALARS}, mode
        for k in LISTS:
            assert got[k].tolist() == want[k][:caps[k]].tolist(), (mode, k)


def test_want_masks(ctx):
    cols = synth.perf_history(3000, 6, seed=5, nemesis_every=400, mean_think_ms=150.0)
    full = ctx.perf(cols, cols.time, f_count=F_COUNT)
    for bit, lists in ((A.PERF_PAIR, ("pair",)), (A.PERF_POINTS, ("pt_row", "series")), (A.PERF_QUANTILES, ("groups",)),
                       (A.PERF_RATE, ("cells",))):
        got = ctx.perf(cols, cols.time, f_count=F_COUNT, want=bit)
        same(got, ref_cols(cols, cols.time, f_count=F_COUNT, want=bit), bit)
        for k in LISTS:
            assert got[k].tolist() == (full[k].tolist() if k in lists else []), (bit, k)


def test_limits(ctx):
    cols, t = paired(64, "rr5")
    agree(ctx, cols, t)

    def refused(c, tt, fc, word):
        assert ref_cols(c, tt, f_count=fc)["rc"] == A.JH_EUNSUPPORTED
        with pytest.raises(_native.JhError) as e:
            ctx.perf(c, tt, f_count=fc)
        assert e.value.code == A.JH_EUNSUPPORTED and word in e.value.msg
    for bad in (A.NIL, -1):
        t2 = t.copy()
        t2[17] = bad
        refused(cols, t2, F_COUNT, "time")
    refused(cols, t, int(cols.f.max()), "f code")            # an f code equal to f_count
    agree(ctx, cols, t, f_count=int(cols.f.max()) + 1)
    with pytest.raises(_native.JhError) as e:
        ctx.perf(cols, t, f_count=0)
    assert e.value.code == A.JH_EINVAL


# -- end to end ----------------------------------------------------------------------
@pytest.mark.parametrize("dangling", [False, True])
def test_checker_perf_device_path_equals_host_path(ctx, dangling):
    cols = synth.perf_history(4000, 7, fs=("read", "write", "cas", "ping"), seed=9, nemesis_every=500, dangling=dangling,
                              mean_think_ms=120.0)
    ops = synth.perf_columns_to_ops(cols)
    spec = [{"name": "partition", "color": "#aa3311", "start": {"start"}, "stop": {"stop"}}]
    test = {"name": "perf-e2e", "plot": {"nemeses": spec}}
    host = checker.perf(force_host=True)
    rh = host.check(test, ops, {})
    assert rh["rate-graph"] == {"valid?": True} and rh["latency-graph"]["valid?"] == ("unknown" if dangling else True)
    for history in (cols, ops):
        dev = checker.perf()
        rd = dev.check(test, history, {})
        assert rd["valid?"] == rh["valid?"] and rd["rate-graph"] == rh["rate-graph"]
        for key in ("latency-graph", "rate-graph"):
            assert dev.checker_map[key].last_path == "device"
            assert dev.checker_map[key].last_plots == host.checker_map[key].last_plots, key
    plots = host.checker_map["latency-graph"].last_plots
    assert list(plots) == (["latency-raw"] if dangling else ["latency-raw", "latency-quantiles"])
    if not dangling:
        assert len(plots["latency-quantiles"]["series"][0]["data"]) > 1          # more than one 30 s bucket
    assert len(host.checker_map["rate-graph"].last_plots["rate"]["series"][0]["data"]) > 3
