"""checker/perf without a GPU: the literal transcriptions of
jepsen.checker.perf (jepsen_amd/perf.py) against the recorded results of the
reference's own unit tests and against hand-written cases, the numpy closed
form of jh_perf's outputs (perf_ref.ref_cols) against the transcriptions on
random histories, one test per detail of the plot assembly, and the ABI
layout of jh_perf's structs."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from jepsen_amd import _abi as A
from jepsen_amd import checker, perf as P, synth
from perf_cases import CASES, EXPECT, S, nem, op, reference_cases, series_of
from perf_ref import bucket, pick_index, ref_cols

REF = reference_cases()


def frac(x):
    return Fraction(x) if isinstance(x, str) else x


# -- the reference's unit tests, as recorded data ---------------------------
def test_bucket_points_reference_test():
    c = REF["bucket_points"]
    got = P.bucket_points(c["dt"], c["points"])
    assert [[k, v] for k, v in got.items()] == c["expect"]


def test_latencies_to_quantiles_reference_test():
    c = REF["latencies_to_quantiles"]
    got = P.latencies_to_quantiles(c["dt"], c["qs"], c["points"])
    want = {int(q): [[frac(t), v] for t, v in pts] for q, pts in c["expect"].items()}
    assert got == want
    assert P.bucket_time(5, 1) == Fraction(5, 2) and isinstance(P.bucket_time(5, 1), Fraction)
    assert P.bucket_time(30, 61.5) == 75 and isinstance(P.bucket_time(30, 61.5), int)


def test_history_to_latencies_reference_history():
    c = REF["history21"]
    h = P.history_to_latencies(c["ops"])
    assert len(h) == 21
    want = {int(k): v for k, v in c["latency_of_invoke"].items()}
    for i, o in enumerate(h):
        partner = c["pair"][i]
        if o["type"] == "invoke":
            assert o["latency"] == want[i] == c["ops"][partner]["time"] - o["time"]
            assert o["completion"]["time"] == c["ops"][partner]["time"] and o["completion"]["latency"] == want[i]
        elif partner >= 0:
            assert o["latency"] == want[partner]
        else:
            assert "latency" not in o
    cols, t = P.encode_rows(c["ops"]), P.time_column(c["ops"])
    r = ref_cols(cols, t)
    assert r["pair"].tolist() == c["pair"] and r["n_paired"] == 10 and r["n_unpaired_invokes"] == 0


# -- the closed form against the transcription ------------------------------
def random_history(rng, n, dirty):
    """Client ops of processes 0..3, -2's stand-in "odd" (a keyword process)
    and 2**40, nemesis rows and, when dirty, double invokes, orphan completions
    and a nemesis invoke; times wander, so a latency may be negative."""
    procs = [0, 1, 2, 3, "odd", 2 ** 40, "nemesis"]
    fs = ["read", "write", "cas", "weird"]
    h, open_ = [], {}
    t = 0
    for _ in range(n):
        p = procs[rng.integers(len(procs))]
        t += int(rng.integers(-2 * S, 9 * S))
        t = max(t, 0)
        if p == "nemesis" and not (dirty and rng.random() < 0.3):
            h.append(op(p, "info", ["start", "stop"][rng.integers(2)], t))
            continue
        if dirty:
            ty = ["invoke", "ok", "fail", "info"][rng.integers(4)]
            h.append(op(p, ty, fs[rng.integers(len(fs))], t))
        elif p in open_:
            h.append(op(p, ["ok", "fail", "info"][rng.integers(3)], open_.pop(p), t))
        else:
            open_[p] = fs[rng.integers(len(fs))]
            h.append(op(p, "invoke", open_[p], t))
    if not dirty:                                   # close what is open
        for p, f in open_.items():
            h.append(op(p, "ok", f, t + 1))
    return h


def encode_with_odd(h):
    """encode_rows, with the keyword process as -2 (the column's encoding)."""
    cols = P.encode_rows(h)
    assert set(np.unique(cols.process).tolist()) <= {-2, -1, 0, 1, 2, 3, 2 ** 40}
    return cols, P.time_column(h)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("dirty", [False, True])
def test_closed_form_against_the_transcription(seed, dirty):
    rng = np.random.default_rng(seed)
    h = random_history(rng, 400, dirty)
    cols, t = encode_with_odd(h)
    names = P.f_names(cols)
    code = {v: k for k, v in names.items()}
    r = ref_cols(cols, t)
    lat = P.history_to_latencies(h)
    # pairing
    for i, o in enumerate(lat):
        if o["type"] == "invoke" and "completion" in o:
            j = int(r["pair"][i])
            assert j >= 0 and o["latency"] == h[j]["time"] - h[i]["time"] and r["pair"][j] == i
            assert {k: v for k, v in o["completion"].items() if k != "latency"} == h[j]
        elif o["type"] == "invoke":
            assert r["pair"][i] == -1
        elif "latency" not in o:
            assert r["pair"][i] == -1
    unp = [i for i, o in enumerate(lat) if o["type"] == "invoke" and "latency" not in o]
    assert r["n_unpaired_invokes"] == len(unp) and r["first_unpaired_invoke"] == (unp[0] if unp else -1)
    assert r["n_invokes"] == sum(o["type"] == "invoke" for o in h) and r["t_max"] == max(o["time"] for o in h)
    # raw points: f ascending by code, :ok :info :fail, row ascending
    by = P.invokes_by_f_type(lat)
    pos = {id(o): i for i, o in enumerate(lat)}
    want_rows, want_series = [], []
    for c in sorted(code[f] for f in by):
        for ty in ("ok", "info", "fail"):
            rows = [pos[id(o)] for o in by[names[c]][ty]]
            if rows:
                want_rows += rows
                want_series.append([c, {"ok": A.TYPE_OK, "info": A.TYPE_INFO, "fail": A.TYPE_FAIL}[ty], len(rows)])
    assert r["pt_row"].tolist() == want_rows and r["series"].tolist() == want_series
    # quantile groups against latencies->quantiles over integer points
    if not unp:
        want = []
        for c in sorted(code[f] for f in P.invokes_by_f(lat)):
            ops = P.invokes_by_f(lat)[names[c]]
            q = P.latencies_to_quantiles(30, P.QS, [[P.nanos_to_secs(o["time"]), o["latency"]] for o in ops])
            counts = {k: len(v) for k, v in P.bucket_points(30, [[P.nanos_to_secs(o["time"]), 0] for o in ops]).items()}
            for j, (mid, v) in enumerate(q[0.5]):
                want.append([c, (mid - 15) // 30, counts[mid], v, q[0.95][j][1], q[0.99][j][1], q[1][j][1]])
        assert r["has_quantiles"] == 1 and r["groups"].tolist() == want
    else:
        assert r["has_quantiles"] == 0 and r["n_groups"] == 0
    # rate cells against the reference's reduce, counting instead of adding td
    cells = {}
    for o in h:
        if o["type"] != "invoke" and P.H._is_int(o["process"]):
            k = (code[o["f"]], P.H.TYPES[o["type"]], (P.bucket_time(10, P.nanos_to_secs(o["time"])) - 5) // 10)
            cells[k] = cells.get(k, 0) + 1
    assert r["cells"].tolist() == [list(k) + [cells[k]] for k in sorted(cells)]


def test_ref_limits_and_empty():
    cols, t = encode_with_odd(CASES["basic"])
    assert ref_cols(cols, t)["rc"] == A.JH_OK
    for bad in (A.NIL, -1):
        t2 = t.copy()
        t2[3] = bad
        assert ref_cols(cols, t2)["rc"] == A.JH_EUNSUPPORTED
    assert ref_cols(cols, t, f_count=1)["rc"] == A.JH_EUNSUPPORTED          # write's code 1 == f_count
    e = ref_cols(P.encode_rows([]), np.zeros(0, np.int64))
    assert e["rc"] == A.JH_OK and all(e[k] == 0 for k in ("n_invokes", "n_series", "n_groups", "n_cells", "t_max"))


def test_bucket_is_two_divisions_and_pick_is_one_multiply():
    for dt in (30, 10):
        for k in (1, 2, 3, 1000, 333333):
            for d in (-1, 0, 1):
                t = k * dt * S + d
                assert bucket([t], dt)[0] == int((float(t) / 1e9) / float(dt))
    # floor(n * q) in doubles is not n * 95 // 100: 100 * 0.95 rounds to 95, 20 * 0.95 to 19
    assert [pick_index(n, 0.95) for n in (1, 2, 19, 20, 21, 100, 101)] == [0, 1, 18, 19, 19, 95, 95]
    assert pick_index(7, 1.0) == 6 and P.quantiles([0.95], list(range(20)))[0.95] == 19


# -- hand-written cases, host path -------------------------------------------
def host_plots(h, test=None, opts=None):
    ck = checker.perf(opts, force_host=True)
    res = ck.check(test or {"name": "t"}, h, {})
    plots = dict(ck.checker_map["latency-graph"].last_plots, **ck.checker_map["rate-graph"].last_plots)
    return res, plots


@pytest.mark.parametrize("name", list(CASES))
def test_hand_written_cases_host_path(name):
    res, plots = host_plots(CASES[name])
    for plot, want in EXPECT[name].items():
        if isinstance(want, type):
            assert plot not in plots and res["latency-graph"]["valid?"] == "unknown"
            assert want.__name__ in res["latency-graph"]["error"]
        else:
            assert series_of(plots[plot]) == want, plot
            assert all(type(a) is type(b) for s, w in zip(series_of(plots[plot]), want)
                       for p, q in zip(s[2], w[2]) for a, b in zip(p, q)), plot
    assert res["rate-graph"] == {"valid?": True}
    assert res["valid?"] == ("unknown" if TypeError in EXPECT[name].values() else True)


def test_plot_map_keys_and_styles():
    _, plots = host_plots(CASES["basic"])
    raw, qs, rate = plots["latency-raw"], plots["latency-quantiles"], plots["rate"]
    assert raw["draw-fewer-on-top?"] is True and raw["logscale"] == "y" and qs["logscale"] == "y" and "logscale" not in rate
    assert [s["with"] for s in raw["series"]] == ["points"] * 3 and {s["with"] for s in qs["series"]} == {"linespoints"}
    assert [s["linetype"] for s in raw["series"]] == [["rgb", "#81BFFC"], ["rgb", "#FFA400"], ["rgb", "#FF1E90"]]
    # qs->colors: the quantiles sorted descending take red, orange, purple, blue
    assert [s["linetype"][1] for s in qs["series"][:4]] == ["blue", "purple", "orange", "red"]
    assert raw["preamble"][:4] == [["set", "output", "latency-raw.png"], ["set", "term", "png", "truecolor", "size", (900, 400)],
                                   ["set", "xlabel", "Time (s)"], ["set", "key", "outside", "top", "right"]]
    assert raw["preamble"][4:7] == [["set", "title", "t latency"], ["set", "ylabel", "Latency (ms)"], ["set", "logscale", "y"]]
    assert rate["preamble"][4:6] == [["set", "title", "t rate"], ["set", "ylabel", "Throughput (hz)"]]
    assert raw["yrange"] == [500.0, 9000.0]                   # logscale: not broadened
    assert raw["xrange"] == P.broaden_range([1.0, 12.0]) and rate["yrange"] == P.broaden_range([0, 0.1])


def test_x_is_one_division_and_y_is_ratio_double():
    t, lat = 12345678901234567, 1234567
    o = {"time": t, "latency": lat}
    assert P.latency_point(o) == [float(t) / 1e9, lat / 1e6]
    assert P.latency_ms([lat, -1500000]).tolist() == [P.ratio_double(Fraction(lat, 10 ** 6)), -1.5]
    assert P.ratio_double(Fraction(1, 3)) == 0.3333333333333333 and P.ratio_double(Fraction(4, 2)) == 2.0
    # below 2^53 the Ratio rule and the correctly rounded quotient agree
    rng = np.random.default_rng(0)
    for x in rng.integers(-(1 << 53) + 1, 1 << 53, 2000).tolist():
        assert P.ratio_double(P.nanos_to_ms(x)) == x / 1e6, x


def test_rate_y_is_a_running_sum_not_a_product():
    td = P.ratio_double(Fraction(1, 10))
    acc, sums = 0, {}
    for c in range(1, 1001):
        acc = td + acc
        sums[c] = acc
    run = np.add.accumulate(np.full(1000, td))
    for c in (1, 2, 3, 10, 1000):
        assert run[c - 1] == sums[c]
    # what the running sum guards: ten additions of 0.1 give 0.9999999999999999, the product 1.0
    assert sums[10] == 0.9999999999999999 != 10 * 0.1 and sums[1000] != 1000 * 0.1
    h = []
    for i in range(10):
        h += [op(i, "invoke", "read", S), op(i, "ok", "read", 6 * S)]
    _, plots = host_plots(h)
    assert series_of(plots["rate"])[0][2] == [[5, 0.9999999999999999]]


def test_dropped_last_rate_bucket():
    h = [op(0, "invoke", "read", 10 * S), op(0, "ok", "read", 11 * S), op(0, "invoke", "read", 11 * S), op(0, "ok", "read", 12 * S)]
    _, plots = host_plots(h)
    assert P.buckets(10, 12.0) == [5]
    assert [s[2] for s in series_of(plots["rate"])] == [[[5, 0]]] * 3       # both ops sit in bucket 15 > t-max


def test_unpaired_invoke_raises_after_the_raw_plot(tmp_path):
    ck = checker.latency_graph(force_host=True)
    with pytest.raises(TypeError):
        ck.check({"name": "t", "store-dir": str(tmp_path)}, CASES["unpaired"], {})
    assert list(ck.last_plots) == ["latency-raw"] and os.path.exists(tmp_path / "latency-raw.gp")
    assert not os.path.exists(tmp_path / "latency-quantiles.gp")


def test_failed_asserts():
    for ck in (checker.latency_graph(force_host=True), checker.rate_graph(force_host=True)):
        with pytest.raises(AssertionError, match=r"\(seq data\)"):
            ck.check({}, [], {})
    with pytest.raises(AssertionError, match=r"\(seq data\)"):     # nemesis rows only: no series at all
        checker.latency_graph(force_host=True).check({}, nem("start", S), {})
    with pytest.raises(AssertionError, match="Series has no :data points"):
        P.plot_commands({"series": [{"title": "a", "with": "points", "data": []}]})
    assert checker.check_safe(checker.rate_graph(force_host=True), {}, [], {})["valid?"] == "unknown"


def test_polysort_and_name_plus():
    assert P.polysort(["write", 7, None, "read", 3]) == [None, "read", "write", 3, 7]
    assert [P.name_plus(x) for x in ("read", 7, None, P.Q("s"), True)] == [":read", "7", "nil", '"s"', "true"]
    assert P.fs_to_points(["a", "b", "c"]) == {"a": 4, "b": 6, "c": 8}


def test_broaden_range_and_math_round():
    assert P.broaden_range([3, 3]) == [2, 4]
    assert P.math_round(0.5) == 1 and P.math_round(-0.5) == 0 and P.math_round(2.5) == 3 and round(2.5) == 2
    assert P.broaden_range([1.0, 12.0]) == [1.0, 12.0] and P.broaden_range([0.0, 133.2]) == [0.0, 140.0]
    # scale 0.01: 0.1 mod 0.01 is 0.00999..., not "super close", and 0.01 + (0.1 - 0.00999...) is 0.1 again
    assert P.broaden_range([0, 0.1]) == [0, 0.1]
    assert P.broaden_range([5, 35]) == [5, 35]                # grid 3: scale 1.0; 35 mod 1.0 = 0.0 keeps b, a' = 5 - 0.0


def test_nemesis_activity_series_and_regions():
    h = CASES["nemesis"]
    iv = P.nemesis_intervals(h)
    assert [[a["time"], b and b["time"]] for a, b in iv] == [[S, 4 * S], [S, 4 * S], [5 * S, None], [5 * S, None]]
    spec = [{"name": "part", "color": "#123456", "start": {"start"}, "stop": {"stop"}}]
    _, plots = host_plots(h, opts={"nemeses": spec})
    raw = plots["latency-raw"]
    assert raw["series"][-1] == {"title": "part", "with": "lines", "linecolor": ["rgb", "#123456"], "linewidth": 6,
                                 "data": [[-1, -1]]}
    rects = [c for c in raw["preamble"] if c[:3] == ["set", "obj", "rect"]]
    arrows = [c for c in raw["preamble"] if c[:2] == ["set", "arrow"]]
    assert len(rects) == 4 and rects[0][4] == (1.0, ["graph", 1 - 0.0834 + 0.00615]) and rects[2][6][0] == raw["xrange"][1]
    assert [c[3][0] for c in arrows] == [t for t in (1.0, 1.0, 4.0, 4.0, 5.0, 5.0) if raw["xrange"][0] <= t <= raw["xrange"][1]]
    _, plots = host_plots(h, test={"name": "t", "plot": {"nemeses": spec}})      # from the test map
    assert plots["rate"]["series"][-1]["title"] == "part"
    _, plots = host_plots(h)                                                     # no spec: the default nemesis
    assert plots["rate"]["series"][-1]["title"] == "nemesis" and plots["rate"]["series"][-1]["linecolor"] == ["rgb", "#cccccc"]


def test_options_merge_and_subdirectory(tmp_path):
    ck = checker.rate_graph({"subdirectory": "a", "nemeses": []}, force_host=True)
    ck.check({"name": "t", "store-dir": str(tmp_path)}, CASES["basic"], {"subdirectory": "b"})     # c-opts win
    assert os.path.exists(tmp_path / "b" / "rate.gp") and not os.path.exists(tmp_path / "a")
    assert ck.last_plots["rate"]["preamble"][0] == ["set", "output", str(tmp_path / "b" / "rate.png")]


def test_draw_fewer_on_top_in_the_script(tmp_path):
    h = CASES["basic"] + [op(2, "invoke", "read", 2 * S), op(2, "ok", "read", 3 * S)]
    ck = checker.latency_graph(force_host=True)
    ck.check({"name": "t", "store-dir": str(tmp_path)}, h, {})
    raw = ck.last_plots["latency-raw"]
    cmds, data = P.plot_commands(raw)
    titled = [s for s in raw["series"]]
    n = len(titled)
    # first every series by point count descending (sort-by is stable, then reverse) without a title ...
    assert n == 3 and [len(d) for d in data[:n]] == [2, 1, 1] and data[0] == [[1.0, 2000.0], [2.0, 1000.0]]
    assert data[1:n] == [s["data"] for s in reversed(titled[1:])]
    # ... then the titled one-point dummies in series order
    assert data[n:] == [[[0, -1]]] * n
    parts = cmds[-1][1]
    assert cmds[-1][0] == "plot" and all("notitle" in p for p in parts[:n])
    assert [p[-1] for p in parts[n:]] == [["title", s["title"]] for s in titled]
    order = [c[:2] for c in cmds]
    assert order.index(["set", "logscale"]) < order.index(["set", "xrange"]) < order.index(["set", "yrange"]) < len(cmds) - 1
    text = open(tmp_path / "latency-raw.gp").read().splitlines()
    assert text[0] == 'set output "%s"' % (tmp_path / "latency-raw.png") and text[-1] == "e"
    assert text.index("1.0 2000.0") < text.index("0 -1") and text.count("e") == 2 * n
    assert text[len(cmds) - 1].startswith('plot "-" with points linetype rgb "#81BFFC" pointtype 4 notitle,')


def test_missing_gnuplot_is_logged_not_raised(tmp_path, monkeypatch, caplog):
    monkeypatch.setattr(P.shutil, "which", lambda name: None)
    with caplog.at_level("WARNING"):
        assert checker.rate_graph(force_host=True).check({"store-dir": str(tmp_path)}, CASES["basic"], {}) == {"valid?": True}
    assert "gnuplot" in caplog.text and os.path.exists(tmp_path / "rate.gp")


def test_synth_perf_history():
    cols = synth.perf_history(2000, 4, seed=1, nemesis_every=300, mean_think_ms=100.0)
    r = ref_cols(cols, cols.time)
    assert r["n_unpaired_invokes"] == 0 and r["n_paired"] == r["n_invokes"] == 1000
    assert (cols.process == -1).sum() == 2 * (2000 // 300) and {t for _, t, _ in r["series"].tolist()} == {1, 2, 3}
    for p in range(4):
        assert (np.diff(cols.time[cols.process == p]) > 0).all()
    d = synth.perf_history(2000, 4, seed=1, nemesis_every=300, dangling=True)
    r = ref_cols(d, d.time)
    assert r["n_unpaired_invokes"] == 1 and d.process[r["first_unpaired_invoke"]] == 3
    ops = synth.perf_columns_to_ops(cols)
    assert ops[0]["type"] == "invoke" and P.encode_rows(ops).f.tolist() == cols.f.tolist()


# -- the ABI ------------------------------------------------------------------
def test_ctypes_layout_of_the_perf_structs(tmp_path, built):
    header = os.path.join(ROOT, "include", "jh.h")
    prog = tmp_path / "szp.c"
    prog.write_text(f'''#include <stdio.h>
#include <stddef.h>
#include "{header}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(jh_perf_opts), offsetof(jh_perf_opts, want),
         offsetof(jh_perf_opts, reserved), sizeof(jh_perf_result), offsetof(jh_perf_result, t_max),
         offsetof(jh_perf_result, n_cells), offsetof(jh_perf_result, has_quantiles), offsetof(jh_perf_result, device_ms),
         JH_PERF_ALL, JH_ABI_VERSION);
  return 0; }}''')
    exe = tmp_path / "szp"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(A.JhPerfOpts), A.JhPerfOpts.want.offset, A.JhPerfOpts.reserved.offset, C.sizeof(A.JhPerfResult),
                   A.JhPerfResult.t_max.offset, A.JhPerfResult.n_cells.offset, A.JhPerfResult.has_quantiles.offset,
                   A.JhPerfResult.device_ms.offset, A.PERF_ALL, A.JH_ABI_VERSION]
    from jepsen_amd import _native
    assert hasattr(C.CDLL(_native.LIB_PATH), "jh_perf") and A.JH_ABI_VERSION == 8
