"""checker/perf measurement (jepsen/src/jepsen/checker/perf.clj) on one MI355X:
jh_perf over `--rows` rows of paired client ops on `--procs` processes
(jepsen_amd/synth.py perf_history), all four outputs wanted.

One JSON line. The history and its :time column are resident in HBM before the
timed region; a step is one jh_perf call with room for the whole result lists.
  device         `device_ms` of every step after the warm-up: the median and the
                 range; rows per second at the median; the algorithmic bytes over
                 it against the copy bandwidth measured in the same process (a
                 device-to-device copy of 1 GiB, read + write bytes over event
                 time, after a warm-up)
  algorithmic bytes, counted from the shapes: 32 B per row read (process, type, f,
                 time) and 8 B per row written (pair): what one pass that did all
                 the work at once would move. The sorts' traffic comes on top.
  numpy          tests/perf_ref.py ref_cols (the closed form) on the same rows
  literal        the transcription of the Clojure (perf.py point_graph,
                 quantiles_graph, rate_graph) on `--cpu-rows` rows, one thread
Per-kernel times: run the tool under `rocprofv3 --kernel-trace --stats`.

    python tools/bench_perf.py [--rows 10000000] [--procs 64] [--steps 7] [--warmup 2] [--cpu-rows 200000] [--no-cpu]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_c2 import DevCols   # noqa: E402
from bench_causal_reverse import copy_bandwidth   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--procs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-rows", type=int, default=200_000)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    from jepsen_amd import _abi as A, _native, perf, synth
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    copy_gbs = copy_bandwidth(dev)
    print(f"# device-to-device copy: {copy_gbs:.0f} GB/s", file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    cols = synth.perf_history(args.rows, args.procs, seed=11, mean_think_ms=200.0)
    gen_s = time.perf_counter() - t0
    rows = int(cols.n)
    f_count = A.F_FIRST_INTERNED + len(cols.f_names)
    print(f"# generated {rows} rows in {gen_s:.1f} s", file=sys.stderr, flush=True)

    d = DevCols(cols, dev)
    t_dev = torch.from_numpy(cols.time).to(dev)
    call = lambda: ctx.perf(d, t_dev.data_ptr(), on_device=True, f_count=f_count, pair_cap=rows, pt_cap=rows,   # noqa: E731
                            series_cap=256, group_cap=1 << 16, cell_cap=1 << 18)
    for _ in range(args.warmup):
        r = call()
    ms, wall = [], []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        r = call()
        wall.append(time.perf_counter() - t0)
        ms.append(r["device_ms"])
    med = statistics.median(ms)
    alg = 40.0 * rows
    dev_gbs = alg / (med * 1e-3) / 1e9

    cpu = None
    if not args.no_cpu:
        from perf_ref import LISTS, SCALARS, ref_cols
        t0 = time.perf_counter()
        want = ref_cols(cols, cols.time, f_count=f_count)
        np_s = time.perf_counter() - t0
        same = all(r[k] == want[k] for k in SCALARS) and all(r[k].tolist() == want[k].tolist() for k in LISTS)
        small = synth.perf_history(min(args.cpu_rows, args.rows), args.procs, seed=11, mean_think_ms=200.0)
        ops = synth.perf_columns_to_ops(small)
        t0 = time.perf_counter()
        perf.point_graph({}, ops)
        perf.quantiles_graph({}, ops)
        perf.rate_graph({}, ops)
        lit_s = time.perf_counter() - t0
        cpu = {"numpy": {"seconds": np_s, "rows_per_s": rows / np_s, "equals_device": same},
               "literal": {"seconds": lit_s, "rows": int(small.n), "rows_per_s": small.n / lit_s}}
    print(json.dumps({
        "metric": "history rows reduced/sec, checker/perf (jh_perf, all four outputs)",
        "value": rows / (med * 1e-3), "unit": "rows/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "higher_is_better": True, "dtype": "int64",
        "data": f"synthetic (jepsen_amd/synth.py perf_history, {rows} rows, {args.procs} processes, seed 11)",
        "config": {"rows": rows, "procs": args.procs, "n_invokes": int(r["n_invokes"]), "n_paired": int(r["n_paired"]),
                   "n_series": int(r["n_series"]), "n_groups": int(r["n_groups"]), "n_cells": int(r["n_cells"]),
                   "t_max_s": r["t_max"] / 1e9, "gen_s": round(gen_s, 1)},
        "device": {"device_ms_median": med, "device_ms_min": min(ms), "device_ms_max": max(ms), "device_ms": ms,
                   "call_ms_median": statistics.median(wall) * 1e3, "algorithmic_bytes": alg, "achieved": dev_gbs,
                   "unit": "GB/s", "copy_bandwidth": copy_gbs, "frac_of_copy": dev_gbs / copy_gbs},
        "cpu_baseline": cpu,
        "speedup_vs_numpy": None if cpu is None else cpu["numpy"]["seconds"] / (med * 1e-3)}), flush=True)


if __name__ == "__main__":
    main()
