"""Monotonic-key measurement (jepsen/src/jepsen/tests/cycle.clj: monotonic-key-graph
under cycle/checker; the increment workload of tidb/src/tidb/monotonic.clj) on
one MI355X: jepsen_amd/synth.py monotonic_history in three shapes.
  chain   every op an :inc, every value unique: groups of one row
  inc8    the increment workload at 8 keys, half of the ops reads
  wide    2 keys, nearly every op a read: a few values, groups of hundreds of rows

One JSON line per shape and mask (MONOTONIC alone, MONOTONIC | REALTIME). The
history is resident in HBM before the timed region; a step is one
jh_check_cycle call asking for what the checker mirror asks for (labels, 8 SCCs).
  value          rows per second of the device route
  edges_per_s    the same call, in edges built
  routes         the device route against the route without the device builder:
                 the host closed form's edges (cycle.map_edges) handed in as
                 extra edges with the same other analyzers, host to host, the
                 edge build and its upload included. Both are timed in this
                 process, alternating, after warm-up; every step's time is listed in
                 run order (value and ms_per_step are means over the steps)
  cpu_baseline   this module's host path (map_edges, realtime_edges, scc_labels;
                 one host thread), and whether labels, counts and the edge
                 multiset agree with the device's. With REALTIME the host's
                 Tarjan over the back-edge regions takes minutes at these sizes:
                 that line's baseline is taken only with --cpu-realtime
  kernels        with --profile: ms per step of every kernel of the MONOTONIC
                 call, from a kernel trace of a fresh child process (a run of its
                 own: tracing slows the call), and k_mo_fill's achieved write
                 bytes/s (8 B per edge over its own kernel time)

    python tools/bench_cycle_mono.py [--ops 200000] [--wide-ops 40000] [--procs 10] [--shapes chain inc8 wide]
                                     [--steps 5] [--warmup 3] [--no-cpu] [--cpu-realtime] [--profile DIR]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_c2 import DevCols   # noqa: E402
from bench_cycle_append import kernel_times   # noqa: E402


def shape_args(args, shape):
    """(n_ops, keys, p_read) of monotonic_history for a shape."""
    if shape == "chain":
        return args.ops, 8, 0.0
    if shape == "inc8":
        return args.ops, 8, 0.5
    return args.wide_ops, 2, 1.0 - 80.0 / args.wide_ops         # about 40 values a key


def profile(args, shape, out_dir):
    """One shape's MONOTONIC call in a fresh child under the kernel trace (steps calls, no warm-up outside them)."""
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__),
           "--ops", str(args.ops), "--wide-ops", str(args.wide_ops), "--procs", str(args.procs), "--shapes", shape,
           "--steps", str(args.steps), "--warmup", "0", "--no-cpu", "--child"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        return {"error": r.stdout[-400:]}
    out = kernel_times(out_dir, args.steps)
    return out if out else {"error": "no kernel statistics under " + out_dir + ": " + " ".join(sorted(os.listdir(out_dir)))[:300]}


def spread(xs):
    """Every step's time in run order, and their smallest, median and largest."""
    o = sorted(xs)
    return {"min_ms": o[0] * 1e3, "median_ms": o[len(o) // 2] * 1e3, "max_ms": o[-1] * 1e3, "steps_ms": [round(x * 1e3, 3) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=200000, help="ops of the chain and inc8 shapes (two rows each)")
    ap.add_argument("--wide-ops", type=int, default=40000, help="ops of the wide shape")
    ap.add_argument("--procs", type=int, default=10)
    ap.add_argument("--shapes", nargs="*", default=["chain", "inc8", "wide"], choices=["chain", "inc8", "wide"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-realtime", action="store_true", help="the host baseline of the MONOTONIC | REALTIME lines too (minutes)")
    ap.add_argument("--profile", metavar="DIR", help="also trace each shape's kernels in a child process, output under DIR")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    import numpy as np
    import torch
    from jepsen_amd import _abi as A
    from jepsen_amd import _native, synth
    from jepsen_amd import cycle as CY
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    MO, RT = A.CY_MONOTONIC, A.CY_REALTIME

    def clock(fn):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    def words(e):
        return np.sort((e[:, 0] << 32) | e[:, 1])

    for shape in args.shapes:
        n_ops, keys, p_read = shape_args(args, shape)
        t0 = time.perf_counter()
        cols = synth.monotonic_history(n_ops, args.procs, keys, p_read, 0.0, 0.02, seed=11)
        gen_s = time.perf_counter() - t0
        d = DevCols(cols, dev)
        if args.child:
            for _ in range(args.steps):
                ctx.check_cycle(d, MO, on_device=True)
            torch.cuda.synchronize()
            continue
        kernels = profile(args, shape, os.path.join(args.profile, shape)) if args.profile else None
        for mask in (MO, MO | RT):
            def device_route():
                return ctx.check_cycle(d, mask, on_device=True)

            def extra_route():
                e = CY.map_edges(cols)
                return ctx.check_cycle(d, mask & ~MO, extra=(e[:, 0], e[:, 1]), on_device=True)
            for _ in range(args.warmup):
                device_route()
                extra_route()
            t_dev, t_x = [], []
            for _ in range(args.steps):
                r, t = clock(device_route)
                t_dev.append(t)
                rx, t = clock(extra_route)
                t_x.append(t)
            sec = sum(t_dev) / len(t_dev)
            sec_x = sum(t_x) / len(t_x)
            edges = sum(r["edge_count"])
            same_answer = bool(r["labels"].tolist() == rx["labels"].tolist() and sum(rx["edge_count"]) == edges
                               and (r["valid"], r["scc_count"]) == (rx["valid"], rx["scc_count"]))
            cpu = None
            if not args.no_cpu and (mask == MO or args.cpu_realtime):
                e = ctx.check_cycle(d, mask, on_device=True, edge_cap=edges, scc_cap=0)["edges"]
                t0 = time.perf_counter()
                he = CY.map_edges(cols)
                n_mono = len(he)
                if mask & RT:
                    he = np.concatenate([he, CY.realtime_edges(np.asarray(cols.process), np.asarray(cols.type))])
                labels = CY.scc_labels(cols.n, he)
                ct = time.perf_counter() - t0
                cpu = {"value": cols.n / ct, "unit": "rows/s", "seconds": ct, "speedup": ct / sec,
                       "kind": "jepsen_amd/cycle.py host path (map_edges, realtime_edges, scc_labels), one thread",
                       "parity": bool(labels.tolist() == r["labels"].tolist() and n_mono == r["edge_count"][2] and len(he) == edges
                                      and np.array_equal(words(he), words(e)))}
            line = {
                "metric": f"history rows checked/sec, monotonic-key cycle checker ({shape}, "
                          f"{'MONOTONIC | REALTIME' if mask & RT else 'MONOTONIC'})",
                "value": cols.n / sec, "unit": "rows/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": sec * 1e3, "higher_is_better": True, "dtype": "int64", "edges_per_s": edges / sec,
                "data": f"synthetic (jepsen_amd/synth.py monotonic_history, {n_ops} ops, {args.procs} processes, {keys} keys, "
                        f"p_read {p_read:.4f}, p_info 0.02, seed 11)",
                "config": {"shape": shape, "rows": int(cols.n), "pairs": r["entries"], "edges": edges, "edge_count": r["edge_count"],
                           "valid": r["valid"], "scc_count": r["scc_count"], "path": r["path"], "device_ms": r["device_ms"],
                           "gen_s": round(gen_s, 1)},
                "routes": {"device": spread(t_dev), "extra_edges_from_host": spread(t_x), "extra_over_device": sec_x / sec,
                           "extra_over_device_medians": sorted(t_x)[len(t_x) // 2] / sorted(t_dev)[len(t_dev) // 2],
                           "same_answer": same_answer},
                "cpu_baseline": cpu}
            if mask == MO:
                fill_ms = (kernels or {}).get("k_mo_fill")
                if isinstance(fill_ms, float) and fill_ms > 0:
                    kernels["fill_write_bytes_per_s"] = 8 * r["edge_count"][2] / (fill_ms / 1e3)
                line["kernels"] = kernels
            print(json.dumps(line), flush=True)
        del d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
