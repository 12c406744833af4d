"""List-append measurement (jepsen/src/jepsen/tests/cycle.clj: appends-and-reads-graph
under cycle/checker) on one MI355X: jepsen_amd/synth.py append_history at 10 and
at 100 processes, valid and with stale reads, read lengths bounded by 64 and by
1 024.

One JSON line per configuration. The history is resident in HBM before the timed
region; a step is one jh_check_cycle call asking for what the checker mirror
asks for (labels, 8 SCCs).
  value          rows per second of the JH_CY_APPEND call
  stages         ms per step of APPEND alone and of APPEND | REALTIME; edges/s
  bytes          the read elements plus the micro-op words, in bytes: what the
                 prefix compare and the record passes stream
  cpu_baseline   this module's host path (jepsen_amd/cycle.py: the three checks,
                 append_edges, scc_labels; one host thread) on the same history,
                 and whether labels, counts and edge sets agree
  kernels        with --profile: ms per step of every k_ap_* kernel and of the
                 rest, from a kernel trace of a fresh child process (a run of
                 its own: tracing slows the call), and the prefix compare's
                 achieved bytes/s

    python tools/bench_cycle_append.py [--txns 200000] [--procs 10 100] [--keys 100] [--anomalies 0 16]
                                       [--max-len 64 1024] [--steps 5] [--warmup 1] [--no-cpu] [--profile DIR]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_c2 import DevCols, timed   # noqa: E402


def short_name(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].strip()
    return name if name.startswith("k_") else name.split("<")[0]


def kernel_times(out_dir, steps):
    """{kernel: ms per step} from the kernel statistics (or, without them, the
    kernel trace) a traced child left in out_dir."""
    out = {}
    stats = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    for path in stats:
        for rec in csv.DictReader(open(path)):
            name = short_name(rec.get("Name", ""))
            out[name] = out.get(name, 0.0) + float(rec.get("TotalDurationNs", 0)) / 1e6 / steps
    if not stats:
        for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
            for rec in csv.DictReader(open(path)):
                name = short_name(rec.get("Kernel_Name", ""))
                out[name] = out.get(name, 0.0) + (int(rec["End_Timestamp"]) - int(rec["Start_Timestamp"])) / 1e6 / steps
    return out


def profile(args, procs, anomalies, max_len, out_dir):
    """One configuration in a fresh child under the kernel trace (steps calls, no warm-up outside them)."""
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__),
           "--txns", str(args.txns), "--procs", str(procs), "--keys", str(args.keys), "--anomalies", str(anomalies),
           "--max-len", str(max_len), "--steps", str(args.steps), "--warmup", "0", "--no-cpu", "--child"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        return {"error": r.stdout[-400:]}
    out = kernel_times(out_dir, args.steps)
    return out if out else {"error": "no kernel statistics under " + out_dir + ": " + " ".join(sorted(os.listdir(out_dir)))[:300]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txns", type=int, default=200000, help="txns (two rows each)")
    ap.add_argument("--procs", type=int, nargs="*", default=[10, 100])
    ap.add_argument("--keys", type=int, default=100)
    ap.add_argument("--anomalies", type=int, nargs="*", default=[0, 16])
    ap.add_argument("--max-len", type=int, nargs="*", default=[64, 1024])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--profile", metavar="DIR", help="also trace each configuration's kernels in a child process, output under DIR")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    import numpy as np
    import torch
    from jepsen_amd import _abi as A
    from jepsen_amd import _native, synth
    from jepsen_amd import cycle as CY
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    for max_len in args.max_len:
        for procs in args.procs:
            for anomalies in args.anomalies:
                t0 = time.perf_counter()
                cols = synth.append_history(args.txns, procs, args.keys, anomalies, 0.02, seed=11, max_len=max_len)
                gen_s = time.perf_counter() - t0
                d = DevCols(cols, dev)
                r, sec = timed(lambda: ctx.check_cycle(d, A.CY_APPEND, on_device=True), args.steps, args.warmup)
                if args.child:
                    continue
                rr, sec_rt = timed(lambda: ctx.check_cycle(d, A.CY_APPEND | A.CY_REALTIME, on_device=True), args.steps, args.warmup)
                edges = sum(r["edge_count"])
                nbytes = 8 * int(r["entries"]) + 8 * 3 * int((np.asarray(cols.value2)).sum())    # elements + 4-word micro-ops
                cpu = None
                if not args.no_cpu:
                    e = ctx.check_cycle(d, A.CY_APPEND, on_device=True, edge_cap=edges, scc_cap=0)["edges"]
                    t0 = time.perf_counter()
                    m = CY._Mops(cols)
                    checks = (CY.duplicate_append(m), CY.duplicate_read(m), CY.bad_order_keys(m))
                    he = CY.append_edges(m)
                    labels = CY.scc_labels(cols.n, he)
                    ct = time.perf_counter() - t0
                    cpu = {"value": cols.n / ct, "unit": "rows/s", "seconds": ct, "speedup": ct / sec,
                           "kind": "jepsen_amd/cycle.py host path (the three checks, append_edges, scc_labels), one thread",
                           "parity": bool(checks == (None, None, {}) and labels.tolist() == r["labels"].tolist()
                                          and len(he) == edges and set(map(tuple, he.tolist())) == set(map(tuple, e.tolist())))}
                kernels = None
                if args.profile:
                    kernels = profile(args, procs, anomalies, max_len,
                                      os.path.join(args.profile, f"len{max_len}_p{procs}_a{anomalies}"))
                    cmp_ms = kernels.get("k_ap_compare")
                    if isinstance(cmp_ms, float) and cmp_ms > 0:
                        kernels["compare_bytes_per_s"] = nbytes / (cmp_ms / 1e3)
                print(json.dumps({
                    "metric": f"history rows checked/sec, list-append cycle checker (appends-and-reads-graph, {procs} processes, "
                              f"reads up to {max_len}, {'stale reads' if anomalies else 'valid'})",
                    "value": cols.n / sec, "unit": "rows/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
                    "ms_per_step": sec * 1e3, "higher_is_better": True, "dtype": "int64", "edges_per_s": edges / sec,
                    "data": f"synthetic (jepsen_amd/synth.py append_history, {args.txns} txns, {procs} processes, {args.keys} live keys, "
                            f"{anomalies} stale reads, p_info 0.02, seed 11, max_len {max_len})",
                    "config": {"rows": int(cols.n), "keys": int(cols.n_keys), "aux_words": int(len(cols.aux)), "entries": r["entries"],
                               "edges": edges, "edge_count": r["edge_count"], "valid": r["valid"], "cause": r["cause"],
                               "scc_count": r["scc_count"], "scc_vertices": r["scc_vertices"], "path": r["path"],
                               "device_ms": r["device_ms"], "gen_s": round(gen_s, 1)},
                    "regions": {"regions": r["regions"], "max_region": r["max_region"], "global_regions": r["global_regions"],
                                "back_edges": r["back_edges"]},
                    "stages": {"append_alone_ms": sec * 1e3, "append_realtime_ms": sec_rt * 1e3,
                               "append_realtime_edges": sum(rr["edge_count"]), "append_realtime_scc_count": rr["scc_count"]},
                    "bytes": {"elements_and_micro_ops": nbytes, "per_s_of_the_whole_call": nbytes / sec},
                    "kernels": kernels, "cpu_baseline": cpu}), flush=True)
                del d
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
