"""Cycle checker measurement (jepsen/src/jepsen/tests/cycle.clj: wr-graph +
realtime-graph under cycle/checker) on one MI355X: transactional histories of
jepsen_amd/synth.py txn_cycle_history at 10 and at 100 processes, valid and with
injected cycles.

One JSON line per configuration. The history is resident in HBM before the timed
region; a step is one jh_check_cycle call asking for what the checker mirror
asks for (labels, 8 SCCs).
  value          edges per second of the whole call (wr + realtime edges built
                 and searched)
  regions        regions of two or more rows, the largest one's rows, how many
                 ran in the global tier, back edges
  stages         ms per step of calls that stop earlier or do less: realtime
                 alone, wr alone, and jh_scc over the same edge list (regions,
                 CSRs, region kernel, results; its host-to-device copy of the
                 edges included)
  cpu_baseline   this module's host path (jepsen_amd/cycle.py: wr_edges,
                 realtime_edges, scc_labels; one host thread) on the same history,
                 and whether labels and counts agree

    python tools/bench_cycle.py [--ops 200000] [--procs 10 100] [--keys 100] [--anomalies 0 16]
                                [--steps 5] [--warmup 1] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_c2 import DevCols, timed   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=200000, help="txns (two rows each)")
    ap.add_argument("--procs", type=int, nargs="*", default=[10, 100])
    ap.add_argument("--keys", type=int, default=100)
    ap.add_argument("--anomalies", type=int, nargs="*", default=[0, 16])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from jepsen_amd import _abi as A
    from jepsen_amd import _native, synth
    from jepsen_amd import cycle as CY
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    mask = A.CY_WR | A.CY_REALTIME
    for procs in args.procs:
        for anomalies in args.anomalies:
            t0 = time.perf_counter()
            cols = synth.txn_cycle_history(args.ops, procs, args.keys, anomalies, 0.02, seed=11)
            gen_s = time.perf_counter() - t0
            d = DevCols(cols, dev)
            r, sec = timed(lambda: ctx.check_cycle(d, mask, on_device=True), args.steps, args.warmup)
            edges = sum(r["edge_count"])
            _, sec_rt = timed(lambda: ctx.check_cycle(d, A.CY_REALTIME, on_device=True), args.steps, args.warmup)
            _, sec_wr = timed(lambda: ctx.check_cycle(d, A.CY_WR, on_device=True), args.steps, args.warmup)
            e = ctx.check_cycle(d, mask, on_device=True, edge_cap=edges, scc_cap=0)["edges"]
            src, dst = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
            rs, sec_scc = timed(lambda: ctx.scc(cols.n, src, dst), args.steps, args.warmup)
            cpu = None
            if not args.no_cpu:
                ops = synth.txn_cycle_columns_to_ops(cols)
                t0 = time.perf_counter()
                g, _ = CY.combine(CY.wr_graph, CY.realtime_graph)(ops)
                labels = CY.scc_labels(g.n, g.edges)
                ct = time.perf_counter() - t0
                cpu = {"value": len(g.edges) / ct, "unit": "edges/s", "seconds": ct, "speedup": ct / sec,
                       "kind": "jepsen_amd/cycle.py host path (wr_edges, realtime_edges, scc_labels), one thread",
                       "parity": bool(labels.tolist() == r["labels"].tolist() and len(g.edges) == edges
                                      and rs["labels"].tolist() == r["labels"].tolist())}
            print(json.dumps({
                "metric": f"dependency edges built and searched/sec, cycle checker (wr + realtime, {procs} processes, "
                          f"{'injected cycles' if anomalies else 'valid'})",
                "value": edges / sec, "unit": "edges/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": sec * 1e3, "higher_is_better": True, "dtype": "int64", "rows_per_s": cols.n / sec,
                "data": f"synthetic (jepsen_amd/synth.py txn_cycle_history, {args.ops} txns, {procs} processes, {args.keys} keys, "
                        f"{anomalies} injected cycles, p_info 0.02, seed 11)",
                "config": {"rows": int(cols.n), "edges": edges, "edge_count": r["edge_count"], "valid": r["valid"],
                           "scc_count": r["scc_count"], "scc_vertices": r["scc_vertices"], "path": r["path"],
                           "device_ms": r["device_ms"], "gen_s": round(gen_s, 1)},
                "regions": {"regions": r["regions"], "max_region": r["max_region"], "global_regions": r["global_regions"],
                            "back_edges": r["back_edges"]},
                "stages": {"realtime_alone_ms": sec_rt * 1e3, "wr_alone_ms": sec_wr * 1e3, "scc_of_edge_list_ms": sec_scc * 1e3,
                           "scc_device_ms": rs["device_ms"]},
                "cpu_baseline": cpu}), flush=True)
            del d
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
