"""checker/unique-ids measurement (jepsen/src/jepsen/checker.clj:631-676) on one
MI355X: one valid `counter` history (consecutive ids: the dense bitmap path)
and one valid `flake` history (random 63-bit ids: the sorted path), 100 M rows
each (jepsen_amd/synth.py unique_ids_history, 8 processes, noise rows on).

One JSON line per history. The history is resident in HBM before the timed
region; a step is one jh_check_unique_ids call. `roofline`: algorithmic bytes
over the call's time against 8 TB/s, by the model of DESIGN.md §4e:
  scan    24 B per row, + 8 B per ack written to the id list
  dense   + 8 B per ack read, + span / 8 B of bitmap cleared and span / 8 touched
  sorted  + 16 B per ack (keys in place), + ceil(key bits / 8) radix passes of
          16 B per ack, + 9 B per ack (the runs pass and its flags)
`cpu_baseline`: the numpy restatement below (boolean indexing and np.unique
with counts, both single-threaded: one host thread) on the same history.

    python tools/bench_unique_ids.py [--rows 100000000] [--steps 5] [--warmup 1] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_c2 import DevCols, timed, PEAK_HBM_GBS   # noqa: E402

NIL = -(1 << 63)


def numpy_restatement(cols, fgen):
    """attempted, acknowledged, duplicated-count, [lo hi] (no nil acks here)."""
    gen = cols.f == fgen
    attempted = int(np.count_nonzero(gen & (cols.type == 0)))
    acks = cols.value[gen & (cols.type == 1)]
    ids, cnt = np.unique(acks, return_counts=True)
    return attempted, int(len(acks)), int(np.count_nonzero(cnt > 1)), int(ids[0]), int(ids[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    from jepsen_amd import _native, synth
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    n_ops = args.rows * 8 // 18                     # 8 ops and 2 noise rows per round of 18 rows
    for kind, path in (("counter", 1), ("flake", 2)):
        t0 = time.perf_counter()
        cols = synth.unique_ids_history(n_ops, n_procs=8, kind=kind, seed=11)
        gen_s = time.perf_counter() - t0
        fgen = 16 + cols.f_names.index("generate")
        d = DevCols(cols, dev)
        r, sec = timed(lambda: ctx.check_unique_ids(d, fgen, on_device=True), args.steps, args.warmup)
        n, acks = int(cols.n), int(r["acknowledged_count"])
        span = r["range_hi"] - r["range_lo"] + 1
        alg = 24.0 * n + 8.0 * acks
        if r["path"] == 1:
            alg += 8.0 * acks + 2.0 * span / 8
        else:
            bits = max(1, int(span - 1).bit_length())
            alg += 16.0 * acks + 16.0 * acks * ((bits + 7) // 8) + 9.0 * acks
        cpu, parity = None, None
        if not args.no_cpu:
            t0 = time.perf_counter()
            want = numpy_restatement(cols, fgen)
            ct = time.perf_counter() - t0
            parity = want == (r["attempted_count"], acks, r["duplicated_count"], r["range_lo"], r["range_hi"])
            cpu = {"value": n / ct, "unit": "entries/s", "kind": "numpy restatement (np.unique with counts)",
                   "sample": f"the whole history ({n} entries, {ct:.2f} s)"}
        print(json.dumps({
            "metric": f"history entries verified/sec, checker/unique-ids ({kind})", "value": n / sec,
            "unit": "entries/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": sec * 1e3, "higher_is_better": True, "dtype": "int64",
            "data": f"synthetic (jepsen_amd/synth.py unique_ids_history, kind {kind}, seed 11)",
            "config": {"entries": n, "acks": acks, "span": int(span), "path": r["path"], "expected_path": path,
                       "valid": r["valid"], "device_ms": r["device_ms"], "gen_s": round(gen_s, 1)},
            "roofline": {"bound": "hbm", "kernel": "whole jh_check_unique_ids call",
                         "achieved": alg / sec / 1e9, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                         "frac": alg / sec / 1e9 / PEAK_HBM_GBS, "algorithmic_bytes": alg},
            "cpu_baseline": cpu, "parity_vs_restatement": parity}), flush=True)
        del d, cols
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
