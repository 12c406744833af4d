"""Long-fork checker measurement (jepsen/src/jepsen/tests/long_fork.clj:158-324)
on one MI355X: a long-fork workload of 100 M rows (jepsen_amd/synth.py
long_fork_history: a block of 1 M ops of 16 processes, repeated with disjoint
keys) with groups of n = 2 and n = 10 keys, on the dense and the sparse path,
for a valid history and for one with planted forks (8 per block).

One JSON line per configuration. The history is resident in HBM before the
timed region; a step is one jh_check_long_fork call asking for up to 1 024
fork pairs (what the checker mirror asks for). `roofline`: algorithmic bytes
over the call's time against 8 TB/s, by the model of DESIGN.md §4g:
  16 B per row (type, f) + 16 B per :ok read and :invoke write row (value,
  value2), 16 B per pair twice (the shape pass and pass A), 4 B counter and
  8 B value-table traffic per non-nil pair, and 28 B per read of records
  (row, start, count, group, mask, slot written once and read about once)
`cpu_baseline`: the numpy restatement tests/long_fork_ref.py ref_cols
(single-threaded: one host thread) on the same history.

    python tools/bench_long_fork.py [--rows 100000000] [--steps 5] [--warmup 1] [--no-cpu] [--block 1000000]
                                       [--n 2 10] [--forks 0 8] [--path 1 2]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_c2 import DevCols, timed, PEAK_HBM_GBS   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--block", type=int, default=1_000_000, help="ops generated before the history is repeated")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--n", type=int, nargs="*", default=[2, 10], help="group sizes")
    ap.add_argument("--forks", type=int, nargs="*", default=[0, 8], help="planted forks per block")
    ap.add_argument("--path", type=int, nargs="*", default=[1, 2], help="1 dense, 2 sparse")
    args = ap.parse_args()
    import numpy as np
    import torch
    from jepsen_amd import _abi as A
    from jepsen_amd import _native, synth
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    block = min(args.block, max(args.rows // 2, 1))
    tile = max(args.rows // (2 * block), 1)
    for n in args.n:
        for forks in args.forks:
            t0 = time.perf_counter()
            cols = synth.long_fork_history(block, n=n, n_procs=16, forks=forks, seed=11, tile=tile)
            gen_s = time.perf_counter() - t0
            print(f"# generated {cols.n} rows, {len(cols.aux) // 2} pairs in {gen_s:.1f} s", file=sys.stderr, flush=True)
            d = DevCols(cols, dev)
            nonnil = int((np.asarray(cols.aux)[1::2] != A.NIL).sum())
            cpu, want = None, None
            if not args.no_cpu:
                from long_fork_ref import ref_cols
                t0 = time.perf_counter()
                want = ref_cols(cols, n)
                ct = time.perf_counter() - t0
                cpu = {"value": cols.n / ct, "unit": "entries/s",
                       "kind": "numpy restatement (tests/long_fork_ref.py ref_cols)",
                       "sample": f"the whole history ({cols.n} entries, {ct:.2f} s)"}
            for path, pname in ((A.LF_PATH_DENSE, "dense"), (A.LF_PATH_SPARSE, "sparse")):
                if path not in args.path:
                    continue
                r, sec = timed(lambda: ctx.check_long_fork(d, n, path, 1024, on_device=True), args.steps, args.warmup)
                rows, reads, pairs = int(cols.n), int(r["reads_count"]), int(r["entries"])
                writes = int(((np.asarray(cols.type) == A.TYPE_INVOKE) & (np.asarray(cols.f) == A.F_WRITE)).sum())
                alg = 16.0 * rows + 16.0 * (reads + writes) + 2 * 16.0 * pairs + 12.0 * nonnil + 2 * 28.0 * reads
                parity = None if want is None else \
                    all(int(r[k]) == int(want[k]) for k in ("valid", "reads_count", "early_count", "late_count",
                                                            "fork_groups", "fork_count"))
                print(json.dumps({
                    "metric": f"history entries verified/sec, long-fork checker (n = {n}, {pname} path, "
                              f"{'planted forks' if forks else 'valid'})",
                    "value": rows / sec, "unit": "entries/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
                    "ms_per_step": sec * 1e3, "higher_is_better": True, "dtype": "int64",
                    "data": f"synthetic (jepsen_amd/synth.py long_fork_history, n {n}, 16 processes, block {block} ops "
                            f"x {tile}, {forks} forks per block, seed 11)",
                    "config": {"entries": rows, "reads": reads, "writes": writes, "pairs": pairs, "non_nil_pairs": nonnil,
                               "valid": r["valid"], "fork_count": int(r["fork_count"]), "path": r["path"],
                               "device_ms": r["device_ms"], "gen_s": round(gen_s, 1)},
                    "roofline": {"bound": "hbm", "kernel": "whole jh_check_long_fork call",
                                 "achieved": alg / sec / 1e9, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                 "frac": alg / sec / 1e9 / PEAK_HBM_GBS, "algorithmic_bytes": alg,
                                 "counter_atomic_bytes": 12.0 * nonnil},
                    "cpu_baseline": cpu, "parity_vs_restatement": parity}), flush=True)
            del d
            torch.cuda.empty_cache()
            del cols


if __name__ == "__main__":
    main()
