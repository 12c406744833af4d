"""Bank checker measurement (jepsen/src/jepsen/tests/bank.clj:46-121) on one
MI355X: a valid bank history of 100 M rows (jepsen_amd/synth.py bank_history,
8 processes, nemesis noise on) in two configurations with the same number of
(account, balance) pairs -- 8 accounts per read (half the ops are reads), and
1 024 accounts per read (one op in 256 is a read).

One JSON line per configuration. The history is resident in HBM before the
timed region; a step is one jh_check_bank call without the per-read triples
(reads_cap 0, what the checker mirror asks for). `roofline`: algorithmic bytes
over the call's time against 8 TB/s, by the model of DESIGN.md §4f:
  32 B per row (type, f, value, value2), 16 B per pair, and the 20-byte
  per-read record written once and read once
`cpu_baseline`: the numpy restatement tests/bank_ref.py ref_cols (cumulative
sums and fancy indexing, single-threaded: one host thread) on the same history.

    python tools/bench_bank.py [--rows 100000000] [--steps 5] [--warmup 1] [--no-cpu]
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

TOTAL = 100


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
    n_ops = args.rows // 2
    for accounts, p_read in ((8, 0.5), (1024, 0.5 * 8 / 1024)):
        t0 = time.perf_counter()
        cols = synth.bank_history(n_ops, n_accounts=accounts, n_procs=8, total=TOTAL, p_read=p_read, seed=11)
        gen_s = time.perf_counter() - t0
        print(f"# generated {cols.n} rows, {len(cols.aux) // 2} pairs in {gen_s:.1f} s", file=sys.stderr, flush=True)
        d = DevCols(cols, dev)
        r, sec = timed(lambda: ctx.check_bank(d, accounts, TOTAL, reads_cap=0, on_device=True), args.steps, args.warmup)
        n, reads, pairs = int(cols.n), int(r["read_count"]), int(r["entries"])
        alg = 32.0 * n + 16.0 * pairs + 2 * 20.0 * reads
        del d
        torch.cuda.empty_cache()
        cpu, parity = None, None
        if not args.no_cpu:
            from bank_ref import ref_cols
            t0 = time.perf_counter()
            want = ref_cols(cols, accounts, TOTAL, exact=True)
            ct = time.perf_counter() - t0
            parity = (want["valid?"], want["read-count"], want["error-count"]) == \
                (r["valid"] == 0, reads, int(r["error_count"]))
            cpu = {"value": n / ct, "unit": "entries/s", "kind": "numpy restatement (tests/bank_ref.py ref_cols)",
                   "sample": f"the whole history ({n} entries, {ct:.2f} s)"}
        print(json.dumps({
            "metric": f"history entries verified/sec, bank checker ({accounts} accounts per read)", "value": n / sec,
            "unit": "entries/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": sec * 1e3, "higher_is_better": True, "dtype": "int64",
            "data": f"synthetic (jepsen_amd/synth.py bank_history, {accounts} accounts, p_read {p_read:g}, seed 11)",
            "config": {"entries": n, "reads": reads, "pairs": pairs, "valid": r["valid"],
                       "error_count": int(r["error_count"]), "device_ms": r["device_ms"], "gen_s": round(gen_s, 1)},
            "roofline": {"bound": "hbm", "kernel": "whole jh_check_bank call",
                         "achieved": alg / sec / 1e9, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                         "frac": alg / sec / 1e9 / PEAK_HBM_GBS, "algorithmic_bytes": alg},
            "cpu_baseline": cpu, "parity_vs_restatement": parity}), flush=True)
        del cols


if __name__ == "__main__":
    main()
