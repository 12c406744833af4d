"""Adya G2 checker measurement (jepsen/src/jepsen/tests/adya.clj:62-88) on one
MI355X: `--keys` keys of two inserts, four rows each (jepsen_amd/synth.py
g2_history), a valid history and one with `--illegal` keys inserted twice.

One JSON line per configuration. The history is resident in HBM before the
timed region; a step is one jh_check_g2 call asking for what the checker mirror
asks for (1 024 illegal pairs).
  value          history rows per second of the whole call
  device         the events around the call's kernels (`device_ms`), the
                 algorithmic bytes over it and that against the copy bandwidth
                 measured in the same process (a device-to-device copy of 1 GiB,
                 read + write bytes over event time, after a warm-up)
  algorithmic bytes, counted from the shapes: 24 B per row (type, f, key) plus
                 8 B per insert row of atomic traffic
  cpu_baseline   adya.check_host, one host thread, on a history of `--cpu-keys`
                 keys of the same generator, its map compared with the device's
Per-kernel times: run the tool under `rocprofv3 --kernel-trace --stats`.

    python tools/bench_g2.py [--keys 2500000] [--illegal 0 1000] [--steps 5] [--warmup 1] [--cpu-keys 100000] [--no-cpu]
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
from bench_causal_reverse import copy_bandwidth   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=2_500_000)
    ap.add_argument("--illegal", type=int, nargs="*", default=[0, 1000], help="keys inserted twice")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-keys", type=int, default=100_000)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    from jepsen_amd import _native, adya, synth
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    copy_gbs = copy_bandwidth(dev)
    print(f"# device-to-device copy: {copy_gbs:.0f} GB/s", file=sys.stderr, flush=True)
    for ill in args.illegal:
        t0 = time.perf_counter()
        cols = synth.g2_history(n_keys=args.keys, illegal=ill, seed=11)
        gen_s = time.perf_counter() - t0
        print(f"# generated {cols.n} rows in {gen_s:.1f} s", file=sys.stderr, flush=True)
        cpu = None
        if not args.no_cpu:
            ck = min(args.cpu_keys, args.keys)
            small = synth.g2_history(n_keys=ck, illegal=min(ill, ck // 10), seed=11)
            ops = synth.g2_columns_to_ops(small)
            t0 = time.perf_counter()
            host = adya.check_host(ops)
            ct = time.perf_counter() - t0
            same = adya.result_map(adya.device_result(ctx, small), small.keys) == host
            cpu = {"value": small.n / ct, "unit": "entries/s", "kind": "adya.check_host, one thread",
                   "sample": f"{ck} keys, {small.n} entries, {ct:.2f} s", "map_equals_device": same}
        d = DevCols(cols, dev)
        rows, K = int(cols.n), int(cols.n_keys)
        r, sec = timed(lambda: ctx.check_g2(d, adya.ILLEGAL_CAP, on_device=True), args.steps, args.warmup)
        alg = 24.0 * rows + 8.0 * int(r["insert_rows"])
        dev_gbs = alg / (r["device_ms"] * 1e-3) / 1e9
        print(json.dumps({
            "metric": f"history entries verified/sec, adya g2 checker ({'illegal keys' if ill else 'valid'})",
            "value": rows / sec, "unit": "entries/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": sec * 1e3, "higher_is_better": True, "dtype": "int64",
            "data": f"synthetic (jepsen_amd/synth.py g2_history, {K} keys of two inserts, {ill} illegal keys, seed 11)",
            "config": {"entries": rows, "keys": K, "insert_rows": int(r["insert_rows"]), "valid": r["valid"],
                       "key_count": int(r["key_count"]), "legal_count": int(r["legal_count"]),
                       "illegal_count": int(r["illegal_count"]), "first_illegal_row": int(r["first_illegal_row"]),
                       "gen_s": round(gen_s, 1)},
            "device": {"device_ms": r["device_ms"], "rows_per_s": rows / (r["device_ms"] * 1e-3), "algorithmic_bytes": alg,
                       "achieved": dev_gbs, "unit": "GB/s", "copy_bandwidth": copy_gbs, "frac_of_copy": dev_gbs / copy_gbs},
            "cpu_baseline": cpu, "speedup_vs_cpu": None if cpu is None else rows / sec / cpu["value"]}), flush=True)
        del d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
