"""Causal checker measurement (jepsen/src/jepsen/tests/causal.clj:33-110 under
independent/checker) on one MI355X: `--keys` keys of five ops, ten rows each
(jepsen_amd/synth.py causal_history), a valid history and one with `--violations`
faulty keys.

One JSON line per configuration. The history is resident in HBM before the
timed region; a step is one jh_check_causal call with every key's record copied
back, as the lifted checker asks for it.
  value          history rows per second of the whole call
  device         the events around the call's kernels (`device_ms`), the
                 algorithmic bytes over it and that against the copy bandwidth
                 measured in the same process (a device-to-device copy of 1 GiB,
                 read + write bytes over event time, after a warm-up)
  algorithmic bytes, counted from the shapes: 16 B per row for the flag pass
                 (type, key), plus per :ok row the 8 B sort pair and 32 B of
                 gathers (f, value, position, link)
  cpu_baseline   causal.check_host over independent.subhistories, one host
                 thread, on a history of `--cpu-keys` keys of the same generator
                 (op maps of the whole history do not fit a run's time), its
                 verdicts compared with the device's on that history
Per-kernel times: run the tool under `rocprofv3 --kernel-trace --stats`.

    python tools/bench_causal.py [--keys 1000000] [--violations 0 1000] [--steps 5] [--warmup 1]
                                 [--cpu-keys 50000] [--no-cpu]
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
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--violations", type=int, nargs="*", default=[0, 1000], help="faulty keys")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-keys", type=int, default=50_000)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    from jepsen_amd import _abi as A
    from jepsen_amd import _native, independent, synth
    from jepsen_amd import causal as CM
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    copy_gbs = copy_bandwidth(dev)
    print(f"# device-to-device copy: {copy_gbs:.0f} GB/s", file=sys.stderr, flush=True)
    for viol in args.violations:
        t0 = time.perf_counter()
        cols = synth.causal_history(n_keys=args.keys, violations=viol, seed=11)
        gen_s = time.perf_counter() - t0
        print(f"# generated {cols.n} rows in {gen_s:.1f} s", file=sys.stderr, flush=True)
        cpu = None
        if not args.no_cpu:
            ck = min(args.cpu_keys, args.keys)
            small = synth.causal_history(n_keys=ck, violations=min(viol, ck // 10), seed=11)
            ops = synth.causal_columns_to_ops(small)
            t0 = time.perf_counter()
            host = {k: CM.check_host(CM.causal_register(), sub) for k, sub in independent.subhistories(ops).items()}
            ct = time.perf_counter() - t0
            got = ctx.check_causal(small)
            same = all((int(got["keys"][k]["valid"]) == A.VALID) == host[k]["valid?"] for k in host)
            cpu = {"value": small.n / ct, "unit": "entries/s", "kind": "causal.check_host per key, one thread",
                   "sample": f"{ck} keys, {small.n} entries, {ct:.2f} s", "verdicts_equal_device": same}
        d = DevCols(cols, dev)
        rows, K = int(cols.n), int(cols.n_keys)
        r, sec = timed(lambda: ctx.check_causal(d, on_device=True), args.steps, args.warmup)
        M = int(r["ok_count"])
        alg = 16.0 * rows + 40.0 * M
        dev_gbs = alg / (r["device_ms"] * 1e-3) / 1e9
        print(json.dumps({
            "metric": f"history entries verified/sec, causal checker ({'faulty keys' if viol else 'valid'})",
            "value": rows / sec, "unit": "entries/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": sec * 1e3, "higher_is_better": True, "dtype": "int64",
            "data": f"synthetic (jepsen_amd/synth.py causal_history, {K} keys of five ops, {viol} faulty keys, seed 11)",
            "config": {"entries": rows, "keys": K, "ok_rows": M, "valid": r["valid"], "invalid_keys": int(r["invalid_keys"]),
                       "unknown_keys": int(r["unknown_keys"]), "first_event_row": int(r["first_event_row"]),
                       "gen_s": round(gen_s, 1)},
            "device": {"device_ms": r["device_ms"], "rows_per_s": rows / (r["device_ms"] * 1e-3), "algorithmic_bytes": alg,
                       "achieved": dev_gbs, "unit": "GB/s", "copy_bandwidth": copy_gbs, "frac_of_copy": dev_gbs / copy_gbs},
            "cpu_baseline": cpu, "speedup_vs_cpu": None if cpu is None else rows / sec / cpu["value"]}), flush=True)
        del d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
