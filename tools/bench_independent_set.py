"""Independent set checker measurement ((independent/checker (checker/set)),
independent.clj:247-298 over checker.clj:182-233) on one MI355X: the C3 shape of
SURVEY.md 8(d) as a set workload -- 10 000 keys of about 1 000 rows each
(jepsen_amd/synth.py independent_set_history: 499 adds per key on 5 threads,
keys in concurrent groups, one final read per key, a :nemesis :info row every
5 000 rows or so, some keys with lost and unexpected elements).

One JSON line:
  batched          one jh_check_set_independent call over every key:
                   device_ms (the events around the call's device work) and
                   host_ms, host to host: the encoded columns in host memory to
                   every key's record and bitmaps in host memory (the bound of
                   the output size, the copies to the device and back included)
  per_key          the path the checker took before (independent.check_per_key:
                   one sub-history, one encode and one jh_check_set_bitmaps
                   call per key) on the op maps of the first `--subset` keys and
                   every un-keyed row, and the same keys through the batched
                   checker (independent.checker(checker.set()), its encode
                   included); `scaled_ms` is the per-key time times keys / subset
  ratio            per_key.scaled_ms over batched.host_ms
  roofline         algorithmic bytes -- 32 B per row (type, f, key, value), 8 B
                   per final-read element, 16 B per 32 elements of span written
                   (the four result words) -- over the call's device time and
                   over its host-to-host time, against 8 TB/s

    python tools/bench_independent_set.py [--keys 10000] [--adds 499] [--subset 100] [--steps 3] [--warmup 1] [--path 0]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_c2 import PEAK_HBM_GBS   # noqa: E402


def subset_ops(cols, n_sub):
    """Op maps of the rows of keys 0 .. n_sub - 1 and of every un-keyed row."""
    import numpy as np
    from jepsen_amd import synth
    from jepsen_amd.history import Columns
    keep = np.nonzero(np.asarray(cols.key) < n_sub)[0]
    sub = Columns(n=len(keep), process=cols.process[keep], type=cols.type[keep], f=cols.f[keep], key=cols.key[keep],
                  value=cols.value[keep], value2=cols.value2[keep], n_keys=n_sub, aux=cols.aux, keys=cols.keys[:n_sub],
                  f_names=cols.f_names)
    return synth.independent_set_columns_to_ops(sub)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=10000)
    ap.add_argument("--adds", type=int, default=499, help="adds per key (2 rows each, plus 2 for the read)")
    ap.add_argument("--subset", type=int, default=100, help="keys the per-key path is timed on")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--path", type=int, default=0, help="0 auto, 1 on-chip, 2 global")
    args = ap.parse_args()
    from jepsen_amd import _native, checker, independent, synth
    t0 = time.perf_counter()
    cols = synth.independent_set_history(n_keys=args.keys, adds_per_key=args.adds, threads_per_key=5, p_fail=0.05, p_info=0.02,
                                         n_lost_keys=args.keys // 100, n_unexpected_keys=args.keys // 100, seed=3,
                                         concurrent=10, nemesis_every=5000)
    gen_s = time.perf_counter() - t0
    print(f"# generated {cols.n} rows, {len(cols.aux)} read elements in {gen_s:.1f} s", file=sys.stderr, flush=True)
    ctx = _native.default_context(0)

    # the batched call, host to host
    r = None
    for _ in range(args.warmup):
        r = ctx.check_set_independent(cols, path=args.path)
    t0 = time.perf_counter()
    dev_ms = 0.0
    for _ in range(args.steps):
        r = ctx.check_set_independent(cols, path=args.path)
        dev_ms += r["device_ms"]
    host_ms = (time.perf_counter() - t0) / args.steps * 1e3
    dev_ms /= args.steps
    alg = 32.0 * cols.n + 8.0 * (int(r["entries"]) - cols.n) + 16.0 * int(r["total_words"])

    # the per-key path and the batched checker on the same keys' op maps
    n_sub = max(1, min(args.subset, args.keys))
    ops = subset_ops(cols, n_sub)
    batched_chk = independent.checker(checker.set())
    for _ in range(args.warmup):
        independent.check_per_key(checker.set(), {}, ops[:2000])
        batched_chk.check({}, ops[:2000], {})
    t0 = time.perf_counter()
    per_key = independent.check_per_key(checker.set(), {}, ops)
    per_key_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    got = batched_chk.check({}, ops, {})
    sub_batched_ms = (time.perf_counter() - t0) * 1e3
    scaled_ms = per_key_ms * args.keys / n_sub
    print(json.dumps({
        "metric": "history entries verified/sec, independent set checker (one batched call, host to host)",
        "value": cols.n / (host_ms * 1e-3), "unit": "entries/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "higher_is_better": True, "dtype": "int64",
        "data": f"synthetic (jepsen_amd/synth.py independent_set_history, {args.keys} keys x {args.adds} adds, 5 threads per key, "
                f"10 keys at a time, {args.keys // 100} keys with lost and as many with unexpected elements, seed 3)",
        "config": {"entries": int(cols.n), "keys": int(cols.n_keys), "read_elements": int(r["entries"]) - int(cols.n),
                   "total_words": int(r["total_words"]), "path": int(r["path"]), "valid": int(r["valid"]),
                   "keys_invalid": int(r["keys_invalid"]), "keys_unknown": int(r["keys_unknown"]), "gen_s": round(gen_s, 1)},
        "batched": {"device_ms": dev_ms, "host_ms": host_ms},
        "per_key": {"subset_keys": n_sub, "subset_rows": len(ops), "ms": per_key_ms, "ms_per_key": per_key_ms / n_sub,
                    "scaled_ms": scaled_ms, "batched_checker_ms_same_keys": sub_batched_ms,
                    "ratio_same_keys": per_key_ms / sub_batched_ms,
                    "parity_with_batched": got["results"] == per_key},
        "ratio": scaled_ms / host_ms,
        "roofline": {"bound": "hbm", "kernel": "whole jh_check_set_independent call", "algorithmic_bytes": alg,
                     "achieved_device": alg / (dev_ms * 1e-3) / 1e9, "achieved_host_to_host": alg / (host_ms * 1e-3) / 1e9,
                     "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac_device": alg / (dev_ms * 1e-3) / 1e9 / PEAK_HBM_GBS}}),
        flush=True)


if __name__ == "__main__":
    main()
