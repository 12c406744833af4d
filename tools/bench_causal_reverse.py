"""Causal-reverse checker measurement (jepsen/src/jepsen/tests/causal_reverse.clj:21-84
under independent/checker) on one MI355X: 20 000 keys of 500 ops (1 000 rows)
each (jepsen_amd/synth.py causal_reverse_history: a block of `--block` keys,
repeated with key ids and element ranges of its own), a valid history and one
with violating reads, on the on-chip and on the global tier.

One JSON line per configuration. The history is resident in HBM before the
timed region; a step is one jh_check_causal_reverse call asking for what the
checker mirror asks for (1 024 error rows, 65 536 missing values).
  value            history rows per second of the whole call
  elements_per_s   read elements (`entries`) per second of the whole call
  stream           8 B x entries over the call's device time (the events around
                   the call's kernels, `device_ms`) against the copy bandwidth
                   measured in the same process: a device-to-device copy of
                   1 GiB (read + write bytes over event time, after a warm-up).
                   Over the time of k_cr_key alone: run the tool under a kernel
                   trace and give it the trace (`--kernel-times`, below).
  roofline         algorithmic bytes over the call's time against 8 TB/s, by the
                   model of DESIGN.md §4h: 16 B per row (type, f) + 16 B per
                   flagged row (key, value / value2) + 12 B per write and 28 B
                   per read of records, written once and read back once (24 B
                   and 56 B) + 8 B per read element
  cpu_baseline     the numpy restatement tests/causal_reverse_ref.py ref_cols
                   (one host thread) on the first block of keys
`--scale` adds jh_check_set and jh_check_long_fork (n = 2, dense) lines on
histories of the same number of rows, for scale.

`--kernel-times DB LINES`: no GPU work; from the rocprofv3 database DB of a traced
run of this tool (`rocprofv3 --kernel-trace -d DIR -o NAME -- python
tools/bench_causal_reverse.py --no-cpu > LINES`) and that run's JSON lines, one
line per configuration with the mean time of k_cr_key (the judging pass) over
the timed calls and 8 B x entries over it, against the copy bandwidth of LINES.

    python tools/bench_causal_reverse.py [--keys 20000] [--ops 500] [--block 200] [--steps 5] [--warmup 1]
                                         [--violations 0 8] [--path 1 2] [--no-cpu] [--scale]
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


def copy_bandwidth(dev, gib=1, reps=10):
    """GB/s of a device-to-device copy (bytes read + bytes written over event time)."""
    import torch
    a = torch.empty(gib << 27, dtype=torch.int64, device=dev).fill_(1)
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * a.numel() * 8 * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9


def kernel_times(db_path, lines_path):
    """8 B x entries over k_cr_key's own time, from a kernel trace of this tool."""
    import sqlite3
    rows = sqlite3.connect(db_path).execute("select name, start, end from kernels order by start").fetchall()
    calls = []                                   # per jh_check_causal_reverse call: ns in the judging k_cr_key
    for name, t0, t1 in rows:
        if "k_cr_meta_init" in name:
            calls.append(0)
        elif calls and "k_cr_key<" in name and ", false>" in name:
            calls[-1] += t1 - t0
    at = 0
    for line in open(lines_path):
        j = json.loads(line)
        if "stream" not in j:
            continue
        per = j["warmup"] + j["steps"]
        timed_calls = calls[at + j["warmup"]:at + per]
        at += per
        if len(timed_calls) != j["steps"]:
            raise SystemExit(f"the trace holds {len(calls)} calls: not the run that wrote {lines_path}")
        sec = sum(timed_calls) / len(timed_calls) * 1e-9
        gbs = j["stream"]["bytes"] / sec / 1e9
        print(json.dumps({"metric": j["metric"] + ": 8 B x entries over k_cr_key time", "k_cr_key_us": sec * 1e6,
                          "bytes": j["stream"]["bytes"], "achieved": gbs, "unit": "GB/s",
                          "copy_bandwidth": j["stream"]["copy_bandwidth"],
                          "frac_of_copy": gbs / j["stream"]["copy_bandwidth"]}), flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--kernel-times":
        return kernel_times(sys.argv[2], sys.argv[3])
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=20000)
    ap.add_argument("--ops", type=int, default=500, help="ops (invocations) per key")
    ap.add_argument("--block", type=int, default=200, help="keys generated before the history is repeated")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--violations", type=int, nargs="*", default=[0, 8], help="violating reads per block")
    ap.add_argument("--path", type=int, nargs="*", default=[1, 2], help="1 on-chip, 2 global")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--scale", action="store_true", help="also jh_check_set and jh_check_long_fork at the same row count")
    args = ap.parse_args()
    import numpy as np
    import torch
    from jepsen_amd import _abi as A
    from jepsen_amd import _native, synth
    from jepsen_amd import causal_reverse as CR
    dev = torch.device("cuda", 0)
    ctx = _native.Context(0)
    copy_gbs = copy_bandwidth(dev)
    print(f"# device-to-device copy: {copy_gbs:.0f} GB/s", file=sys.stderr, flush=True)
    block = min(args.block, args.keys)
    tile = max(args.keys // block, 1)
    rows = 0
    for viol in args.violations:
        t0 = time.perf_counter()
        cols = synth.causal_reverse_history(n_keys=block, ops_per_key=args.ops, n_procs=5, violations=viol, seed=11, tile=tile)
        gen_s = time.perf_counter() - t0
        print(f"# generated {cols.n} rows, {len(cols.aux)} elements in {gen_s:.1f} s", file=sys.stderr, flush=True)
        d = DevCols(cols, dev)
        cpu, want = None, None
        if not args.no_cpu:
            from causal_reverse_ref import ref_cols
            one = synth.causal_reverse_history(n_keys=block, ops_per_key=args.ops, n_procs=5, violations=viol, seed=11)
            t0 = time.perf_counter()
            want = ref_cols(one)
            ct = time.perf_counter() - t0
            cpu = {"value": one.n / ct, "unit": "entries/s", "kind": "numpy restatement (tests/causal_reverse_ref.py ref_cols)",
                   "sample": f"the first block ({block} keys, {one.n} entries, {ct:.2f} s)"}
        rows = int(cols.n)
        writes = int(((np.asarray(cols.f) == A.F_WRITE) & (np.asarray(cols.type) <= A.TYPE_OK)).sum())
        for path, pname in ((A.CR_PATH_LDS, "on-chip"), (A.CR_PATH_GLOBAL, "global")):
            if path not in args.path:
                continue
            r, sec = timed(lambda: ctx.check_causal_reverse(d, path, CR.ERR_CAP, CR.MISSING_CAP, on_device=True),
                           args.steps, args.warmup)
            reads, entries = int(r["read_count"]), int(r["entries"])
            alg = 16.0 * rows + 16.0 * (reads + writes) + 24.0 * writes + 56.0 * reads + 8.0 * entries
            parity = None if want is None else \
                all(int(r[k]) == int(want[k]) * tile for k in ("read_count", "error_count", "invalid_keys", "missing_total", "entries"))
            print(json.dumps({
                "metric": f"history entries verified/sec, causal-reverse checker ({pname} tier, "
                          f"{'violating reads' if viol else 'valid'})",
                "value": rows / sec, "unit": "entries/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": sec * 1e3, "higher_is_better": True, "dtype": "int64",
                "elements_per_s": entries / sec,
                "data": f"synthetic (jepsen_amd/synth.py causal_reverse_history, {args.ops} ops per key, 5 processes, block "
                        f"{block} keys x {tile}, {viol} violating reads per block, seed 11)",
                "config": {"entries": rows, "keys": int(cols.n_keys), "reads": reads, "writes": writes, "elements": entries,
                           "valid": r["valid"], "error_count": int(r["error_count"]), "missing_total": int(r["missing_total"]),
                           "path": r["path"], "device_ms": r["device_ms"], "gen_s": round(gen_s, 1)},
                "stream": {"bytes": 8.0 * entries, "device_ms": r["device_ms"],
                           "achieved": 8.0 * entries / (r["device_ms"] * 1e-3) / 1e9, "copy_bandwidth": copy_gbs,
                           "unit": "GB/s", "frac_of_copy": 8.0 * entries / (r["device_ms"] * 1e-3) / 1e9 / copy_gbs},
                "roofline": {"bound": "hbm", "kernel": "whole jh_check_causal_reverse call", "achieved": alg / sec / 1e9,
                             "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": alg / sec / 1e9 / PEAK_HBM_GBS,
                             "algorithmic_bytes": alg},
                "cpu_baseline": cpu, "parity_vs_restatement": parity}), flush=True)
        del d
        torch.cuda.empty_cache()
        del cols
    if args.scale and rows:
        cols = synth.set_history(n_adds=rows // 2, n_procs=10, p_fail=0.05, p_info=0.02, n_lost=100, n_unexpected=10, seed=2)
        d = DevCols(cols, dev)
        r, sec = timed(lambda: ctx.check_set(d, runs_cap=1 << 22, on_device=True), args.steps, args.warmup)
        print(json.dumps({"metric": "for scale: jh_check_set (runs output)", "entries": int(cols.n), "ms_per_step": sec * 1e3,
                          "value": cols.n / sec, "unit": "entries/s"}), flush=True)
        del d, cols
        torch.cuda.empty_cache()
        blk = min(1_000_000, max(rows // 2, 1))
        cols = synth.long_fork_history(blk, n=2, n_procs=16, forks=0, seed=11, tile=max(rows // (2 * blk), 1))
        d = DevCols(cols, dev)
        r, sec = timed(lambda: ctx.check_long_fork(d, 2, A.LF_PATH_DENSE, 1024, on_device=True), args.steps, args.warmup)
        print(json.dumps({"metric": "for scale: jh_check_long_fork (n = 2, dense)", "entries": int(cols.n),
                          "ms_per_step": sec * 1e3, "value": cols.n / sec, "unit": "entries/s"}), flush=True)


if __name__ == "__main__":
    main()
