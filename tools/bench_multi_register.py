"""Multi-register linearizability measurement ((independent/checker
(checker/linearizable {:model (multi-register {})})), yugabyte
multi_key_acid.clj:112-127) on one MI355X: the C3 shape of SURVEY.md 8(d) as a
txn workload -- 10 000 keys of about 1 000 entries each, 10 threads per key, 3
registers, 5 values, 2 % crashed ops, 1 % of the keys faulted, a fixed seed
(jepsen_amd/synth.py multi_register_history).

Generating and encoding ten million op maps in Python takes minutes, so the
tool simulates `--distinct` keys (100) and tiles their encoded columns up to
`--keys`: every key is searched on its own, but only `--distinct` different
searches exist. `--distinct` equal to `--keys` is the untiled measurement.

One JSON line: entries, keys, entries_per_s over the whole call (host columns
in, verdicts out) and over its device time, the counts of valid / invalid /
:unknown keys at the budget (the :unknown count is part of the result: a key
past the budget is not checked), explored (the sum of the cache sizes), the
largest cache and the search waves.

    python tools/bench_multi_register.py [--keys 10000] [--ops 500] [--distinct 100] [--steps 3] [--warmup 1] [--budget 0]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tiled(cols, times):
    """The columns `times` times over, each copy with keys and triples of its own."""
    import numpy as np
    from jepsen_amd.history import Columns
    n, K, na = cols.n, cols.n_keys, len(cols.aux) // 3
    rep = lambda a: np.tile(a, times)
    shift = np.repeat(np.arange(times, dtype=np.int64), n)
    key = rep(cols.key) + np.where(rep(cols.key) >= 0, shift * K, 0)
    value = rep(cols.value)
    value = np.where(value >= 0, value + shift * na, value)
    return Columns(n=n * times, process=rep(cols.process), type=rep(cols.type), f=rep(cols.f), key=key, value=value,
                   value2=rep(cols.value2), n_keys=K * times, aux=np.tile(cols.aux, times),
                   keys=[(c, k) for c in range(times) for k in cols.keys], f_names=cols.f_names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=10000)
    ap.add_argument("--ops", type=int, default=500, help="ops per key (2 entries each)")
    ap.add_argument("--distinct", type=int, default=100, help="keys simulated; tiled up to --keys")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--budget", type=int, default=0, help="0: the default, 2^20")
    args = ap.parse_args()

    from jepsen_amd import _abi as A
    from jepsen_amd import _native, multi_register, synth
    from jepsen_amd.model import multi_register as model

    distinct = min(args.distinct, args.keys)
    times = max(1, args.keys // distinct)
    h = synth.multi_register_history(n_keys=distinct, ops_per_key=args.ops, threads=10, regs=3, values=5, p_info=0.02,
                                     faulted_keys=max(1, distinct // 100), seed=20260)
    cols, meta = multi_register.encode(h, model({}), keyed=True)
    if times > 1:
        cols = tiled(cols, times)
    ctx = _native.default_context(0)
    call = lambda: ctx.check_multi_register(cols, meta["n_regs"], meta["bits"], meta["init"], args.budget)
    for _ in range(args.warmup):
        call()
    host_ms, dev_ms = [], []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        v, s = call()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(s.device_ms)
    host, dev = sorted(host_ms)[len(host_ms) // 2], sorted(dev_ms)[len(dev_ms) // 2]
    print(json.dumps({
        "bench": "multi_register", "keys": int(cols.n_keys), "distinct_keys": distinct, "entries": int(cols.n),
        "host_ms": round(host, 3), "device_ms": round(dev, 3),
        "entries_per_s": round(cols.n / (host / 1e3)), "entries_per_s_device": round(cols.n / (dev / 1e3)),
        "valid": int((v["valid"] == A.VALID).sum()), "invalid": int((v["valid"] == A.INVALID).sum()),
        "unknown": int((v["valid"] == A.UNKNOWN).sum()), "budget": args.budget or A.DEFAULT_BUDGET,
        "explored": int(s.explored), "max_explored": int(v["explored"].max()), "waves": int(s.waves[0]),
        "steps": args.steps, "warmup": args.warmup}))


if __name__ == "__main__":
    main()
