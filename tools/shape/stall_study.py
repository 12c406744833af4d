"""How many C3 keys ever stall, and when (round 7, the late helpers' pick by
stall): every key's canonical WGL DFS (the device's order) with the stall --
the inserts since its deepest layer last rose -- tracked at every insert; per
threshold, the keys that ever reach it, split by verdict, and among the keys
above 8 000 inserts. CPU only.
    python tools/shape/stall_study.py [rank] [key ...]"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from bench import WORKLOADS  # noqa: E402
from jepsen_amd import _abi as A, synth  # noqa: E402

so = os.path.join(HERE, "libwgl_stall.so")
subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-std=gnu11", "-o", so, os.path.join(HERE, "wgl_stall.c"), "-lpthread"])
L = C.CDLL(so)
rank = int(sys.argv[1]) if len(sys.argv) > 1 else 0
show = [int(x) for x in sys.argv[2:]] or [1086]
THR = np.array([1024, 2048, 4096, 8192], np.int64)
wl = WORKLOADS["c3"]
cols, _ = synth.cas_register(n_keys=wl["keys"], ops_per_key=500, seed=wl["seed"] + 7919 * rank, **wl["gen"])
h = A.make_history(cols)
p64 = C.POINTER(C.c_int64)
order = np.argsort(cols.key, kind="stable")
bounds = np.searchsorted(cols.key[order], np.arange(cols.n_keys + 1))
unk = np.nonzero(cols.key < 0)[0]
tot = np.zeros(cols.n_keys, np.int64)
verdict = np.zeros(cols.n_keys, np.int64)
first = np.full((cols.n_keys, len(THR)), -1, np.int64)
for k in range(cols.n_keys):
    sel = np.sort(np.concatenate([order[bounds[k]:bounds[k + 1]], unk])).astype(np.int64)
    out = np.zeros(4, np.int64)
    L.wgl_stall(C.byref(h), sel.ctypes.data_as(p64), C.c_int64(len(sel)), C.c_int64(A.NIL), C.c_int64(wl["budget"]),
                THR.ctypes.data_as(p64), C.c_int(len(THR)), first[k].ctypes.data_as(p64), out.ctypes.data_as(p64))
    tot[k], verdict[k] = out[0], out[1]
invalid = verdict == A.INVALID
big = tot > 8000
res = {"rank": rank, "keys": int(cols.n_keys), "inserts": int(tot.sum()), "invalid_keys": int(invalid.sum()),
       "keys_above_8000_inserts": int(big.sum()), "thresholds": {}}
for i, th in enumerate(THR.tolist()):
    hit = first[:, i] >= 0
    res["thresholds"][th] = {"keys": int(hit.sum()), "invalid": int((hit & invalid).sum()),
                             "valid": int((hit & ~invalid).sum()), "of_keys_above_8000": int((hit & big).sum())}
res["shown"] = {k: {"inserts": int(tot[k]), "verdict": int(verdict[k]),
                    "first_insert_at_stall": dict(zip(THR.tolist(), first[k].tolist()))} for k in show}
print(json.dumps(res, indent=1))
