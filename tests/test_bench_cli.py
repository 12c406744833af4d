"""bench.py's command line: a plain run times its steps and prints the line
with nothing else measured; --full adds the host-buffer rate and the parity
check; --dump-outputs writes the last timed step's verdicts, the same from
run to run and equal to the oracle's on the same seeded history."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import ROOT

KEYS = 64


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--keys", str(KEYS), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_dump_outputs_files(built, tmp_path):
    import bench
    from jepsen_amd import _abi as A
    v = np.zeros(3, A.VERDICT_DTYPE)
    v["valid"] = [A.VALID, A.INVALID, A.VALID]
    v["fail_entry"] = [-1, 1 << 40, -1]
    v["explored"] = [A.EXPLORED_UNCOUNTED, 12, 7]
    s = types.SimpleNamespace(valid=A.INVALID, n_invalid=1, n_unknown=0, first_fail_entry=1 << 40, n_keys=3)
    bench.dump_outputs(str(tmp_path / "d"), 0, s, A.VERDICT_FIELDS, v)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(["summary.npy"] + [f"verdict_{f}.npy" for f in A.VERDICT_FIELDS])
    for f in A.VERDICT_FIELDS:
        a = np.load(tmp_path / "d" / f"verdict_{f}.npy")
        assert a.dtype == np.float64 and (a.astype(np.int64) == v[f]).all()
    assert np.load(tmp_path / "d" / "summary.npy").tolist() == [A.INVALID, 1, 0, float(1 << 40), 3]


@pytest.mark.gpu
def test_plain_run_and_dump(built, tmp_path):
    import bench
    from jepsen_amd import _abi as A
    from jepsen_amd import synth
    from oracle import oracle
    line = _bench("--dump-outputs", str(tmp_path / "a"))
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "entries/s" and line["higher_is_better"] is True and line["dtype"] == "int64"
    ent = line["config"]["entries_per_gpu"]
    assert line["value"] == pytest.approx(ent / (line["ms_per_step"] / 1e3), rel=1e-9)
    # nothing but the timed steps was measured
    for f in ("e2e_host_buffers", "cpu_baseline", "cpu_baseline_faithful", "parity_vs_oracle"):
        assert line[f] is None, f
    # the same inputs and outputs from run to run
    _bench("--dump-outputs", str(tmp_path / "b"))
    wl = bench.WORKLOADS["c3"]
    cols, _ = synth.cas_register(n_keys=KEYS, ops_per_key=500, seed=wl["seed"], **wl["gen"])
    assert int(cols.n) == ent
    ov, _ = oracle.check_cas_independent(cols, budget=wl["budget"], threads=8)
    for f in A.VERDICT_FIELDS:
        a = np.load(tmp_path / "a" / f"verdict_{f}.npy")
        assert a.dtype == np.float64 and a.shape == (KEYS,)
        assert (a == np.load(tmp_path / "b" / f"verdict_{f}.npy")).all(), f
        if f == "explored":
            unc = a == A.EXPLORED_UNCOUNTED
            assert (a[~unc] == ov[f][~unc]).all() and (ov["valid"][unc] == A.VALID).all()
        else:
            assert (a == ov[f]).all(), f
    summ = np.load(tmp_path / "a" / "summary.npy")
    assert summ.dtype == np.float64
    assert summ[1] == (ov["valid"] == A.INVALID).sum() and summ[4] == KEYS


@pytest.mark.gpu
def test_full_run(built):
    line = _bench("--full", "--no-cpu")
    assert line["parity_vs_oracle"] is True
    assert line["e2e_host_buffers"]["calls"] == 2 and line["e2e_host_buffers"]["ms_per_call"] > 0
    assert line["cpu_baseline"] is None
