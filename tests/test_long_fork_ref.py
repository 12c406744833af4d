"""jepsen.tests.long-fork/checker without a GPU: the mirror's host path
(jepsen_amd/long_fork.py) against hand-written answers (tests/long_fork_cases.py)
and the reference's own test (tests/golden/long_fork.json), the two CPU
restatements (tests/long_fork_ref.py) against each other on synthetic
workloads, the fact the device's chain test rests on, and the ctypes layout of
the new structs."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from jepsen_amd import _abi as A
from jepsen_amd import checker, synth
from jepsen_amd import long_fork as L
from long_fork_cases import CASES, HOST_ONLY, RAISING, R, W, inv, ok
from long_fork_ref import Illegal, raw_of_map, ref_cols, ref_ops, strip

HEADER = os.path.join(ROOT, "include", "jh.h")


@pytest.mark.parametrize("name", list(CASES))
def test_hand_written_answers(name):
    n, h, want = CASES[name]
    assert strip(L.check_host(n, h)) == want
    assert ref_ops(n, h) == want
    cols = L.encode(h)
    raw = ref_cols(cols, n)
    if name in HOST_ONLY:
        assert raw == {"rc": A.JH_EUNSUPPORTED}
        return
    want_raw = raw_of_map(want, h)
    assert {k: raw[k] for k in want_raw if k not in ("forks", "fork_groups")} == \
        {k: v for k, v in want_raw.items() if k not in ("forks", "fork_groups")}
    assert raw["forks"].tolist() == want_raw["forks"]
    # the same answer from the op maps the columns decode to
    assert strip(L.check_host(n, L.decode(cols))) == want


@pytest.mark.parametrize("name", list(RAISING))
def test_raising_cases(name):
    n, h, kind, row = RAISING[name]
    with pytest.raises(L.IllegalHistory) as e:
        L.check_host(n, h)
    assert (e.value.type, e.value.row) == ("illegal-history", row)
    assert ("exactly 2 keys" in e.value.msg) == (kind == 1) and ("distinct values" in e.value.msg) == (kind == 2)
    with pytest.raises(Illegal) as e2:
        ref_ops(n, h)
    assert e2.value.kind == kind and e2.value.row in (row, None)
    raw = ref_cols(L.encode(h), n)
    assert (raw["valid"], raw["cause"], raw["illegal_kind"], raw["illegal_row"]) == \
        (A.UNKNOWN, A.CAUSE_ILLEGAL_HISTORY, kind, row)


def test_error_payloads():
    n, h, _, _ = RAISING["wrong-size"]
    with pytest.raises(L.IllegalHistory) as e:
        L.check_host(n, h)
    assert e.value.msg == ("Every read in this history should have observed exactly 2 keys, but this read observed "
                           "3 instead: #{2 3 4}")
    assert e.value.data["op"]["value"] == h[1]["value"]
    n, h, _, _ = RAISING["distinct-values"]
    with pytest.raises(L.IllegalHistory) as e:
        L.check_host(n, h)
    assert e.value.data["key"] == 0 and e.value.data["reads"] == [{0: 1, 1: 5}, {0: 2, 1: 5}]


def test_golden_case_is_the_reference_map():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "long_fork.json")))
    got = L.check_host(g["n"], g["history"])
    for pair in got["forks"]:
        for op in pair:
            op.pop("index")
    assert got == g["expected"]
    assert CASES["golden"][0] == g["n"] and [op["value"] for op in CASES["golden"][1]] == \
        [op["value"] for op in g["history"]]


def test_namespace_functions():
    assert list(L.group_for(3, 7)) == [6, 7, 8] and list(L.group_for(3, -1)) == [-3, -2, -1]
    assert list(L.group_for(1, 5)) == [5] and list(L.group_for(4, -8)) == [-8, -7, -6, -5]
    t = L.read_txn_for(4, 9)
    assert sorted(m[1] for m in t) == [8, 9, 10, 11] and all(m[0] == "r" and m[2] is None for m in t)
    a, b = {0: 1, 1: None}, {0: None, 1: 1}
    assert L.read_compare(a, b) is None and L.read_compare(b, a) is None
    assert L.read_compare(a, a) == 0 and L.read_compare({0: 1, 1: 1}, a) == -1 and L.read_compare(a, {0: 1, 1: 1}) == 1
    for bad in (({0: 1}, {0: 1, 1: 1}), ({0: 1, 1: 1}, {0: 1, 2: 1}), ({0: 1}, {0: 2})):
        with pytest.raises(L.IllegalHistory):
            L.read_compare(*bad)
    assert L.read_op_to_value_map(ok(R((3, 1), (4, None)))) == {3: 1, 4: None}
    assert L.read_op_to_value_map({"value": None}) == {}
    assert L.distinct_pairs([1, 2, 3]) == [[1, 2], [1, 3], [2, 3]] and L.distinct_pairs([1]) == []
    assert L.read_txn_p(None) and L.read_txn_p([]) and L.read_txn_p(R((0, 1))) and not L.read_txn_p(W(0))
    assert L.write_txn_p(W(0)) and not L.write_txn_p(W(0) + W(1)) and not L.write_txn_p(None) and not L.write_txn_p([])
    assert L.legal_txn_p(W(1)) and L.legal_txn_p([]) and not L.legal_txn_p([["r", 0, 1], ["w", 1, 2]])
    h = CASES["two-groups-in-key-order"][1]
    assert [len(g) for g in L.groups(2, L.reads(h))] == [2, 3, 1]            # first appearance
    assert len(L.early_reads(L.reads(h))) == 0 and len(L.late_reads(L.reads(h))) == 1
    assert [[a["process"], b["process"]] for a, b in L.find_forks(L.reads(h)[:2])] == [[0, 1]]
    w = L.workload()
    assert isinstance(w["checker"], L.LongForkChecker) and w["checker"].n == 2 and L.workload(5)["checker"].n == 5
    assert checker.long_fork is L


def test_encoding():
    h = CASES["shape-not-f"][1] + [ok(None, 3, f="read"), ok([], 4), {"process": "nemesis", "type": "info", "f": "start",
                                                                         "value": "majority"}, inv(R((8, None), (9, None)))]
    c = L.encode(h)
    assert c.f.tolist() == [A.F_WRITE, A.F_READ, A.F_WRITE, 16, A.F_READ, A.F_READ, 17, A.F_READ]
    assert c.value.tolist() == [0, 0, 0, A.NIL, A.NIL, 2, A.NIL, A.NIL]
    assert c.value2.tolist() == [1, 2, 1, A.NIL, 0, 0, A.NIL, 0]         # only :ok rows carry their pairs
    assert c.aux.tolist() == [0, 1, 1, A.NIL] and c.process[6] == -1
    back = L.decode(c)
    assert back[1]["value"] == R((0, 1), (1, None)) and back[0]["value"] == W(0) and back[4]["value"] is None
    for v in (R(("x", 1)), R((0, 1.5)), R((0, False)), R((0, "a")), W(0.5), W(1, "v")):
        with pytest.raises(TypeError):
            L.encode([ok(v)])
    with pytest.raises(OverflowError):
        L.encode([ok(R((1 << 63, 1)))])
    # ... and the checker then answers from the host implementation
    h = [ok(R(("x", 1), ("y", None))), ok(R(("y", 1), ("x", None)), 1)]
    assert strip(L.checker(2).check({}, h, {})) == {"reads-count": 2, "early-read-count": 0, "late-read-count": 0,
                                                    "valid?": False, "forks": [[0, 1]]}


SYNTH = [dict(n=2, seed=0), dict(n=2, seed=1, forks=3), dict(n=3, seed=2, forks=2, sparse=True),
         dict(n=5, seed=3, forks=1, n_procs=9, p_info=0.2, p_fail=0.2), dict(n=1, seed=4),
         dict(n=2, seed=5, forks=2, repeat_write=300), dict(n=64, seed=6, forks=2, n_ops=300),
         dict(n=2, seed=7, forks=1, tile=3, sparse=True)]


@pytest.mark.parametrize("kw", SYNTH)
def test_restatements_agree_on_synth(kw):
    kw = dict(kw)
    n_ops = kw.pop("n_ops", 1200)
    cols = synth.long_fork_history(n_ops, **kw)
    n = kw["n"]
    ops = synth.long_fork_columns_to_ops(cols)
    a, b = ref_ops(n, ops), ref_cols(cols, n)
    assert b["rc"] == A.JH_OK
    want = raw_of_map(a, ops)
    assert {k: b[k] for k in want if k not in ("forks", "fork_groups")} == \
        {k: v for k, v in want.items() if k not in ("forks", "fork_groups")}
    assert b["forks"].tolist() == want["forks"]
    assert strip(L.check_host(n, ops)) == a
    tile = kw.get("tile", 1)
    assert cols.n >= 2 * n_ops * tile and a["reads-count"] > n_ops * tile // 4
    if kw.get("repeat_write") is not None:
        assert a["valid?"] == "unknown"
    else:
        assert b["fork_count"] == b["fork_groups"] == kw.get("forks", 0) * tile
        assert a["valid?"] is (b["fork_count"] == 0)
    if n <= 5:                                              # wide groups are hardly ever all nil or all seen
        assert 0 < a["early-read-count"] and 0 < a["late-read-count"] < a["reads-count"]


def _chain(masks):
    return all((a & ~b) == 0 or (b & ~a) == 0 for a, b in itertools.combinations(masks, 2))


def _counter_test(masks, n):
    """The device's pass A / pass B: no read has min(cnt over its set bits)
    <= max(cnt over its clear bits)."""
    cnt = [sum((m >> b) & 1 for m in masks) for b in range(n)]
    for m in masks:
        s = [cnt[b] for b in range(n) if (m >> b) & 1]
        c = [cnt[b] for b in range(n) if not (m >> b) & 1]
        if s and c and min(s) <= max(c):
            return False
    return True


def test_chain_equals_counter_test():
    """The masks of a group, as a multiset, form a chain under inclusion
    exactly when no read fails the counter test: every family of up to 4 masks
    for n <= 4, and 20 000 random families up to n = 8."""
    for n in range(1, 5):
        for size in range(0, 5):
            for fam in itertools.combinations_with_replacement(range(1 << n), size):
                assert _chain(fam) == _counter_test(fam, n), (n, fam)
    rng = np.random.default_rng(0)
    seen_false = 0
    for _ in range(20000):
        n = int(rng.integers(1, 9))
        size = int(rng.integers(1, 13))
        if rng.random() < 0.5:                              # a chain with duplicates, perhaps broken in one place
            order = rng.permutation(n)
            fam = [sum(1 << int(b) for b in order[:int(k)]) for k in rng.integers(0, n + 1, size)]
            if rng.random() < 0.5:
                fam[int(rng.integers(size))] ^= 1 << int(rng.integers(n))
        else:
            fam = rng.integers(0, 1 << n, size).tolist()
        ok_ = _chain(fam)
        seen_false += not ok_
        assert ok_ == _counter_test(fam, n), (n, fam)
    assert 2000 < seen_false < 18000


def test_ctypes_layout_long_fork(tmp_path):
    prog = tmp_path / "sz5.c"
    prog.write_text(f'''#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(jh_long_fork_opts),
         offsetof(jh_long_fork_opts, path), offsetof(jh_long_fork_opts, reserved), sizeof(jh_long_fork_result),
         offsetof(jh_long_fork_result, path), offsetof(jh_long_fork_result, illegal_kind),
         offsetof(jh_long_fork_result, reads_count), offsetof(jh_long_fork_result, late_count),
         offsetof(jh_long_fork_result, multiple_key), offsetof(jh_long_fork_result, illegal_row),
         offsetof(jh_long_fork_result, fork_groups), offsetof(jh_long_fork_result, entries),
         offsetof(jh_long_fork_result, device_ms), JH_ABI_VERSION, JH_CAUSE_MULTIPLE_WRITES,
         JH_CAUSE_ILLEGAL_HISTORY);
  return 0; }}''')
    exe = tmp_path / "sz5"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    O, Rs = A.JhLongForkOpts, A.JhLongForkResult
    want = [C.sizeof(O), O.path.offset, O.reserved.offset, C.sizeof(Rs), Rs.path.offset, Rs.illegal_kind.offset,
            Rs.reads_count.offset, Rs.late_count.offset, Rs.multiple_key.offset, Rs.illegal_row.offset,
            Rs.fork_groups.offset, Rs.entries.offset, Rs.device_ms.offset, A.JH_ABI_VERSION,
            A.CAUSE_MULTIPLE_WRITES, A.CAUSE_ILLEGAL_HISTORY]
    assert got == want
    assert A.JH_ABI_VERSION == 8                      # additive: the version does not move
    assert (C.sizeof(O), C.sizeof(Rs)) == (48, 96)
    assert A.CAUSES[10] == "multiple-writes" and A.CAUSES[11] == "illegal-history"
    assert A.LF_TILE == 4096 and "jh_check_long_fork" in __import__("jepsen_amd._native", fromlist=["x"]).EXPORTED_SYMBOLS
