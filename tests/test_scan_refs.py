"""The plain restatements of checker/counter and checker/set (counter_ref.py,
set_ref.py) against the reference's known answers and, field by field,
against the C oracle over the cases of scan_cases.py -- the same cases
test_gpu_scan_edges.py runs on the device. No GPU. The two sides were
written separately from checker.clj: a misreading on either side shows here.
"""
import json
import os

import pytest

import counter_ref
import scan_cases as S
import set_ref
from conftest import GOLD, load_npz_cols
from jepsen_amd import _abi as A
from jepsen_amd import history as H
from oracle import oracle
from oracle import queue as Q

inv, ok = H.invoke_op, H.ok_op


def _json(name):
    return json.load(open(os.path.join(GOLD, name)))


counter_same = counter_ref.same
set_same = set_ref.same


# -- known answers --------------------------------------------------------------
@pytest.mark.parametrize("case", _json("counter.json")["cases"], ids=lambda c: c["name"])
def test_counter_ref_known_answers(case):
    """checker_test.clj:90-166: the exact result maps."""
    assert counter_ref.result_map(case["history"]) == case["expected"]


@pytest.mark.parametrize("case", _json("interval_str.json")["cases"], ids=lambda c: c["expected"])
def test_set_ref_interval_str(case):
    """util_test.clj:14-31."""
    assert set_ref.interval_str(case["input"]) == case["expected"]


def test_set_ref_known_answers():
    """The set cases the suite checks the device and the oracle with."""
    assert set_ref.result_map([inv(0, "add", 1), ok(0, "add", 1)]) == \
        {"valid?": "unknown", "error": "Set was never read"}
    h = [inv(0, "add", 1), ok(0, "add", 1), inv(0, "add", 2), ok(0, "add", 2),
         inv(1, "read", None), ok(1, "read", [5]),
         inv(1, "read", None), ok(1, "read", [2, 1, 9])]
    r = set_ref.result_map(h)
    assert r == {"valid?": False, "attempt-count": 2, "acknowledged-count": 2, "ok-count": 2, "lost-count": 0,
                 "recovered-count": 0, "unexpected-count": 1, "ok": "#{1..2}", "lost": "#{}",
                 "unexpected": "#{9}", "recovered": "#{}"}
    # an empty final read is a read ((if-not []) is false); a nil one is none
    r = set_ref.result_map([inv(0, "add", 1), ok(0, "add", 1), inv(1, "read", None), ok(1, "read", [])])
    assert r["valid?"] is False and r["lost"] == "#{1}" and r["ok-count"] == 0
    assert set_ref.result_map([inv(1, "read", None), ok(1, "read", None)])["valid?"] == "unknown"


def _set_cols_to_ops(cols):
    """Op maps of a set history's columns (reads' elements from aux)."""
    ops = []
    for i in range(cols.n):
        f = {A.F_ADD: "add", A.F_READ: "read"}.get(int(cols.f[i]), "other")
        v = int(cols.value[i])
        if v == A.NIL:
            v = None
        elif f == "read":
            v = cols.aux[v:v + int(cols.value2[i])].tolist()
        ops.append({"process": int(cols.process[i]), "type": H.TYPE_NAMES[int(cols.type[i])], "f": f, "value": v})
    return ops


def test_set_ref_golden_vector(built):
    """tests/golden/synthetic_set.npz: the recorded verdict and lost runs."""
    cols, z = load_npz_cols("synthetic_set.npz")
    r = set_ref.check(_set_cols_to_ops(cols))
    assert r["valid"] == int(z["valid"]) and r["first_fail_entry"] == int(z["first_fail_entry"])
    assert r["runs"][1] == z["runs_lost"].tolist()
    assert [r[k] for k in set_ref.COUNTS] == [int(x) for x in z["counts"]]
    set_same(r, oracle.check_set(cols), "golden")


# -- the conventions for what the reference leaves to exceptions -----------------
@pytest.mark.parametrize("h,cause", [
    ([inv(0, "add", 1), inv(0, "add", 1)], "double-invoke"),
    ([ok(0, "add", 1)], "orphan-completion"),
    ([inv(0, "add", 1), H.info_op(0, "add", 1), inv(0, "add", 1)], "double-invoke"),
    ([inv(0, "add", None), ok(0, "add", None)], "nil-value"),
    ([inv(0, "add", None)], "nil-value"),
    ([inv(0, "read", None), ok(0, "read", None)], "nil-value"),
    ([inv(0, "add", 1), ok(0, "read", 1)], "orphan-completion"),
    (S.counter_big_adds(1 << 62, 3), "overflow"),
])
def test_counter_ref_unknown_causes(built, h, cause):
    r = counter_ref.check(h)
    assert r["valid"] == A.UNKNOWN and A.CAUSES[r["cause"]] == cause
    counter_same(r, oracle.check_counter(H.encode(h, keyed=False)))


def test_counter_ref_details(built):
    """(or inv ok), (remove :fails?), a read invoked with its value, a crashed
    add counted in upper only, negative adds (lower above upper)."""
    h = [inv(0, "add", None), ok(0, "add", 5),              # upper 5 lower 5
         inv(1, "add", 7), H.fail_op(1, "add", 7),          # removed
         inv(2, "add", 2),                                  # crashed: upper 7
         inv(3, "read", 6), ok(3, "read", 6),               # [5 6 7]
         inv(0, "add", -10),                                # upper -3
         inv(1, "read", None), ok(1, "read", 5),            # [5 5 -3]: an error
         ok(0, "add", -10)]
    r = counter_ref.check(h)
    assert r["reads"] == [[5, 6, 7], [5, 5, -3]] and r["n_errors"] == 1 and r["first_err_entry"] == 9
    counter_same(r, oracle.check_counter(H.encode(h, keyed=False)))
    # just inside the device's overflow guard: two adds of 2^60 have a sum
    assert counter_ref.check(S.counter_big_adds(1 << 60, 2))["reads"] == [[1 << 61, 1 << 61, 1 << 61]]


# -- restatement against the C oracle over the shared cases -----------------------
def test_counter_sweep_vs_oracle(built):
    """Every row count x process count x value set of the device sweep. The
    reference alone may answer :unknown for at most 10% of them."""
    n = unknown = 0
    for vs in S.COUNTER_VALUE_SETS:
        for n_procs in S.COUNTER_PROCS:
            for name, ops in S.counter_sweep(vs, n_procs):
                r = counter_ref.check(ops)
                counter_same(r, oracle.check_counter(S.encode(ops)[1]), name)
                n += 1
                unknown += r["valid"] == A.UNKNOWN
    assert n == len(S.COUNTER_VALUE_SETS) * len(S.COUNTER_PROCS) * len(S.COUNTER_ROWS)
    assert unknown <= 0.10 * n, (unknown, n)


def test_counter_builder_rules():
    """Every invocation is completed by an :ok or a :fail of its process, and
    the sweep does use nil invocation values and values outside the 27-bit
    field."""
    nil = wide = 0
    for name, ops in S.counter_sweep("field-edges", 33):
        open_ = {}
        for o in ops:
            if o["type"] == "invoke":
                assert o["process"] not in open_, name
                open_[o["process"]] = o
                nil += o["f"] == "add" and o["value"] is None
            elif o["type"] in ("ok", "fail"):
                i = open_.pop(o["process"])
                wide += i["f"] == "add" and not -(1 << 26) <= o["value"] < (1 << 26)
        assert not open_, name
    assert nil > 100 and wide > 100


@pytest.mark.parametrize("name", list(S.COUNTER_EDGE_CASES))
def test_counter_edge_cases_vs_oracle(built, name):
    ops = S.COUNTER_EDGE_CASES[name]()
    r = counter_ref.check(ops)
    assert r["valid"] != A.UNKNOWN
    for off in (0, -5, 10 ** 9):
        o2, cols = S.encode(ops, off)
        counter_same(counter_ref.check(o2), oracle.check_counter(cols), name)
        assert counter_ref.check(o2)["reads"] == r["reads"]
    if name == "errors-around-chunk-edges":
        assert (r["n_errors"], r["first_err_entry"]) == (6, 2046)
    if name == "many-processes":
        assert len({o["process"] for o in ops[:2048]}) > 1024


def test_set_cases_vs_oracle(built):
    unknown = 0
    for name, build in S.SET_CASES.items():
        ops = build()
        r = set_ref.check(ops)
        set_same(r, oracle.check_set(S.encode(ops)[1]), name)
        unknown += r["valid"] == A.UNKNOWN
    assert unknown <= 0.10 * len(S.SET_CASES)


def test_set_case_shapes():
    """The cases are what their names say."""
    for k in S.SET_READ_SIZES:
        ops = S.SET_CASES[f"read-{k}"]()
        assert len(ops[-1]["value"]) == k and ops[-1]["type"] == "ok"
    assert len(S.SET_CASES["odd-n"]()) % 2 == 1 and len(S.SET_CASES["asc"]()) % 2 == 0
    base, dense, sparse = (set_ref.check(S.SET_CASES[f"switch-{s}"]()) for s in ("base", "dense", "sparse"))
    for r in (dense, sparse):        # the far element is one more ok run; nothing else moves
        assert r["runs"][0][:-1] == base["runs"][0] and r["runs"][1:] == base["runs"][1:]
    assert sparse["runs"][0][-1][0] == dense["runs"][0][-1][0] + 1
    ops = S.SET_CASES["switch-dense"]()
    n, cnt = len(ops), len(ops[-1]["value"])
    lo = min(min(ops[-1]["value"]), min(o["value"] for o in ops if o["f"] == "add"))
    assert dense["runs"][0][-1][1] - lo + 1 == 8 * (n + cnt) + 4096
    r = set_ref.check(S.SET_CASES["vmin-17"]())
    assert [200 + 17, 299 + 17] in r["runs"][0] and [30 + 17, 34 + 17] in r["runs"][0]
    assert (r["lost_count"], r["unexpected_count"], r["recovered_count"]) == (1, 1, 1)


def test_queue_cases_build():
    """oracle/queue.py runs every queue case; the clean span cases are
    accepted by the queue model with nil in the final queue."""
    for name, build in S.QUEUE_CASES.items():
        ops = build()
        t = Q.total_queue(ops)
        assert t["attempt-count"] > 0, name
        q = Q.queue(ops)
        if name.endswith("-clean"):
            assert q["valid?"] and q["final-queue"][None] > 0, name
    for k in S.DRAIN_SIZES:
        ops = S.QUEUE_CASES[f"drain-{k}"]()
        assert len(ops[-1]["value"]) == k and None in ops[-1]["value"]
