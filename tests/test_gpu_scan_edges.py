"""The counter, set and queue scan kernels (jh_counter.hip, jh_set.hip,
jh_queue.hip) at their structural edges, against the plain restatements
(counter_ref.py, set_ref.py, oracle/queue.py) and the C oracle, every result
field. The cases come from scan_cases.py; test_scan_refs.py checks the same
cases between the restatements and the oracle without a device.

Which input takes which branch is argued from the kernels' code in each
docstring (CHUNK = CNT_TILE = 2048 rows, PAIR_PROCS = 32, HSLOTS = 1024,
RB_CH = 8192, DRAIN_CHUNK = 4096).
"""
import pytest

import counter_ref
import scan_cases as S
import set_ref
from jepsen_amd import _abi as A
from jepsen_amd import checker, model
from jepsen_amd import history as H
from jepsen_amd._native import JhError, bits_to_runs
from oracle import oracle
from oracle import queue as Q

pytestmark = pytest.mark.gpu

inv, ok, fail, info = H.invoke_op, H.ok_op, H.fail_op, H.info_op


# -- counter --------------------------------------------------------------------
def _counter_all(ctx, ops, what, proc_offset=0):
    ops, cols = S.encode(ops, proc_offset)
    ref = counter_ref.check(ops)
    counter_ref.same(ref, ctx.check_counter(cols), what)
    counter_ref.same(ref, oracle.check_counter(cols), what + " (oracle)")
    return ref, cols


@pytest.mark.parametrize("n_procs", S.COUNTER_PROCS)
@pytest.mark.parametrize("vs", list(S.COUNTER_VALUE_SETS))
def test_counter_sweep(ctx, vs, n_procs):
    """Row counts 1 .. 6150 around the 2048-row chunk / tile edges, adds of
    every value set with 20% nil invocation values.

    field-edges and wide: cw_make / the word pass set CW_X for a value outside
    [-2^26, 2^26-1]; k_cnt_tile_scan's cw_val then reads val[r], and for a nil
    invocation val[pair[r]], which the pack wrote (hi && !own && !fits). With
    33 and 70 processes a chunk has more than PAIR_PROCS distinct ones: the
    invocations of the others spill, and k_cnt_pair_spill writes CW_X words
    and pair[r] = got itself. -1 and -2^40 make lower pass upper. 4097 and
    6150 rows invoke their reads with the value (val[inv] != nil in
    k_cnt_triples)."""
    n = unknown = 0
    for name, ops in S.counter_sweep(vs, n_procs):
        ref, _ = _counter_all(ctx, ops, name)
        n += 1
        unknown += ref["valid"] == A.UNKNOWN
    assert unknown == 0 and n == len(S.COUNTER_ROWS)


@pytest.mark.parametrize("proc_offset", [0, -5, 10 ** 9])
@pytest.mark.parametrize("name", list(S.COUNTER_EDGE_CASES))
def test_counter_edge_cases(ctx, name, proc_offset):
    """many-processes: 1100 distinct processes in the first chunk overflow its
    1024-slot process table: the rest take slot = -1 (atomicMax on the global
    last[] row by row), and tab_n > PAIR_PROCS makes every spill walk the rows.
    error-read-across-chunks: the read invoked at row 2000 spills; its :ok at
    row 2100 keeps CW_U until k_cnt_pair_spill claims it, writes pair[] and
    counts it in tile 1. errors-around-chunk-edges: k_cnt_triples' atomicMin
    must leave row 2046. Process ids offset by -5 and 10^9: cp = proc - pmin."""
    ref, _ = _counter_all(ctx, S.COUNTER_EDGE_CASES[name](), name, proc_offset)
    assert ref["n_reads"] > 0


def test_counter_reads_cap(ctx):
    """reads_cap 0 and n_reads - 1: the counts and the first error are those of
    the full result, the triples its prefix."""
    ops, cols = S.encode(S.COUNTER_EDGE_CASES["completed-history-reads"]())
    ref = counter_ref.check(ops)
    assert ref["n_reads"] > 2 and ref["n_errors"] > 0
    for cap in (0, ref["n_reads"] - 1):
        g = ctx.check_counter(cols, reads_cap=cap)
        for k in ("valid", "cause", "n_reads", "n_errors", "first_err_entry"):
            assert g[k] == ref[k], (cap, k)
        assert g["reads"].tolist() == ref["reads"][:cap], cap


def test_counter_overflow_guard(ctx):
    """The guard refuses when amax_abs > LLONG_MAX / n_add, n_add the :invoke
    and :ok :add rows. Two acknowledged adds of 2^60: n_add = 4, LLONG_MAX / 4
    = 2^61 - 1 >= 2^60: answered, and equal to the reference (no prefix sum
    passes 2^61). Three of 2^62: n_add = 6, LLONG_MAX / 6 < 2^61 < 2^62:
    refused (the reference throws: upper passes a long at the third)."""
    ref, _ = _counter_all(ctx, S.counter_big_adds(1 << 60, 2), "inside the guard")
    assert ref["valid"] == A.VALID and ref["reads"] == [[1 << 61] * 3]
    ops = S.counter_big_adds(1 << 62, 3)
    assert A.CAUSES[counter_ref.check(ops)["cause"]] == "overflow"
    with pytest.raises(JhError) as e:
        ctx.check_counter(S.encode(ops)[1])
    assert e.value.code == A.JH_EUNSUPPORTED


def test_counter_process_span_refused(ctx):
    ops = [inv(0, "add", 1), ok(0, "add", 1), inv(1 << 28, "add", 1), ok(1 << 28, "add", 1)]
    with pytest.raises(JhError) as e:
        ctx.check_counter(S.encode(ops)[1])
    assert e.value.code == A.JH_EUNSUPPORTED


# -- set --------------------------------------------------------------------------
def _bits_same(ref, b, what):
    for k in ("valid", "cause", "first_fail_entry", "final_read_entry") + set_ref.COUNTS:
        assert ref[k] == b[k], (what, k, ref[k], b[k])
    assert ref["n_runs"] == b["n_runs"], what
    for i in range(4):
        assert bits_to_runs(b["bits"][i], b["base"]).tolist() == ref["runs"][i], (what, set_ref.NAMES[i])


def _set_all(ctx, ops, what):
    cols = S.encode(ops)[1]
    ref = set_ref.check(ops)
    set_ref.same(ref, ctx.check_set(cols), what)
    _bits_same(ref, ctx.check_set_bitmaps(cols), what + " (bitmaps)")
    set_ref.same(ref, oracle.check_set(cols), what + " (oracle)")
    return ref, cols


@pytest.mark.parametrize("name", list(S.SET_CASES))
def test_set_cases(ctx, name):
    """asc / desc: consecutive lanes of k_rb_hist / k_rb_scatter fall into one
    bucket (lane_runs: one run per wave), and k_rb_build's neighbouring lanes
    share words (the segmented OR). read-twice: duplicate elements in a read.
    attempted-twice: idempotent byte stores. earlier-reads: elements of :ok
    reads before the last one, outside its span, and an :info and a :fail
    read after it. vmin-*: bit b is element vmin + b; the named runs cross
    word edges (32) and bucket edges (2^sb = 64 at this span); 100 consecutive
    elements make k_set_emit follow a run over four words. read-k: k around
    the RB_CH = 8192 block edges, spans over 8192 (sb > 5). switch-*: the
    same history at span == 8 (n + cnt) + 4096 (k_rb_* and the byte maps) and
    one element further (k_set_mark_*)."""
    ref, _ = _set_all(ctx, S.SET_CASES[name](), name)
    assert ref["valid"] != A.UNKNOWN


def test_set_dense_sparse_switch(ctx):
    """Either side of the switch: the device's runs differ by the far element
    only."""
    res = {}
    for side in ("base", "dense", "sparse"):
        cols = S.encode(S.SET_CASES[f"switch-{side}"]())[1]
        res[side] = ctx.check_set(cols)
    base = [r.tolist() for r in res["base"]["runs"]]
    for side in ("dense", "sparse"):
        got = [r.tolist() for r in res[side]["runs"]]
        assert got[0][:-1] == base[0] and got[1:] == base[1:], side
    assert res["sparse"]["runs"][0][-1][0] == res["dense"]["runs"][0][-1][0] + 1


@pytest.mark.parametrize("name", ["asc", "vmin-neg-1000"])
def test_set_runs_cap_and_words_cap(ctx, name):
    """runs_cap = n_runs - 1 of each set in turn and words_cap < n_words: the
    counts stay complete, what is written is a prefix."""
    ops = S.SET_CASES[name]()
    cols = S.encode(ops)[1]
    ref = set_ref.check(ops)
    assert all(n > 0 for n in ref["n_runs"])
    for cap in sorted({n - 1 for n in ref["n_runs"]}):
        g = ctx.check_set(cols, runs_cap=cap)
        assert g["n_runs"] == ref["n_runs"], cap
        for k in ("valid", "first_fail_entry") + set_ref.COUNTS:
            assert g[k] == ref[k], (cap, k)
        for i in range(4):
            assert g["runs"][i].tolist() == ref["runs"][i][:cap], (cap, set_ref.NAMES[i])
    full = ctx.check_set_bitmaps(cols)
    nw = full["n_words"]
    assert nw > 8
    for cap in (nw - 1, 3):
        b = ctx.check_set_bitmaps(cols, words_cap=cap)
        assert b["n_words"] == nw and b["base"] == full["base"] and b["n_runs"] == ref["n_runs"]
        for k in ("valid", "first_fail_entry") + set_ref.COUNTS:
            assert b[k] == ref[k], (cap, k)
        for i in range(4):
            assert len(b["bits"][i]) == cap and (b["bits"][i] == full["bits"][i][:cap]).all()


@pytest.mark.parametrize("ops", [
    [inv(0, "add", None), ok(0, "add", None), inv(1, "read", None), ok(1, "read", [1])],
    [inv(0, "add", None), info(0, "add", None), inv(1, "read", None), ok(1, "read", [1])],
    [inv(0, "add", 0), ok(0, "add", 0), inv(0, "add", 1 << 35), ok(0, "add", 1 << 35),
     inv(1, "read", None), ok(1, "read", [0, 1 << 35])],
], ids=["nil-acknowledged", "nil-attempted", "span-2^35"])
def test_set_refusals(ctx, ops):
    cols = S.encode(ops)[1]
    for call in (lambda: ctx.check_set(cols), lambda: ctx.check_set_bitmaps(cols, words_cap=16)):
        with pytest.raises(JhError) as e:
            call()
        assert e.value.code == A.JH_EUNSUPPORTED


# -- queue ------------------------------------------------------------------------
MULTISETS = ("lost", "unexpected", "duplicated", "recovered")


def _total_same(got, want, what):
    for k, v in want.items():
        assert (dict(got[k]) if k in MULTISETS else got[k]) == (dict(v) if k in MULTISETS else v), (what, k)


def _queue_same(got, want, what):
    assert got["valid?"] == want["valid?"], what
    if want["valid?"]:
        assert dict(got["final-queue"]) == dict(want["final-queue"]), what
    else:
        assert (got["fail-entry"], got["error"]) == (want["fail-index"], want["error"]), what


def _nil_last(pairs):
    """(value, multiplicity) pairs ascending by value, nil after every value."""
    v = [int(x) for x in pairs[:, 0]]
    body = v[:-1] if v and v[-1] == A.NIL else v
    return A.NIL not in body and body == sorted(set(body)) and all(int(c) > 0 for c in pairs[:, 1])


def _queue_all(ctx, ops, what):
    cols = S.encode(ops)[1]
    want = Q.total_queue(ops)
    _total_same(checker.total_queue().check({}, ops, {}), want, what + " (op maps)")
    _total_same(checker.total_queue().check({}, cols, {}), want, what + " (columns)")
    raw = ctx.check_total_queue(cols)
    assert all(_nil_last(raw[k]) for k in MULTISETS), what
    qm = checker.queue(model.unordered_queue())
    wq = Q.queue(ops)
    _queue_same(qm.check({}, ops, {}), wq, what + " (op maps)")
    _queue_same(qm.check({}, cols, {}), wq, what + " (columns)")
    if wq["valid?"]:
        assert _nil_last(ctx.check_queue(cols)["final_queue"]), what
    return want, wq, cols


@pytest.mark.parametrize("name", list(S.QUEUE_CASES))
def test_queue_cases(ctx, name):
    """S-k: the value table has k slots and nil takes id k - 1; at k = 2^8 + 1
    and 2^16 + 1 that id alone needs the radix sort's top bit (end_bit is the
    first with 2^end_bit >= S). drain-k: k_q_drain takes DRAIN_CHUNK = 4096
    elements per block (gridDim.x = 1, 1, 2, 3). drains: a drain [], a nil
    drain (count 0), a :fail drain (skipped)."""
    want, wq, _ = _queue_all(ctx, S.QUEUE_CASES[name](), name)
    if name.endswith("-clean"):
        assert wq["valid?"] and wq["final-queue"][None] > 0
    if name.startswith("drain-"):
        assert want["duplicated-count"] > 0 and want["unexpected-count"] > 0


def test_queue_many_drains(ctx):
    """70,000 :ok :drain rows: k_q_drain's grid takes 65,535 rows in y, so
    total_queue_check launches it twice (the r0 loop); the last 4,465 drains
    count in the second launch."""
    ops = S.many_drains()
    cols = S.encode(ops)[1]
    want = Q.total_queue(ops)
    assert sum(1 for o in ops if o["f"] == "drain" and o["type"] == "ok") == 70_000
    _total_same(checker.total_queue().check({}, cols, {}), want, "many drains")
    _queue_same(checker.queue(model.unordered_queue()).check({}, cols, {}), Q.queue(ops), "many drains")


def test_queue_pairs_cap(ctx):
    """pairs_cap = n_pairs - 1 of each multiset in turn, and of the final
    queue: n_pairs stays complete, the pairs are a prefix in the documented
    order (ascending by value, nil last), so the pair left out of a multiset
    that holds nil is nil's."""
    ops = S.QUEUE_CASES["S-257"]()
    cols = S.encode(ops)[1]
    want = Q.total_queue(ops)
    full = ctx.check_total_queue(cols)
    assert all(n > 0 for n in full["n_pairs"]) and any(None in want[k] for k in MULTISETS)
    for i, k in enumerate(MULTISETS):
        assert full["n_pairs"][i] == len(want[k]) and _nil_last(full[k])
        assert (int(full[k][-1, 0]) == A.NIL) == (None in want[k])
    for cap in sorted({n - 1 for n in full["n_pairs"]}):
        g = ctx.check_total_queue(cols, pairs_cap=cap)
        assert g["n_pairs"] == full["n_pairs"], cap
        for k in MULTISETS:
            assert g[k].tolist() == full[k][:cap].tolist(), (cap, k)
            assert g[k + "_count"] == full[k + "_count"]
    ops = S.QUEUE_CASES["S-257-clean"]()
    cols = S.encode(ops)[1]
    want = Q.queue(ops)["final-queue"]
    full = ctx.check_queue(cols)
    n = full["n_pairs"][0]
    assert n == len(want) > 1 and int(full["final_queue"][-1, 0]) == A.NIL and _nil_last(full["final_queue"])
    g = ctx.check_queue(cols, pairs_cap=n - 1)
    assert g["n_pairs"][0] == n and g["final_queue"].tolist() == full["final_queue"][:n - 1].tolist()
    assert A.NIL not in g["final_queue"][:, 0].tolist()


def _deq(p, v):
    return [inv(p, "dequeue", None), ok(p, "dequeue", v)]


def _enq(p, v, t="ok"):
    return [inv(p, "enqueue", v), {"process": p, "type": t, "f": "enqueue", "value": v}]


@pytest.mark.parametrize("name,ops,fail_row", [
    # values 7, -3 and 9 go negative at rows 9, 11 and 13
    ("three-negative", _enq(0, 7) + _enq(0, -3) + _deq(1, -3) + _deq(1, 7) + _deq(2, 7) + _deq(2, -3) +
     _deq(1, 9), 9),
    ("negative-then-enqueued-again", _enq(0, 4) + _deq(1, 4) + _deq(1, 4) + _enq(0, 4) + _enq(0, 4), 5),
    ("failing-dequeue-at-row-0", [ok(1, "dequeue", 5)] + _enq(0, 5) + _deq(1, 5), 0),
    ("no-queue-rows", [inv(0, "read", None), ok(0, "read", 3), inv(1, "drain", None), fail(1, "drain", None)], None),
    ("failed-enqueue-counts", _enq(0, 1, "fail") + _deq(1, 1) + _enq(0, None, "fail") + _deq(1, None), None),
])
def test_queue_model_rows(ctx, name, ops, fail_row):
    """The queue model's first failing row is the smallest row at which any
    value's running count goes negative (k_q_neg's atomicMin over the sorted
    segments); an :invoke :enqueue counts whatever completes it."""
    want, wq, cols = _queue_all(ctx, ops, name)
    assert wq.get("fail-index") == fail_row
    if name == "three-negative":
        # the rows are sorted by value: -3's failure (row 11) comes first there, 7's (row 9) first in the history
        assert ctx.check_queue(cols)["fail_value"] == 7
    if name == "no-queue-rows":
        assert wq["final-queue"] == {} and want["attempt-count"] == 0


def test_queue_refusals(ctx):
    """Values spanning 2^31 or more: JH_EUNSUPPORTED from both entry points, for
    op maps and columns alike. A crashed drain: JH_EINVAL (the reference
    throws)."""
    ops = _enq(0, 0) + _enq(0, 1 << 31) + _deq(1, 0)
    cols = S.encode(ops)[1]
    tq, qm = checker.total_queue(), checker.queue(model.unordered_queue())
    for call in (lambda: tq.check({}, ops, {}), lambda: tq.check({}, cols, {}),
                 lambda: qm.check({}, ops, {}), lambda: qm.check({}, cols, {})):
        with pytest.raises(JhError) as e:
            call()
        assert e.value.code == A.JH_EUNSUPPORTED
    crashed = _enq(0, 1) + [inv(2, "drain", None), info(2, "drain", None)]
    with pytest.raises(ValueError):
        Q.total_queue(crashed)
    with pytest.raises(JhError) as e:
        ctx.check_total_queue(S.encode(crashed)[1])
    assert e.value.code == A.JH_EINVAL
