"""(checker/unique-ids) on the device (jh_check_unique_ids, jh_uids.hip)
against the CPU restatements of tests/unique_ids_ref.py: whole result maps,
on the dense (bitmap) and the sorted path, and the path taken.
checker_test.clj has no unique-ids case: parity is unpinned against the
reference's own tests."""
import numpy as np
import pytest

from jepsen_amd import _abi as A
from jepsen_amd import _native, checker, independent, synth
from jepsen_amd import history as H
from jepsen_amd.history import Columns
from unique_ids_ref import f_generate, ref_cols, ref_ops

pytestmark = pytest.mark.gpu

PATHS = [1, 2]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def g(t, v, p=0, f="generate"):
    return {"process": p, "type": t, "f": f, "value": v}


def run(history, path, cap=48):
    """(result map, path taken) of the device checker."""
    c = checker.UniqueIds(path=path, dup_cap=cap)
    r = c.check({}, history, {})
    return r, c.last_path


def same(got, want):
    assert got == want
    assert list(got["duplicated"]) == list(want["duplicated"])      # ascending id


def ok_cols(ids):
    """Columns of :ok :generate rows carrying `ids`, in order."""
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    return Columns(n=n, process=np.arange(n, dtype=np.int64) % 7, type=np.full(n, A.TYPE_OK, np.int64),
                   f=np.full(n, 16, np.int64), key=np.full(n, -1, np.int64), value=ids,
                   value2=np.full(n, A.NIL, np.int64), n_keys=0, aux=np.zeros(1, np.int64), f_names=["generate"])


def want_of(cols):
    """The op-map restatement's answer for a Columns history."""
    return ref_ops(synth.unique_ids_columns_to_ops(cols))


EMPTY = {"valid?": True, "attempted-count": 0, "acknowledged-count": 0, "duplicated-count": 0,
         "duplicated": {}, "range": [None, None]}

HAND = {
    "empty": ([], 0),
    "no-generate": ([g("invoke", None, 0, "read"), g("ok", 5, 0, "read"), g("info", None, "nemesis", "start")], 0),
    "only-invokes": ([g("invoke", None, p) for p in range(5)], 0),
    "one-ack": ([g("invoke", None), g("ok", -12345678901)], None),
    "all-nil": ([g("invoke", None, p) for p in range(3)] + [g("ok", None, p) for p in range(3)], None),
    "fail-info-carry-an-acked-id": ([g("invoke", None), g("ok", 4), g("invoke", None, 1), g("fail", 4, 1),
                                     g("invoke", None, 2), g("info", 4, 2), g("invoke", None, 3), g("ok", 9, 3)], None),
    "read-collides": ([g("invoke", None), g("ok", 4), g("invoke", None, 1, "read"), g("ok", 4, 1, "read"),
                       g("invoke", None, 1, "read"), g("ok", 4, 1, "read")], None),
    "nemesis-generate": ([g("invoke", None, "nemesis"), g("ok", 8, "nemesis"), g("invoke", None), g("ok", 8),
                          g("info", None, "nemesis", "start")], None),
}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(HAND))
def test_hand_cases(ctx, name, path):
    h, want_path = HAND[name]
    assert len(h) <= 40
    want = ref_ops(h)
    got, took = run(h, path)
    same(got, want)
    assert took == (path if want_path is None else want_path)
    if name in ("empty", "no-generate"):
        assert got == EMPTY
    if name == "only-invokes":
        assert got == dict(EMPTY, **{"attempted-count": 5})
    if name == "all-nil":
        assert got["range"] == [None, None] and got["duplicated"] == {None: 3} and got["valid?"] is False
    if name == "fail-info-carry-an-acked-id":
        assert got["valid?"] is True and got["acknowledged-count"] == 2 and got["range"] == [4, 9]
    if name == "read-collides":
        assert got["valid?"] is True and got["acknowledged-count"] == 1
    if name == "nemesis-generate":
        assert got["duplicated"] == {8: 2} and got["attempted-count"] == 2


def test_same_bit_within_one_wave(ctx):
    """Dense path: two lanes of one wave carrying the same bit. Rows 3 and 4
    of 64 consecutive acks share an id; then all 64 rows carry one id."""
    ids = 1000 + np.arange(64, dtype=np.int64)
    ids[4] = ids[3]
    cols = ok_cols(ids)
    got, took = run(cols, 1)
    assert took == 1
    same(got, want_of(cols))
    assert got["duplicated"] == {1003: 2} and got["duplicated-count"] == 1
    cols = ok_cols(np.full(64, -77, np.int64))
    got, took = run(cols, 1)
    assert took == 1
    same(got, want_of(cols))
    assert got["duplicated"] == {-77: 64} and got["range"] == [-77, -77]


@pytest.mark.parametrize("path", PATHS)
def test_same_word_different_waves_and_blocks(ctx, path):
    lo = -5_000_000_000
    ids = lo + np.arange(20_000, dtype=np.int64)
    ids[[10, 9_000, 19_990]] = lo + 5
    cols = ok_cols(ids)
    got, took = run(cols, path)
    assert took == path
    same(got, want_of(cols))
    assert got["duplicated"] == {lo + 5: 4} and got["acknowledged-count"] == 20_000


def test_sorted_path_extremes(ctx):
    """The full signed range: keys id - lo wrap from INT64_MIN + 1 to
    INT64_MAX without losing the order; nil twice; the dense path refuses."""
    ids = [I64_MIN + 1, -1, 0, I64_MAX, A.NIL, 0, I64_MAX, -1, I64_MIN + 1, A.NIL]
    cols = ok_cols(ids)
    want = want_of(cols)
    assert want["duplicated"] == {None: 2, I64_MIN + 1: 2, -1: 2, 0: 2, I64_MAX: 2}
    assert want["range"] == [None, I64_MAX]
    for path in (2, 0):
        got, took = run(cols, path)
        assert took == 2
        same(got, want)
    with pytest.raises(_native.JhError) as e:
        run(cols, 1)
    assert e.value.code == A.JH_EINVAL


@pytest.mark.parametrize("path", PATHS)
def test_run_longer_than_a_block(ctx, path):
    """One id 5 000 times among 30 000 sparse ids (a run over many blocks of
    the runs kernel), one id 3 times, and the largest id twice (a run that
    ends at n - 1). The ids span 2^30, so both paths take them."""
    rng = np.random.default_rng(5)
    ids = 123_456_789_012 + rng.permutation(1 << 20)[:30_000].astype(np.int64) * 1024 + rng.integers(0, 1024, 30_000)
    ids[1 + rng.permutation(29_999)[:4_999]] = ids[0]
    top = int(ids.max())
    free = np.nonzero((ids != ids[0]) & (ids != top))[0]
    ids[free[:2]] = ids[free[2]]
    ids[free[3]] = top
    cols = ok_cols(ids)
    want = want_of(cols)
    assert sorted(want["duplicated"].values()) == [2, 3, 5_000] and want["duplicated"][top] == 2
    got, took = run(cols, path)
    assert took == path
    same(got, want)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n_dup", [47, 48, 49, 300])
def test_selection(ctx, n_dup, path):
    """Many equal counts, a few larger ones and nil among the duplicated ids,
    around the reference's (take 48) and at other caps."""
    cols = synth.unique_ids_history(4000, dups=[(n_dup - 4, 2), (2, 5), (1, 3)], nil_acks=2, seed=n_dup)
    ops = synth.unique_ids_columns_to_ops(cols)
    assert ref_ops(ops)["duplicated-count"] == n_dup
    for cap in (0, 1, 48, n_dup + 10):
        want = ref_ops(ops, cap=cap)
        assert len(want["duplicated"]) == min(cap, n_dup)
        got, took = run(cols, path, cap=cap)
        assert took == path
        same(got, want)


def test_auto_path(ctx):
    cols = synth.unique_ids_history(5000, kind="counter", dups=[(3, 2)], seed=1)
    got, took = run(cols, 0)
    assert took == 1
    same(got, want_of(cols))
    cols = synth.unique_ids_history(5000, kind="flake", dups=[(3, 2)], seed=1)
    got, took = run(cols, 0)
    assert took == 2
    same(got, want_of(cols))


@pytest.mark.parametrize("path", PATHS)
def test_interned_string_ids(ctx, path):
    """String ids, nemesis rows with string values: op maps through
    checker.unique_ids(); the ids reach the device as ranks in compare order."""
    cols = synth.unique_ids_history(600, kind="string", dups=[(4, 2), (1, 3)], nil_acks=2, seed=2)
    assert cols.values_interned and any(isinstance(x, str) and x.startswith("partition") for x in cols.value_table)
    ops = synth.unique_ids_columns_to_ops(cols)
    want = ref_ops(ops)
    assert want["duplicated-count"] == 6 and isinstance(want["range"][1], str)
    same(checker.unique_ids(path).check({}, ops, {}), want)
    same(checker.unique_ids(path).check({}, cols, {}), want)


def test_mixed_id_types_are_unknown(ctx):
    h = [g("invoke", None), g("ok", 5), g("invoke", None, 1), g("ok", "five", 1),
         g("info", "partitioned", "nemesis", "start")]
    with pytest.raises(TypeError):
        ref_ops(h)
    r = checker.check_safe(checker.unique_ids(), {}, h, {})
    assert r["valid?"] == "unknown" and "TypeError" in r["error"]
    # a nil ack beside them: nil compares with everything, 5 and "five" still do not
    hn = [g("invoke", None, 2), g("ok", None, 2)] + h
    with pytest.raises(TypeError):
        ref_ops(hn)
    for path in (0, 1, 2):
        r = checker.check_safe(checker.unique_ids(path), {}, hn, {})
        assert r["valid?"] == "unknown" and "TypeError" in r["error"]
    # string ids next to a nemesis string value alone are fine
    h[1] = g("ok", "four")
    same(checker.unique_ids().check({}, h, {}), ref_ops(h))


@pytest.mark.parametrize("shift", [0, 1])
def test_device_columns_and_multi_context(ctx, shift):
    """Device-resident columns, 16-byte aligned (row pairs in one load) and
    8-byte aligned only, and a jh_open_multi context: the host columns' result."""
    from hipcols import DevCols
    cols = synth.unique_ids_history(30_001, dups=[(5, 2), (2, 7)], nil_acks=3, seed=4)
    fg = f_generate(cols)
    d = DevCols(cols, shift)
    mctx = _native.Context(n_gpus=1)
    try:
        for path in PATHS:
            host = ctx.check_unique_ids(cols, fg, path=path)
            assert host["duplicated_count"] == 8 and host["path"] == path
            for other in (ctx.check_unique_ids(d, fg, path=path, on_device=True),
                          mctx.check_unique_ids(cols, fg, path=path)):
                for k, v in host.items():
                    if k == "duplicated":
                        assert (other[k] == v).all()
                    elif k != "device_ms":
                        assert other[k] == v, k
    finally:
        mctx.close()


def test_c_abi_arguments(ctx):
    cols = ok_cols([1, 2, 2])
    with pytest.raises(_native.JhError) as e:
        ctx.check_unique_ids(cols, -1)
    assert e.value.code == A.JH_EINVAL
    r = ctx.check_unique_ids(cols, 16, dup_cap=0)
    assert r["duplicated_count"] == 1 and len(r["duplicated"]) == 0 and r["valid"] == A.INVALID
    assert r["nil_count"] == 0 and (r["range_lo"], r["range_hi"]) == (1, 2)


def test_under_independent_checker(ctx):
    """A generic inner checker of independent/checker: one check per key."""
    t = H.tuple_
    h = []
    for k, ids in (("a", [1, 2, 3, 2]), ("b", [10, 11]), ("c", [None, None, 7])):
        for i in ids:
            h += [g("invoke", t(k, None), 1), g("ok", t(k, i), 1)]
    h.insert(4, g("info", None, "nemesis", "start"))
    got = independent.checker(checker.unique_ids()).check({}, h, {})
    assert got["valid?"] is False and sorted(got["failures"]) == ["a", "c"]
    for k, sub in independent.subhistories(h).items():
        same(got["results"][k], ref_ops(sub))
    assert got["results"]["a"]["duplicated"] == {2: 2} and got["results"]["c"]["duplicated"] == {None: 2}


SEEDED = [(0, "counter", [(5, 2), (2, 7), (60, 2)], 0), (1, "flake", [(5, 2), (2, 7), (60, 2)], 3),
          (2, "counter", (), 0), (3, "flake", (), 1), (4, "string", [(3, 2), (1, 4)], 2)]


@pytest.mark.parametrize("seed,kind,dups,nil_acks", SEEDED)
def test_seeded_vs_numpy(ctx, seed, kind, dups, nil_acks):
    cols = synth.unique_ids_history(200_000, kind=kind, dups=dups, nil_acks=nil_acks, seed=seed)
    want = ref_cols(cols)
    assert want["duplicated-count"] == sum(h for h, _ in dups) + (nil_acks >= 2)
    for path in PATHS:
        if kind == "flake" and path == 1:                 # 63-bit ids span more than 2^35: the dense path refuses
            with pytest.raises(_native.JhError) as e:
                run(cols, path)
            assert e.value.code == A.JH_EINVAL
            continue
        got, took = run(cols, path)
        assert took == path
        same(got, want)


@pytest.mark.parametrize("path,kind", [(1, "counter"), (2, "flake")])
def test_two_million_rows(ctx, path, kind):
    """Every grid-stride and hipcub tile boundary: 2 M rows (the packed host
    staging path as well)."""
    cols = synth.unique_ids_history(888_889, kind=kind, dups=[(7, 2), (1, 9)], nil_acks=2, seed=8)
    assert cols.n >= 2_000_000
    got, took = run(cols, path)
    assert took == path
    same(got, ref_cols(cols))
