"""jepsen.tests.bank/checker on the device (jh_check_bank, jh_bank.hip) against
the CPU restatements of tests/bank_ref.py: whole result maps through
bank.checker, and the raw result and [row, total, class] triples of the C
entry point. The reference tree has no bank test: parity is unpinned against
the reference's own tests."""
import numpy as np
import pytest

from bank_cases import CASES, RAISING, T
from bank_ref import points_ref, ref_cols, ref_ops, rows_of
from jepsen_amd import _abi as A
from jepsen_amd import _native, bank, checker, synth
from jepsen_amd.history import Columns

pytestmark = pytest.mark.gpu

NIL = A.NIL
I64_MAX = (1 << 63) - 1
TOTAL = 100


def raw_rows(r):
    """The C result in the shape of ref_cols' map."""
    errors = {}
    for name, e in zip(A.BANK_TYPES, r["errors"]):
        if e["count"]:
            m = {"count": e["count"], "first": e["first_row"], "worst": e["worst_row"], "last": e["last_row"]}
            if name == "wrong-total":
                m["lowest"], m["highest"] = e["lowest_row"], e["highest_row"]
            else:
                assert (e["lowest_row"], e["highest_row"]) == (-1, -1)
            errors[name] = m
        else:
            assert (e["first_row"], e["last_row"], e["worst_row"], e["lowest_row"], e["highest_row"]) == (-1,) * 5
    return {"valid?": r["valid"] == A.VALID, "read-count": r["read_count"], "error-count": r["error_count"],
            "first-error": None if r["first_error_row"] < 0 else r["first_error_row"], "errors": errors}


def agree(ctx, cols, n_acc, total=TOTAL, negb=False, want=None):
    """The raw call against ref_cols: the whole result and every triple.
    Returns (raw result, ref_cols map)."""
    want = dict(ref_cols(cols, n_acc, total, negb, exact=True) if want is None else want)
    tri = want.pop("triples")
    r = ctx.check_bank(cols, n_acc, total, negb)
    assert r["n_reads"] == len(tri) == len(r["reads"]) and r["entries"] == int(cols.value2[bank.is_read(cols)].sum())
    bad = np.nonzero((r["reads"] != tri).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5], r["reads"][bad[:5]], tri[bad[:5]])
    if "raises" in want:
        assert (r["valid"], r["cause"]) == (A.UNKNOWN, 7)
    else:
        assert raw_rows(r) == want
        assert r["cause"] == 0
    return r, want


def build(sizes, plant=(), order=None, gap=0, odd=False, nil_value=(), total=TOTAL):
    """Columns of len(sizes) reads (an :invoke row and the :ok :read row each;
    odd: one nemesis row first, so the history has an odd length and ends in a
    read). A read of size s holds accounts 0..s-1, the first balance `total`,
    the others 0. plant: (read, kind, pair) -- kind "u" an unexpected key, "n"
    a nil, "w" a wrong total, "-" a negative balance made up for by the next
    pair. order: the reads' ranges lie in aux in this order of reads, `gap`
    poisoned pairs between them. nil_value: reads whose :value is nil."""
    sizes = np.asarray(sizes, np.int64)
    K = len(sizes)
    off = np.zeros(K + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    E = int(off[K])
    rid = np.repeat(np.arange(K, dtype=np.int64), sizes)
    code = np.arange(E, dtype=np.int64) - off[rid]
    bal = np.zeros(E, np.int64)
    bal[off[:-1][sizes > 0]] = total
    for t, (r, kind, j) in enumerate(plant):
        s, at = int(sizes[r]), int(off[r] + j)
        assert 0 <= j < s
        if kind == "u":
            code[at] = 1 << 40
        elif kind == "n":
            bal[at] = NIL
        elif kind == "w":
            bal[at] += 3 + t % 5
        else:
            assert s >= 2
            d = total + 1 + t % 7
            bal[at] -= d
            bal[off[r] + (j + 1) % s] += d
    order = np.arange(K) if order is None else np.asarray(order)
    pos = np.zeros(K, np.int64)                              # first pair of each read in aux
    pos[order] = np.concatenate([[0], np.cumsum(sizes[order] + gap)[:-1]])
    half = int(sizes.sum() + gap * K)
    aux = np.empty(2 * half, np.int64)
    aux[0::2], aux[1::2] = -7, NIL                            # poison: an unexpected key and a nil
    dst = pos[rid] + (np.arange(E, dtype=np.int64) - off[rid])
    aux[2 * dst], aux[2 * dst + 1] = code, bal
    n = 2 * K + (1 if odd else 0)
    typ = np.tile(np.asarray([A.TYPE_INVOKE, A.TYPE_OK], np.int64), K)
    val = np.full(2 * K, NIL, np.int64)
    val2 = np.full(2 * K, NIL, np.int64)
    val[1::2], val2[1::2] = pos, sizes
    nv = np.asarray(list(nil_value), np.int64)
    val[2 * nv + 1], val2[2 * nv + 1] = NIL, 0
    proc = np.repeat(np.arange(K, dtype=np.int64) % 5, 2)
    fc = np.zeros(2 * K, np.int64)
    if odd:
        typ, val, val2 = (np.concatenate([[x], a]) for x, a in ((A.TYPE_INFO, typ), (NIL, val), (NIL, val2)))
        proc, fc = np.concatenate([[-1], proc]), np.concatenate([[16], fc])
    return Columns(n=n, process=proc, type=typ, f=fc, key=np.full(n, -1, np.int64), value=val, value2=val2,
                   n_keys=0, aux=aux, f_names=["start"], value_table=list(range(int(max(sizes.max(), 1)))))


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_hand_cases(ctx, name):
    test, opts, h, want = CASES[name]
    got = bank.checker(opts).check(test, h, {})
    assert got == want
    assert list(got["errors"]) == list(ref_ops(test, h, bool(opts.get("negative-balances?")))["errors"])
    cols, table = bank.encode(h, test["accounts"])
    assert rows_of(bank.checker(opts).check(test, cols, {})) == rows_of(want)      # from the Columns: the same map
    agree(ctx, cols, len(set(test["accounts"])), test["total-amount"], bool(opts.get("negative-balances?")))


def test_float_tie_c_result_is_exact_order(ctx):
    test, opts, h, want = CASES["float-tie-long"]
    cols, _ = bank.encode(h, test["accounts"])
    r = ctx.check_bank(cols, 3, test["total-amount"])
    e = r["errors"][2]
    assert (e["worst_row"], e["worst_badness"]) == (3, (1 << 24) + 1)      # the mirror re-ranks: row 1
    assert rows_of(want)["errors"]["wrong-total"]["worst"] == 1


@pytest.mark.parametrize("name", list(RAISING))
def test_raising_cases_and_check_safe(ctx, name):
    test, opts, h = RAISING[name]
    with pytest.raises(ArithmeticError):
        bank.checker(opts).check(test, h, {})
    r = checker.check_safe(bank.checker(opts), test, h, {})
    assert r["valid?"] == "unknown" and "ArithmeticError" in r["error"]
    r = checker.compose({"SI": bank.checker(opts)}).check(test, h, {})
    assert r["valid?"] == "unknown"


SWEEP = [0, 1, 2, 63, 64, 65] + [64 * k + d for k in range(2, 129, 2) for d in (-1, 0, 1)]


@pytest.mark.parametrize("lead", [0, 1, 63, 66])
def test_read_size_sweep(ctx, lead):
    """A read boundary on every wave-span and tile edge: after a leading read
    of `lead` pairs, reads of every size of SWEEP, each size with every error
    type planted in the first, a middle and the last pair, and a clean read."""
    sizes, plant = [lead], []
    for s in SWEEP:
        for kind in "unw-":
            for j in sorted({0, s // 2, s - 1}) if s else [0]:
                if s == 0 or (kind == "-" and s < 2):
                    continue
                plant.append((len(sizes), kind, j))
                sizes.append(s)
        sizes.append(s)
    cols = build(sizes, plant)
    r, want = agree(ctx, cols, int(max(sizes)))
    assert set(want["errors"]) == set(A.BANK_TYPES) and r["entries"] > 9_000_000
    test = {"accounts": range(int(max(sizes))), "total-amount": TOTAL}
    assert rows_of(bank.checker().check(test, cols, {})) == want
    agree(ctx, cols, int(max(sizes)), negb=True)


@pytest.mark.parametrize("lead", [0, 5, 1000])
def test_runs_of_empty_reads(ctx, lead):
    """200 empty reads (nil :value and the empty map) at the start, across
    wave-step, span and tile edges, and at the end of the history."""
    sizes, nilv = [], []
    for s in (lead, 58, 6, 1024 - 64, 64, 2048 - 7, 7, 4096, 1):
        sizes += [0] * 200
        nilv += list(range(len(sizes) - 200, len(sizes), 2))
        sizes.append(s)
    sizes += [0] * 200
    cols = build(sizes, [(len(sizes) - 201, "n", 0)], nil_value=nilv)
    r, want = agree(ctx, cols, 4096)
    assert want["errors"]["wrong-total"]["count"] == 2000 + (lead == 0)
    agree(ctx, cols, 4096, total=0)                          # an empty read is then no error
    assert agree(ctx, build([0] * 130, nil_value=range(0, 130, 3)), 1, total=0)[0]["valid"] == A.VALID


@pytest.mark.parametrize("kind", ["n", "u"])
def test_long_reads(ctx, kind):
    """Reads of 10 000 and 300 000 pairs (many waves, many blocks of partial
    sums), the single nil / unexpected key in the last pair."""
    sizes = [3, 10_000, 8, 300_000, 8, 10_000, 1]
    cols = build(sizes, [(1, kind, 9_999), (3, kind, 299_999), (5, "w", 5_000)])
    r, want = agree(ctx, cols, 300_000)
    name = {"n": "nil-balance", "u": "unexpected-key"}[kind]
    assert want["errors"][name] == {"count": 2, "first": 3, "worst": 3, "last": 7}
    assert want["errors"]["wrong-total"]["count"] == 1 and r["error_count"] == 3


def test_odd_length_history_ends_in_a_read(ctx):
    for sizes in ([3], [8] * 2047 + [5], [8] * 2048 + [5]):     # 4097 rows: the last row alone in its tile
        cols = build(sizes, [(len(sizes) - 1, "w", 0)], odd=True)
        assert cols.n % 2 == 1
        r, want = agree(ctx, cols, 8)
        assert want["first-error"] == cols.n - 1 and r["error_count"] == 1


def test_permuted_and_gapped_ranges(ctx):
    rng = np.random.default_rng(3)
    sizes = rng.integers(0, 200, 3000)
    sizes[[7, 1500]] = 5000
    plant = [(r, "unw-"[r % 4], 0) for r in range(0, 3000, 17) if sizes[r] >= 2]
    for order, gap in ((np.arange(3000)[::-1], 0), (rng.permutation(3000), 3), (np.arange(3000), 1)):
        cols = build(sizes, plant, order=order, gap=gap)
        r, want = agree(ctx, cols, 5000)
        assert r["error_count"] >= len(plant) - 1
    # overlapping ranges are legal too: every read sees the same pairs
    cols = build([8] * 50, [(0, "w", 3)])
    cols.value[1::2] = 0
    assert agree(ctx, cols, 8)[0]["error_count"] == 50


def test_malformed_ranges_are_einval(ctx):
    def bad(mut):
        cols = build([4, 4, 4])
        mut(cols)
        with pytest.raises(_native.JhError) as e:
            ctx.check_bank(cols, 8, TOTAL)
        assert e.value.code == A.JH_EINVAL
    bad(lambda c: c.value.__setitem__(5, 9))                 # 9 + 4 > 12 pairs
    bad(lambda c: c.value.__setitem__(3, 13))
    bad(lambda c: c.value.__setitem__(3, -1))
    bad(lambda c: c.value2.__setitem__(1, -2))
    bad(lambda c: c.value2.__setitem__(1, 1 << 62))
    bad(lambda c: setattr(c, "aux", c.aux[:-1]))             # odd n_aux
    cols = build([4, 4, 4])
    cols.value[0], cols.value2[0] = 99, -5                   # an :invoke row: never read
    cols.value[5], cols.value2[5] = 12, 0                    # an empty range at the very end
    agree(ctx, cols, 8)


def overflow_cols(balances_of, pad=0):
    """One read per list of balances (then `pad` zero balances), accounts in
    order."""
    sizes = [len(b) + pad for b in balances_of]
    cols = build(sizes, total=0)
    at = 0
    for b, s in zip(balances_of, sizes):
        cols.aux[2 * at + 1:2 * (at + len(b)) + 1:2] = np.asarray(b, np.int64)
        at += s
    return cols


@pytest.mark.parametrize("pad", [0, 9_997])
def test_overflow_depends_on_the_order(ctx, pad):
    """[MAX, 1, -1] overflows at its second prefix, [MAX, -1, 1] (the same
    multiset) never does; as short reads and inside reads of 10 000 pairs."""
    ok = overflow_cols([[I64_MAX, -1, 1], [5, -5], [-I64_MAX, -1, 1]], pad)
    r, want = agree(ctx, ok, 20_000, total=0, negb=True)
    assert r["reads"][:, 1].tolist() == [I64_MAX, 0, -I64_MAX] and r["reads"][:, 2].tolist() == [3, 0, 3]
    for balances in ([I64_MAX, 1, -1], [-I64_MAX, -2, 5], [I64_MAX, I64_MAX, -I64_MAX, -I64_MAX]):
        cols = overflow_cols([[1, 2], balances, [3]], pad)
        r, want = agree(ctx, cols, 20_000, total=3, negb=True)
        assert want["raises"] is ArithmeticError
        assert r["reads"][:, 1].tolist() == [3, NIL, 3] and r["reads"][:, 2].tolist() == [0, 8, 0]
        test = {"accounts": range(20_000), "total-amount": 3}
        with pytest.raises(ArithmeticError):
            bank.checker({"negative-balances?": True}).check(test, cols, {})
    # beside a nil or an unexpected key the overflow is not this checker's error
    cols = overflow_cols([[I64_MAX, 1, NIL], [I64_MAX, I64_MAX, 7], [3]], pad)
    cols.aux[2 * (3 + pad) + 4] = 1 << 50                     # the 7's account
    r, want = agree(ctx, cols, 20_000, total=3)
    assert r["valid"] == A.INVALID and r["reads"][:, 2].tolist() == [2 + 8, 1 + 8, 0]
    assert r["reads"][:, 1].tolist() == [NIL, NIL, 3]


def test_host_device_and_multi_device_contexts_agree(ctx):
    from hipcols import DevCols
    cols = synth.bank_history(30_001, unexpected=[5, 900], nils=[17], wrong=[3, 4000, 4001], negative=[77],
                              read_sizes=[2, 8, 8, 8], nil_values=[30, 31], seed=4)
    host, want = agree(ctx, cols, 8)
    mctx = _native.Context(n_gpus=1)
    try:
        for shift in (0, 1):                                 # 16-byte aligned columns, and 8-byte aligned only
            d = DevCols(cols, shift)
            for other in (ctx.check_bank(d, 8, TOTAL, on_device=True), mctx.check_bank(cols, 8, TOTAL)):
                for k, v in host.items():
                    if k == "reads":
                        assert (other[k] == v).all()
                    elif k != "device_ms":
                        assert other[k] == v, k
    finally:
        mctx.close()


def test_reads_cap_and_arguments(ctx):
    cols = synth.bank_history(2000, wrong=[10], seed=6)
    full = ctx.check_bank(cols, 8, TOTAL)
    for cap in (0, 7):
        r = ctx.check_bank(cols, 8, TOTAL, reads_cap=cap)
        assert r["n_reads"] == full["n_reads"] > 500 and len(r["reads"]) == cap
        assert (r["reads"] == full["reads"][:cap]).all() and r["errors"] == full["errors"]
    with pytest.raises(_native.JhError) as e:
        ctx.check_bank(cols, -1, TOTAL)
    assert e.value.code == A.JH_EINVAL
    none = Columns(n=3, process=np.zeros(3, np.int64), type=np.zeros(3, np.int64), f=np.zeros(3, np.int64),
                   key=np.full(3, -1, np.int64), value=np.full(3, NIL, np.int64), value2=np.full(3, NIL, np.int64),
                   n_keys=0, aux=np.zeros(0, np.int64))
    r = ctx.check_bank(none, 8, TOTAL)
    assert (r["valid"], r["read_count"], r["n_reads"], r["first_error_row"]) == (A.VALID, 0, 0, -1)


SYNTH = [(200_000, dict(seed=0, unexpected=[3, 40_000], nils=[5, 6, 7], wrong=[9, 40_001, 40_002], negative=[11, 12])),
         (200_000, dict(seed=1, n_accounts=1024, p_read=0.05, read_sizes=[1024, 1000, 2], wrong=[1, 2], nils=[3])),
         (1_100_000, dict(seed=2, unexpected=[250_000], wrong=[7, 500_000], nil_values=[100, 400_000]))]


@pytest.mark.parametrize("n_ops,kw", SYNTH)
def test_synth_histories(ctx, n_ops, kw):
    """200 000-row histories, and 2.2 M rows: past the packed host staging
    path at 2 M rows, with every grid-stride boundary."""
    cols = synth.bank_history(n_ops // 2 if n_ops == 200_000 else n_ops, **kw)
    assert cols.n >= (2_200_000 if n_ops > 200_000 else 200_000)
    na = kw.get("n_accounts", 8)
    r, want = agree(ctx, cols, na)
    assert r["error_count"] >= sum(len(kw.get(k, ())) for k in ("unexpected", "nils", "wrong", "negative"))
    test = {"accounts": range(na), "total-amount": TOTAL}
    assert rows_of(bank.checker().check(test, cols, {})) == want


def test_points(ctx):
    h = [dict(op, time=1_500_000_000 * i) for i, op in enumerate(CASES["first-error"][2] + CASES["valid"][2])]
    assert bank.points(T, h) == points_ref(T, h)
    assert bank.points(T, [op for op in h if op["type"] != "ok"]) is None
    cols = synth.bank_history(3000, nils=[4], unexpected=[9], seed=9)
    ops = synth.bank_columns_to_ops(cols)
    test = {"accounts": range(8), "total-amount": TOTAL, "nodes": ["a", "b", "c"]}
    assert bank.points(test, cols) == points_ref(test, ops)
    r = bank.test()["checker"].check(dict(bank.test(), nodes=["a"]), ops, {})
    assert r["valid?"] is False and r["plot"] == {"valid?": True} and r["SI"]["error-count"] == 2
