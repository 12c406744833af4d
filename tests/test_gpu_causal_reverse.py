"""jepsen.tests.causal-reverse on the device (jh_check_causal_reverse,
jh_causal.hip) against the CPU restatements of tests/causal_reverse_ref.py: the
raw result, every error row and every missing value of the C entry point
against the numpy restatement ref_cols, and the checker's maps against the
literal transcription of the Clojure loop. Every case runs on both forced tiers
and on auto; everything is integer, so every comparison is exact.

JH_EUNSUPPORTED for more than 2^31 - 2 reads or writes is reached with device
columns that alias one 16 GiB buffer of ones (test_count_limits)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLD
from jepsen_amd import _abi as A
from jepsen_amd import _native, checker, independent, synth
from jepsen_amd import causal_reverse as CR
from jepsen_amd.history import Columns, tuple_
from causal_reverse_cases import CASES, I64_MAX, I64_MIN, QUIRK_AS_SETS, edge, rd, ri, seq, wi, wo
from causal_reverse_ref import RAW_FIELDS, clj_check, ref_cols

pytestmark = pytest.mark.gpu

PATHS = (A.CR_PATH_AUTO, A.CR_PATH_LDS, A.CR_PATH_GLOBAL)
POISON = 4242                    # between the reads' ranges: a value some key writes


def agree(ctx, cols, paths=PATHS, caps=None):
    """The raw call on every path against ref_cols: every field, key_valid,
    every error row and every missing value. Returns ref_cols' answer on auto."""
    first = None
    for path in paths:
        want = ref_cols(cols, path)
        assert want["rc"] == A.JH_OK
        ecap, mcap = caps or (max(want["error_count"], 1), max(want["missing_total"], 1))
        r = ctx.check_causal_reverse(cols, path, ecap, mcap)
        assert {k: r[k] for k in RAW_FIELDS} == {k: want[k] for k in RAW_FIELDS}, path
        assert r["key_valid"].tolist() == want["key_valid"].tolist(), path
        assert r["errors"].tolist() == want["errors"][:ecap].tolist(), path
        assert r["missing"].tolist() == want["missing"][:mcap].tolist(), path
        first = first or want
    return first


def maps_agree(h):
    """The checker's map on every path against the Clojure loop over sets."""
    want = clj_check(h, as_sets=True)
    for path in PATHS:
        assert CR.checker(vectors_as_sets=True, path=path).check({}, h, {}) == want, path
    return want


def relayout(cols, gap=3):
    """The same history with the reads' ranges in aux in reversed order of
    reads and `gap` poisoned elements in front of each."""
    val, aux = cols.value.copy(), []
    reads = [i for i in range(cols.n) if cols.type[i] == A.TYPE_OK and cols.f[i] == A.F_READ and cols.value2[i] > 0]
    for i in reversed(reads):
        aux += [POISON] * gap
        val[i] = len(aux)
        aux += cols.aux[cols.value[i]:cols.value[i] + cols.value2[i]].tolist()
    aux += [POISON] * gap
    return Columns(n=cols.n, process=cols.process, type=cols.type, f=cols.f, key=cols.key, value=val, value2=cols.value2,
                   n_keys=cols.n_keys, aux=np.asarray(aux, np.int64), keys=cols.keys)


def keyed(subs):
    """{key: ops} -> one history, the keys interleaved row by row."""
    out = []
    for i in range(max(len(s) for s in subs.values())):
        for k, s in subs.items():
            if i < len(s):
                out.append(dict(s[i], value=tuple_(k, s[i]["value"])))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_hand_written_cases(ctx, name):
    h = CASES[name]
    agree(ctx, CR.encode(h))
    maps_agree(h)
    if name == "vector-quirk":
        assert maps_agree(h) == QUIRK_AS_SETS
    if name == "repeated-element":
        r = ctx.check_causal_reverse(CR.encode(h), 0, 4, 4)
        assert r["errors"].tolist() == [[6, 0, 2, 1, 0]] and r["missing"].tolist() == [2]


def test_empty_and_unkeyed_forms(ctx):
    e = CR.encode([])
    for path in PATHS:
        r = ctx.check_causal_reverse(e, path, 1, 1)
        assert {k: r[k] for k in RAW_FIELDS} == {k: ref_cols(e)[k] for k in RAW_FIELDS} and r["path"] == 0
    # key == NULL, and the same rows as key 0 of n_keys = 1
    h = CASES["invoked-twice-with-another"] + CASES["extreme-values"]
    c0 = CR.encode(h)
    none = Columns(n=c0.n, process=c0.process, type=c0.type, f=c0.f, key=None, value=c0.value, value2=c0.value2,
                   n_keys=0, aux=c0.aux)
    one = CR.encode([dict(o, value=tuple_("k", o["value"])) for o in h], keyed=True)
    assert one.n_keys == 1 and (one.key == 0).all()
    a, b, c = agree(ctx, c0), agree(ctx, none), agree(ctx, one)
    assert a["error_count"] > 0
    for k in RAW_FIELDS + ("errors", "missing", "key_valid"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k])


def test_golden_histories(ctx):
    for case in json.load(open(os.path.join(GOLD, "causal_reverse.json")))["cases"]:
        h, want = case["history"], case["valid?"]
        assert CR.checker().check({}, h, {})["valid?"] is want                    # vectors: the host
        assert maps_agree(h)["valid?"] is want                                     # as sets: both tiers and auto
        agree(ctx, CR.encode(h))


@pytest.mark.parametrize("c", [31, 32, 33, 63, 64, 65, 255, 256, 257])
def test_bitmap_and_wave_edges(ctx, c):
    """expected_count = c with the single missing value at rank 0 and at rank
    c - 1; reads of c and of c + 1 elements."""
    for drop in (0, c - 1):
        h = edge(c, drop)
        want = agree(ctx, relayout(CR.encode(h)))
        assert want["errors"][:, 2:4].tolist() == [[c, 1], [c, 1]] and want["missing"].tolist() == [100 + drop] * 2
        assert want["entries"] == 3 * c + 2
        maps_agree(h)


def tile_edge_history(N):
    """N rows of one key. Around the first tile edge E = CR_TILE: a write and an
    :ok read on E - 2 and E - 1, a write and an :ok read on E and E + 1. 3 is
    invoked (E - 2) after 1 and 2 completed, so the read of [3] alone on E + 1
    misses both; the reads on E - 1 and E + 2 are satisfied. A history that
    goes on past the edge ends with the violating read once more."""
    E = A.CR_TILE
    h = [ri() for _ in range(N)]
    h[:4] = seq(1, 2)
    for i, o in ((E - 2, wi(3)), (E - 1, rd([2, 1])), (E, wo(3)), (E + 1, rd([3])), (E + 2, rd([1, 3, 2]))):
        if i < N:
            h[i] = o
    if N > E + 5:
        h[N - 1] = rd([3])
    return h


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_tile_edges(ctx, d):
    """CR_TILE - 1, CR_TILE and CR_TILE + 1 rows (then two tiles more): the
    flagged rows on both sides of a tile edge, and a last tile of one row, of a
    full tile and of a full tile less one row."""
    for extra in (0, 2 * A.CR_TILE):
        N = A.CR_TILE + d + extra
        cols = CR.encode(tile_edge_history(N))
        assert cols.n == N
        for path in PATHS:                                   # the CPU reference takes the history, before any device run
            assert ref_cols(cols, path)["rc"] == A.JH_OK
        want = agree(ctx, cols)
        bad = [i for i in (A.CR_TILE + 1, N - 1) if extra and i < N]
        assert want["errors"][:, 0].tolist() == bad and want["missing"].tolist() == [1, 2] * len(bad)
        assert want["read_count"] == sum(1 for i in (A.CR_TILE - 1, A.CR_TILE + 1, A.CR_TILE + 2) if i < N) + bool(extra)


def big_key(n_values):
    """n_values writes complete in order, then one more; reads of it with all
    but the first, with all but the last, and with everything."""
    vs = list(range(1000, 1000 + n_values - 1))
    return seq(*vs) + seq(7) + [rd(frozenset(vs[1:] + [7])), rd(frozenset(vs[:-1] + [7])), rd(frozenset(vs + [7]))]


def test_tier_boundary(ctx):
    cap = A.CR_LDS_VALUES
    fits, over = CR.encode(big_key(cap)), CR.encode(big_key(cap + 1))
    want = agree(ctx, fits)
    assert want["path"] == 1 and want["errors"][:, 2:4].tolist() == [[cap - 1, 1], [cap - 1, 1]]
    want = agree(ctx, over, paths=(A.CR_PATH_AUTO, A.CR_PATH_GLOBAL))
    assert want["path"] == 2 and want["errors"][:, 2:4].tolist() == [[cap, 1], [cap, 1]]
    assert ref_cols(over, A.CR_PATH_LDS)["rc"] == A.JH_EINVAL
    with pytest.raises(_native.JhError) as e:
        ctx.check_causal_reverse(over, A.CR_PATH_LDS, 4, 4)
    assert e.value.code == A.JH_EINVAL
    # one key on each side in one history: auto judges the small one on chip, the other in the global tier
    both = CR.encode(keyed({"small": big_key(40), "large": big_key(cap + 1), "edge": big_key(cap)}), keyed=True)
    want = agree(ctx, both, paths=(A.CR_PATH_AUTO, A.CR_PATH_GLOBAL))
    assert want["path"] == 2 and want["error_count"] == 6 and want["invalid_keys"] == 3


def test_cross_talk(ctx):
    """Three interleaved keys write and read the same values; one is invalid."""
    good = seq(-1, I64_MAX, I64_MIN + 1) + [rd([-1, I64_MAX, I64_MIN + 1]), rd([-1]), rd([I64_MAX, -1])]
    bad = seq(-1, I64_MAX, I64_MIN + 1) + [rd([I64_MIN + 1]), rd([I64_MAX]), rd([-1])]
    late = [rd([I64_MAX])] + seq(I64_MAX, -1, I64_MIN + 1) + [rd([I64_MAX, I64_MIN + 1, -1])]
    h = keyed({"a": good, "b": bad, "c": late})
    cols = CR.encode(h, keyed=True)
    want = agree(ctx, relayout(cols))
    assert want["key_valid"].tolist() == [A.VALID, A.INVALID, A.VALID] and want["invalid_keys"] == 1
    assert want["errors"][:, 1].tolist() == [1, 1] and want["missing"].tolist() == [-1, I64_MAX, -1]
    for path in PATHS:
        got = independent.checker(CR.checker(vectors_as_sets=True, path=path)).check({}, h, {})
        assert got["failures"] == ["b"]
        assert got["results"] == {k: clj_check(independent.subhistory(k, h), as_sets=True) for k in "abc"}


def test_caps(ctx):
    cols = synth.causal_reverse_history(n_keys=16, ops_per_key=60, violations=12, seed=7)
    full = agree(ctx, cols)
    E, M = full["error_count"], full["missing_total"]
    assert E >= 3 and M >= 3
    for caps in ((1, 1), (E - 1, M - 1), (2, M + 5), (E + 5, 2)):
        agree(ctx, cols, caps=caps)
    for path in PATHS:                       # err_cap = 0: NULL output pointers, totals exact
        r = ctx.check_causal_reverse(cols, path, 0, 0, key_valid=False)
        assert {k: r[k] for k in RAW_FIELDS} == {k: ref_cols(cols, path)[k] for k in RAW_FIELDS}
        assert r["key_valid"] is None and len(r["errors"]) == 0 and len(r["missing"]) == 0


def raw(cols, **over):
    c = Columns(n=cols.n, process=cols.process, type=cols.type, f=cols.f, key=cols.key, value=cols.value.copy(),
                value2=cols.value2.copy(), n_keys=cols.n_keys, aux=cols.aux, keys=cols.keys)
    for name, (i, v) in over.items():
        a = getattr(c, name).copy()
        a[i] = v
        setattr(c, name, a)
    return c


def test_return_codes(ctx):
    h = seq(1, 2, 3) + [rd([3, 2]), rd([1])]
    cols = CR.encode(h)                      # rows 6 and 7 read aux[0:2] and aux[2:3]; n_aux = 3
    kcols = CR.encode([dict(o, value=tuple_("k", o["value"])) for o in h], keyed=True)
    cases = {
        "range past n_aux": (raw(cols, value2=(7, 2)), A.JH_EINVAL),
        "start past n_aux": (raw(cols, value=(7, 4)), A.JH_EINVAL),
        "negative start": (raw(cols, value=(6, -1)), A.JH_EINVAL),
        "negative count": (raw(cols, value2=(6, -2)), A.JH_EINVAL),
        "nil count": (raw(cols, value2=(6, A.NIL)), A.JH_EINVAL),
        "key past n_keys": (raw(kcols, key=(2, 1)), A.JH_EINVAL),
        "keyless invoke write": (raw(kcols, key=(0, -1)), A.JH_EUNSUPPORTED),
        "keyless ok write": (raw(kcols, key=(1, -1)), A.JH_EUNSUPPORTED),
        "keyless ok read": (raw(kcols, key=(7, -1)), A.JH_EUNSUPPORTED),
        "write of nil": (raw(cols, value=(2, A.NIL)), A.JH_EUNSUPPORTED),
    }
    for name, (c, code) in cases.items():
        assert ref_cols(c)["rc"] == code, name
        for path in PATHS:
            with pytest.raises(_native.JhError) as e:
                ctx.check_causal_reverse(c, path, 4, 4)
            assert e.value.code == code, (name, path)
    # harmless: a count of 0 with any value, a range that ends at n_aux, keyless rows of other kinds
    agree(ctx, raw(cols, value=(7, 99), value2=(7, 0)))
    agree(ctx, raw(cols, value=(7, 3), value2=(7, 0)))
    agree(ctx, raw(kcols, key=(0, -1), type=(0, A.TYPE_FAIL)))
    # the mirror answers what the device does not take through check_host
    for name, (c, code) in cases.items():
        if code != A.JH_EUNSUPPORTED:
            continue
        ops = [CR.decode_op(c, i, unwrap=True) for i in range(c.n)]
        for path in PATHS:
            assert CR.checker(path=path).check({}, c, {}) == clj_check(ops, as_sets=True), (name, path)
    hu = [wi(1), wo(1)] + keyed({"a": seq(2) + [rd({2})], "b": seq(2) + [rd({2, 1})]})
    got = independent.checker(CR.checker()).check({}, hu, {})
    assert got["results"] == {k: clj_check(independent.subhistory(k, hu)) for k in "ab"} and got["failures"] == ["a"]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("violations", [0, 5])
def test_random_parity(ctx, seed, violations):
    cols = synth.causal_reverse_history(n_keys=64, ops_per_key=60, violations=violations, seed=seed)
    want = agree(ctx, cols)
    assert (want["error_count"] > 0) == (violations > 0) and want["read_count"] > 64
    agree(ctx, relayout(cols, gap=1), paths=(A.CR_PATH_AUTO,))
    h = CR.decode(cols)
    got = independent.checker(CR.checker(vectors_as_sets=True)).check({}, h, {})
    assert got["results"] == {k: clj_check(independent.subhistory(k, h), as_sets=True) for k in range(64)}


def test_lifting_equals_the_per_key_path(ctx):
    cols = synth.causal_reverse_history(n_keys=16, ops_per_key=60, violations=4, seed=5)
    h = [dict(o, value=tuple_(o["value"].key, frozenset(o["value"].val))) if o["type"] == "ok" and o["f"] == "read"
         and o["value"].val is not None else o for o in CR.decode(cols)]
    inner = CR.checker()
    generic = independent.checker(checker._Fn(lambda t, hh, o: inner.check(t, hh, o))).check({}, h, {})
    for path in PATHS:
        assert independent.checker(CR.checker(path=path)).check({}, h, {}) == generic
    assert generic["valid?"] is False and 1 <= len(generic["failures"]) <= 4
    comp = checker.compose({"sequential": CR.checker(), "optimism": checker.unbridled_optimism()})
    got = independent.checker(comp).check({}, h, {})
    assert got["failures"] == generic["failures"]
    assert all(r["sequential"] == generic["results"][k] for k, r in got["results"].items())


def test_count_limits(ctx):
    """2^31 - 1 :ok writes, and 2^31 - 1 :ok reads: one past what the device
    counts in 32 bits. Every column of the device history is the same buffer of
    ones (type 1 = :ok, f 1 = :write), filled by doubling device copies; for the
    reads f is a zeroed buffer (f 0 = :read, count 1 from value2)."""
    import ctypes as C
    from hipcols import DevCols
    n = (1 << 31) - 1
    seed = DevCols(CR.encode([]), 0)                         # loads the HIP runtime libjh.so uses
    hip = seed._hip
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    ones, zeros = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(ones), 8 * (n + 1)) == 0 and hip.hipMalloc(C.byref(zeros), 8 * (n + 1)) == 0
    try:
        first = np.ones(1 << 17, np.int64)
        assert hip.hipMemcpy(ones.value, first.ctypes.data, first.nbytes, 1) == 0
        have = len(first)
        while have < n + 1:                                  # device-to-device, doubling
            step = min(have, n + 1 - have)
            assert hip.hipMemcpy(ones.value + 8 * have, ones.value, 8 * step, 3) == 0
            have += step
        assert hip.hipMemset(zeros.value, 0, 8 * (n + 1)) == 0

        class Dev:
            pass
        for f_col, what in ((ones.value, "writes"), (zeros.value, "reads")):
            d = Dev()
            d.n, d.n_keys, d.key, d.aux, d.n_aux = n, 0, 0, ones.value, 16
            d.process = d.type = d.value = d.value2 = ones.value
            d.f = f_col
            for path in PATHS:
                with pytest.raises(_native.JhError) as e:
                    ctx.check_causal_reverse(d, path, 4, 4, on_device=True)
                assert e.value.code == A.JH_EUNSUPPORTED and what in e.value.msg, (what, path)
            d.n = 1000                                        # the same columns within the limit: a plain answer
            r = ctx.check_causal_reverse(d, 0, 4, 4, on_device=True)
            assert r["read_count"] == (1000 if what == "reads" else 0) and r["valid"] == A.VALID
    finally:
        hip.hipFree(ones)
        hip.hipFree(zeros)
