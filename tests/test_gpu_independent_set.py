"""jh_check_set_independent on the device against the closed form (ref_cols,
tests/independent_set_ref.py) field by field -- the result, every key record,
all four bitmaps -- on the auto, on-chip and global paths, and the checker's
maps against the transcription of the two Clojure functions (clj_check) and
against the per-key path. Everything is integer: every comparison is exact."""
import numpy as np
import pytest

from jepsen_amd import _abi as A
from jepsen_amd import _native, checker, independent, synth
from jepsen_amd import history as H
from jepsen_amd.history import Columns, tuple_
from independent_set_cases import CASES, I64_MAX, I64_MIN, UNKEYED, added, ia, ir, keyed, na, nem, oa, rd
from independent_set_ref import COUNTS, clj_check, ref_cols, same_raw

pytestmark = pytest.mark.gpu
PATHS = (0, 1, 2)
POISON = I64_MAX - 12345


def agree(ctx, cols, paths=PATHS):
    """The raw call equals ref_cols on every path, return code included. Returns the auto path's answer."""
    for path in paths:
        want = ref_cols(cols, path)
        if want["rc"] != A.JH_OK:
            with pytest.raises(_native.JhError) as e:
                ctx.check_set_independent(cols, path=path)
            assert e.value.code == want["rc"], path
        else:
            same_raw(want, ctx.check_set_independent(cols, path=path), f"path {path}")
    return ref_cols(cols, paths[0])


def maps_agree(h):
    got = independent.checker(checker.set()).check({}, h, {})
    assert got == clj_check(h)
    assert got["results"] == independent.check_per_key(checker.set(), {}, h)
    return got


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


def with_cols(cols, **kw):
    return Columns(**{**cols.__dict__, **kw})


@pytest.mark.parametrize("name", list(CASES))
def test_hand_written_cases(ctx, name):
    h = CASES[name]
    agree(ctx, H.encode(h, keyed=True))
    maps_agree(h)


def edge_keys(span):
    """full: every element of [0, span) attempted and read, the top one
    recovered, so its sets reach the last bit the span has (bit 31 of its last
    word when span is a multiple of 32). lossy: the same span with element 0
    acknowledged and not read."""
    full = added(range(span - 1)) + [ia(span - 1), na(span - 1), ir(), rd(set(range(span)))]
    lossy = added(range(span)) + [ir(), rd(set(range(1, span)))]
    return full, lossy


@pytest.mark.parametrize("span", [1, 31, 32, 33, 63, 64, 65])
def test_word_and_segment_edges(ctx, span):
    """Neighbours in word_off order: no bit of one key bleeds into the other's words."""
    full, lossy = edge_keys(span)
    for subs in ({"full": full, "lossy": lossy}, {"lossy": lossy, "full": full}):
        h = keyed(subs)
        cols = H.encode(h, keyed=True)
        want = agree(ctx, cols)
        assert want["keys"]["n_words"].tolist() == [(span + 31) // 32] * 2 and want["total_words"] == 2 * ((span + 31) // 32)
        lk = cols.keys.index("lossy")
        assert want["keys"]["lost_count"].tolist() == [1 if k == lk else 0 for k in range(2)]
        assert want["bits"][1][int(want["keys"]["word_off"][lk])] == 1          # element 0 of the lossy key, nothing else
        assert sum(bin(int(w)).count("1") for w in want["bits"][1]) == 1
        got = maps_agree(h)
        assert got["failures"] == ["lossy"]


def spanning(span, lose_top=False):
    """A key whose elements span exactly `span`: 0 and span - 1."""
    return added([0, span - 1]) + [ir(), rd({0} if lose_top else {0, span - 1})]


def test_tier_edge(ctx):
    L = A.SI_LDS_SPAN
    three = keyed({"under": spanning(L - 1), "at": spanning(L, lose_top=True), "over": spanning(L + 1, lose_top=True)})
    cols = H.encode(three, keyed=True)
    want = agree(ctx, cols, paths=(0, 2))
    assert want["path"] == 2 and want["keys"]["n_words"].tolist() == [L // 32, L // 32, L // 32 + 1]
    assert want["keys"]["valid"].tolist() == [A.VALID, A.INVALID, A.INVALID]
    with pytest.raises(_native.JhError) as e:
        ctx.check_set_independent(cols, path=1)
    assert e.value.code == A.JH_EINVAL and ref_cols(cols, 1)["rc"] == A.JH_EINVAL
    two = H.encode(keyed({"under": spanning(L - 1), "at": spanning(L, lose_top=True)}), keyed=True)
    want = agree(ctx, two)
    assert want["path"] == 1
    assert maps_agree(three)["failures"] == ["at", "over"]


def test_aux_layout(ctx):
    """The reads' ranges anywhere in aux, in any order, with foreign elements between them."""
    for name in ("all", "extremes", "base-not-word-aligned"):
        cols = H.encode(CASES[name], keyed=True)
        want = agree(ctx, cols)
        moved = agree(ctx, relayout(cols))
        same_raw(want, moved, name)


def test_empty_history(ctx):
    cols = H.encode([], keyed=True)
    want = agree(ctx, cols)
    assert want["path"] == 0 and want["total_words"] == 0 and want["valid"] == A.VALID
    assert independent.checker(checker.set()).check({}, [], {}) == {"valid?": True, "results": {}, "failures": []}


@pytest.mark.parametrize("name", list(UNKEYED))
def test_unkeyed_forms_equal_check_set_bitmaps(ctx, name):
    """key == NULL, and n_keys = 1 with every key 0: key 0's record and bits are jh_check_set_bitmaps'."""
    cols = H.encode(UNKEYED[name], keyed=False)
    one = ctx.check_set_bitmaps(cols)
    forms = (with_cols(cols, key=None, n_keys=0), with_cols(cols, key=np.zeros(cols.n, np.int64), n_keys=1),
             with_cols(cols, n_keys=0))
    for form in forms:
        want = agree(ctx, form)
        rec = want["keys"][0]
        for k in ("valid", "cause", "first_fail_entry", "final_read_entry") + COUNTS:
            assert int(rec[k]) == int(one[k]), k
        assert (int(rec["base"]), int(rec["n_words"]), int(rec["rows"])) == (one["base"], one["n_words"], cols.n)
        got = ctx.check_set_independent(form)
        for i in range(4):
            assert np.array_equal(got["bits"][i], one["bits"][i])


def test_keys_in_no_row(ctx):
    cols = H.encode(CASES["lost"], keyed=True)
    more = with_cols(cols, n_keys=cols.n_keys + 3, keys=cols.keys + ["x", "y", "z"])
    want = agree(ctx, more)
    assert want["keys"]["rows"][-3:].tolist() == [0, 0, 0] and want["keys"]["n_words"][-3:].tolist() == [0, 0, 0]
    assert want["keys_valid"] + want["keys_invalid"] + want["keys_unknown"] == cols.n_keys
    # a key id in the middle that no row carries
    gap = with_cols(cols, key=np.where(cols.key >= 1, cols.key + 1, cols.key), n_keys=cols.n_keys + 1)
    want = agree(ctx, gap)
    assert want["keys"]["rows"][1] == 0


def test_words_cap(ctx):
    cols = H.encode(CASES["all"], keyed=True)
    want = ref_cols(cols)
    total = want["total_words"]
    assert total > 8
    for cap in (0, 1, total - 1, total, total + 5):
        for path in PATHS:
            got = ctx.check_set_independent(cols, path=path, words_cap=cap)
            assert got["total_words"] == total
            for name in A.SET_KEY_DTYPE.names:
                assert got["keys"][name].tolist() == want["keys"][name].tolist(), name
            for i in range(4):
                assert np.array_equal(got["bits"][i], want["bits"][i][:cap])


BASE = keyed({"a": added([1, 2]) + [ir(), rd({1, 2})], "b": added([5]) + [ir(), rd({4})]})


@pytest.mark.parametrize("extra", [rd({1}), ia(7), oa(7), dict(ia(None), value=tuple_("a", None))],
                         ids=["unkeyed-ok-read", "unkeyed-invoke-add", "unkeyed-ok-add", "nil-add"])
def test_unsupported_histories_fall_back(ctx, extra):
    h = BASE + [extra]
    cols = H.encode(h, keyed=True)
    for path in PATHS:
        with pytest.raises(_native.JhError) as e:
            ctx.check_set_independent(cols, path=path)
        assert e.value.code == A.JH_EUNSUPPORTED == ref_cols(cols, path)["rc"]
    got = independent.checker(checker.set()).check({}, h, {})
    assert got["results"] == independent.check_per_key(checker.set(), {}, h)
    maps_agree(BASE)


def test_span_refusal_and_invalid_columns(ctx):
    huge = keyed({"a": added([0, A.SI_SPAN_MAX]) + [ir(), rd({0})], "b": added([5]) + [ir(), rd({5})]})
    assert agree(ctx, H.encode(huge, keyed=True))["rc"] == A.JH_EUNSUPPORTED
    got = independent.checker(checker.set()).check({}, huge, {})
    assert got["results"] == independent.check_per_key(checker.set(), {}, huge)
    assert got["results"]["b"]["valid?"] is True and got["results"]["a"]["valid?"] == "unknown"
    cols = H.encode(BASE, keyed=True)
    assert agree(ctx, with_cols(cols, key=np.where(cols.key == 1, 2, cols.key)))["rc"] == A.JH_EINVAL
    last = int(np.nonzero((cols.type == A.TYPE_OK) & (cols.f == A.F_READ))[0][-1])
    for v, c in ((len(cols.aux), 1), (0, len(cols.aux) + 1), (-1, 1), (0, -1), (I64_MAX, 2)):
        val, val2 = cols.value.copy(), cols.value2.copy()
        val[last], val2[last] = v, c
        assert agree(ctx, with_cols(cols, value=val, value2=val2))["rc"] == A.JH_EINVAL
    with pytest.raises(_native.JhError) as e:
        ctx.check_set_independent(cols, path=3)
    assert e.value.code == A.JH_EINVAL
    maps_agree(BASE)


def test_seeded_random(ctx):
    for kw in (dict(n_keys=64, adds_per_key=99, n_lost_keys=9, n_unexpected_keys=7, p_fail=0.1, p_info=0.1, seed=5),
               dict(n_keys=2000, adds_per_key=3, n_lost_keys=100, n_unexpected_keys=100, p_fail=0.1, p_info=0.2, seed=6)):
        cols = synth.independent_set_history(**kw)
        want = agree(ctx, cols)
        assert want["keys_invalid"] > 0 and want["keys_valid"] > 0
        h = synth.independent_set_columns_to_ops(cols)
        got = independent.checker(checker.set()).check({}, h, {})
        assert got == clj_check(h)


def test_context_reuse(ctx):
    """No stale workspace bits: a wide key, then a narrow one at the same
    word_off, and each call twice with another history in between."""
    wide = H.encode(keyed({"a": added(range(0, 3000, 7)) + [ir(), rd(set(range(0, 3000, 7)) | {2999})],
                           "b": added(range(40)) + [ir(), rd(set(range(40)))]}), keyed=True)
    narrow = H.encode(keyed({"a": added([5]) + [ir(), rd(set())], "b": added(range(100, 140)) + [ir(), rd({100})]}),
                      keyed=True)
    other = synth.independent_set_history(n_keys=32, adds_per_key=50, n_lost_keys=4, n_unexpected_keys=4, seed=9)
    for path in PATHS:
        first = ctx.check_set_independent(wide, path=path)
        same_raw(ref_cols(wide, path), first)
        same_raw(ref_cols(narrow, path), ctx.check_set_independent(narrow, path=path))
        same_raw(ref_cols(other, path), ctx.check_set_independent(other, path=path))
        same_raw(first, ctx.check_set_independent(wide, path=path))
        same_raw(ref_cols(narrow, path), ctx.check_set_independent(narrow, path=path))
