"""jepsen.tests.adya/g2-checker on the device (jh_check_g2, jh_g2.hip) against
the CPU restatements of tests/g2_ref.py: the raw result and the illegal pairs
of the C entry point against the numpy restatement ref_cols, and the checker's
maps against the literal transcription of the Clojure reduce. Everything is
integer, so every comparison is exact."""
import numpy as np
import pytest

from jepsen_amd import _abi as A
from jepsen_amd import _native, adya, checker, synth
from jepsen_amd.history import Columns
from g2_cases import CASES, EXPECT, UNKEYED, other, pair
from g2_ref import RAW_FIELDS, clj_check, ref_cols

pytestmark = pytest.mark.gpu

T = A.G2_TILE


def agree(ctx, cols, caps=None):
    """The raw call against ref_cols, every field and every pair, with every
    pair asked for and with the given caps. Returns ref_cols' answer."""
    want = ref_cols(cols)
    assert want["rc"] == A.JH_OK
    for cap in [want["illegal_count"] + 1] + list(caps or ()):
        r = ctx.check_g2(cols, cap)
        assert {k: r[k] for k in RAW_FIELDS} == {k: want[k] for k in RAW_FIELDS}, cap
        assert r["illegal"].tolist() == want["illegal"][:max(cap, 0)].tolist(), cap
    return want


def same(a, b):
    return a == b and list(a["illegal"].items()) == list(b["illegal"].items())


def columns(typ, key, n_keys, f=None):
    n = len(typ)
    z = np.zeros(n, np.int64)
    return Columns(n=n, process=z.copy(), type=np.asarray(typ, np.int64),
                   f=np.full(n, A.F_INSERT, np.int64) if f is None else np.asarray(f, np.int64),
                   key=np.asarray(key, np.int64), value=z, value2=z.copy(), n_keys=n_keys, aux=np.zeros(1, np.int64),
                   keys=list(range(n_keys)))


@pytest.mark.parametrize("name", list(CASES))
def test_hand_written_cases(ctx, name):
    h = CASES[name]
    agree(ctx, adya.encode(h), caps=(0, 1))
    got = adya.g2_checker().check({}, h, {})
    assert same(got, clj_check(h)) and same(got, EXPECT[name])


def test_unkeyed_insert_raises_from_the_host_path(ctx):
    for h in UNKEYED:
        with pytest.raises(TypeError):
            adya.g2_checker().check({}, h, {})
    assert checker.check_safe(adya.g2_checker(), {}, UNKEYED[0], {})["valid?"] == "unknown"


@pytest.mark.parametrize("K", [1, 63, 64, 65, T - 1, T, T + 1])
def test_key_counts_and_edges(ctx, K):
    """Every key inserted once :ok, the first and the last id twice; then the
    same with an :info insert only for every third key in between."""
    key = np.concatenate([np.arange(K), [0, K - 1]])
    want = agree(ctx, columns(np.full(K + 2, A.TYPE_OK), key, K), caps=(1,))
    ill = [[0, 3 if K == 1 else 2]] + ([[K - 1, 2]] if K > 1 else [])
    assert want["illegal"].tolist() == ill and want["key_count"] == K and want["legal_count"] == K - len(ill)
    assert want["first_illegal_row"] == K
    typ = np.where(np.arange(K + 2) % 3 == 1, A.TYPE_INFO, A.TYPE_OK)
    typ[[0, K - 1, K, K + 1]] = A.TYPE_OK
    want = agree(ctx, columns(typ, key, K))
    assert want["key_count"] == K and want["illegal"].tolist() == ill and want["legal_count"] == int((typ[:K] == A.TYPE_OK).sum()) - len(ill)


def test_one_hot_key(ctx):
    """4096 :ok inserts of one key among others: every row hits one counter."""
    key = np.full(4096 + 64, 5, np.int64)
    key[::65] = np.arange(64) + 6
    want = agree(ctx, columns(np.full(len(key), A.TYPE_OK), key, 80))
    assert want["illegal"].tolist() == [[5, 4096]] and want["key_count"] == 65 and want["legal_count"] == 64
    assert want["first_illegal_row"] == 2 and want["insert_rows"] == 4160


def test_caps(ctx):
    cols = synth.g2_history(n_keys=3 * T + 7, illegal=40, seed=8)
    want = ref_cols(cols)
    I = want["illegal_count"]
    assert I == 40
    agree(ctx, cols, caps=(0, 1, I - 1, I, I + 5))


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("illegal", [0, 7])
def test_random_parity(ctx, seed, illegal):
    cols = synth.g2_history(n_keys=500, illegal=illegal, seed=seed, nemesis_every=97)
    want = agree(ctx, cols, caps=(3,))
    assert want["illegal_count"] == illegal and want["key_count"] == 500
    h = synth.g2_columns_to_ops(cols)
    assert same(adya.g2_checker().check({}, h, {}), clj_check(h))
    assert same(adya.g2_checker().check({}, cols, {}), clj_check(h))


def test_illegal_in_key_order_and_second_call(ctx, monkeypatch):
    h = CASES["unsorted-ids"] + CASES["string-keys"][:0]
    cols = adya.encode(h)
    assert cols.keys == [9, 2, 5, 1]
    assert agree(ctx, cols)["illegal"].tolist() == [[0, 2], [1, 2], [2, 2]]
    assert list(adya.g2_checker().check({}, h, {})["illegal"].items()) == [(2, 2), (5, 2), (9, 2)]
    monkeypatch.setattr(adya, "ILLEGAL_CAP", 2)         # the first call's cap is too small: a second one
    assert same(adya.g2_checker().check({}, h, {}), EXPECT["unsorted-ids"])


def test_return_codes(ctx):
    h = pair(1, "ok", "ok") + pair(2, "ok", "ok") + [other("read", 1)]
    cols = adya.encode(h)

    def mod(**over):
        c = adya.encode(h)
        for name, (i, v) in over.items():
            getattr(c, name)[i] = v
        return c
    nokey = Columns(n=cols.n, process=cols.process, type=cols.type, f=cols.f, key=None, value=cols.value,
                    value2=cols.value2, n_keys=0, aux=cols.aux)
    cases = {"key past n_keys": (mod(key=(0, 2)), A.JH_EINVAL), "insert without a key": (mod(key=(0, -1)), A.JH_EUNSUPPORTED),
             "no key column": (nokey, A.JH_EUNSUPPORTED)}
    for name, (c, code) in cases.items():
        assert ref_cols(c)["rc"] == code, name
        with pytest.raises(_native.JhError) as e:
            ctx.check_g2(c, 4)
        assert e.value.code == code, name
    agree(ctx, mod(key=(8, 7)))                           # not an insert: its key is not read
    agree(ctx, adya.encode([]))
    noins = Columns(n=cols.n, process=cols.process, type=cols.type, f=np.full(cols.n, 16, np.int64), key=None,
                    value=cols.value, value2=cols.value2, n_keys=0, aux=cols.aux)
    agree(ctx, noins)
