"""jepsen.tests.adya/g2-checker without a GPU: the literal transcription of the
Clojure (g2_ref.clj_check), the numpy closed form of include/jh.h (ref_cols)
and the mirror's host path (adya.check_host) agree on the hand cases and on
seeded histories; the mirror's device path runs with ref_cols in the device's
place (FakeCtx); tests/test_gpu_g2.py holds the device to ref_cols."""
import numpy as np
import pytest

from jepsen_amd import _abi as A
from jepsen_amd import adya, checker, synth
from jepsen_amd.history import Columns
from g2_cases import CASES, EXPECT, UNKEYED, ins, other, pair
from g2_ref import FakeCtx, NotAMapEntry, clj_check, ref_cols


@pytest.fixture
def fake(monkeypatch):
    f = FakeCtx()
    monkeypatch.setattr(checker, "_ctx", lambda: f)
    return f


def same(a, b):
    """Equal maps with :illegal in the same order."""
    return a == b and list(a["illegal"].items()) == list(b["illegal"].items())


@pytest.mark.parametrize("name", list(CASES))
def test_hand_written_cases(fake, name):
    h = CASES[name]
    want = clj_check(h)
    assert same(want, EXPECT[name])
    assert same(adya.check_host(h), want)
    assert same(adya.g2_checker().check({}, h, {}), want) and fake.calls == 1
    cols = adya.encode(h)
    r = ref_cols(cols)
    assert r["rc"] == A.JH_OK and same(adya.result_map(r, cols.keys), want)
    assert r["insert_rows"] == sum(1 for o in h if o["f"] == "insert")


def test_first_illegal_row():
    h = CASES["ok-counts-0-1-2-3"]                      # key 2's second :ok is row 11, key 3's rows 14, 15, 16
    assert ref_cols(adya.encode(h))["first_illegal_row"] == 11
    assert ref_cols(adya.encode(CASES["nemesis-insert"]))["first_illegal_row"] == 2
    assert ref_cols(adya.encode(CASES["single-key-legal"]))["first_illegal_row"] == -1


def test_unkeyed_insert_raises(fake):
    for h in UNKEYED:
        with pytest.raises(NotAMapEntry):
            clj_check(h)
        with pytest.raises(TypeError):
            adya.check_host(h)
        with pytest.raises(TypeError):
            adya.g2_checker().check({}, h, {})
        assert checker.check_safe(adya.g2_checker(), {}, h, {})["valid?"] == "unknown"
    assert fake.calls == 0


def adversarial(seed, n_keys=120, n_ops=700):
    """Inserts and other ops of random types and processes over n_keys keys,
    about a third of them never inserted."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_ops):
        k = int(rng.integers(n_keys))
        t = ["invoke", "ok", "ok", "fail", "info"][int(rng.integers(5))]
        p = "nemesis" if rng.random() < 0.05 else int(rng.integers(4))
        if k % 3 == 0 or rng.random() < 0.1:
            out.append(other(["read", "delete"][int(rng.integers(2))], k, t, p))
        else:
            out.append(ins(k, t, p))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_adversarial_histories(fake, seed):
    h = adversarial(seed)                               # 360 keys over the seeds
    want = clj_check(h)
    assert want["illegal-count"] > 5 and want["legal-count"] > 5 and want["key-count"] > want["illegal-count"] + want["legal-count"]
    assert same(adya.check_host(h), want)
    cols = adya.encode(h)
    assert cols.keys != sorted(cols.keys)
    r = ref_cols(cols)
    assert r["rc"] == A.JH_OK and same(adya.result_map(r, cols.keys), want)
    assert same(adya.g2_checker().check({}, h, {}), want)
    ids = r["illegal"][:, 0].tolist()
    assert ids == sorted(ids)
    oks = [i for i, o in enumerate(h) if o["f"] == "insert" and o["type"] == "ok" and o["value"].key in want["illegal"]]
    firsts = {}
    for i in oks:
        firsts.setdefault(h[i]["value"].key, i)
    assert r["first_illegal_row"] == min(i for i in oks if firsts[h[i]["value"].key] != i)


def test_second_call_when_the_cap_is_small(fake, monkeypatch):
    monkeypatch.setattr(adya, "ILLEGAL_CAP", 2)
    h = adversarial(5)
    want = clj_check(h)
    assert want["illegal-count"] > 2
    assert same(adya.g2_checker().check({}, h, {}), want) and fake.calls == 2


def test_ref_cols_return_codes_and_caps():
    h = pair(1, "ok", "ok") + pair(2, "ok", "ok") + [other("read", 1)]
    cols = adya.encode(h)

    def mod(**over):
        c = adya.encode(h)
        for name, (i, v) in over.items():
            getattr(c, name)[i] = v
        return c
    assert ref_cols(mod(key=(0, 2)))["rc"] == A.JH_EINVAL
    assert ref_cols(mod(key=(0, -1)))["rc"] == A.JH_EUNSUPPORTED
    assert ref_cols(mod(key=(8, 7)))["rc"] == A.JH_OK               # not an insert: its key is not read
    nokey = Columns(n=cols.n, process=cols.process, type=cols.type, f=cols.f, key=None, value=cols.value,
                    value2=cols.value2, n_keys=0, aux=cols.aux)
    assert ref_cols(nokey)["rc"] == A.JH_EUNSUPPORTED
    for cap, k in ((0, 0), (1, 1), (2, 2), (7, 2), (None, 2)):
        r = ref_cols(cols, cap)
        assert len(r["illegal"]) == k and r["illegal_count"] == 2 and r["first_illegal_row"] == 3
    assert ref_cols(adya.encode([]))["rc"] == A.JH_OK


@pytest.mark.parametrize("illegal", [0, 3])
def test_synthetic_history(illegal):
    cols = synth.g2_history(n_keys=64, illegal=illegal, seed=4, nemesis_every=50)
    assert cols.n == 256 + 256 // 50
    h = synth.g2_columns_to_ops(cols)
    again = adya.encode(h)
    for name in ("type", "f", "key"):
        assert np.array_equal(getattr(again, name), getattr(cols, name)), name
    r = ref_cols(cols)
    want = clj_check(h)
    assert same(adya.result_map(r, cols.keys), want)
    assert want["illegal-count"] == illegal and want["key-count"] == 64 and r["insert_rows"] == 256
    assert adya.workload()["checker"].__class__ is adya.G2Checker
