"""jepsen.tests.causal-reverse without a GPU: the literal transcription of the
Clojure loop (tests/causal_reverse_ref.py clj_check) against the mirror's host
implementation and against the closed-form numpy restatement (ref_cols, what
the device must return), the reference's own six histories, the vector quirk,
the encoding, and the independent lifting. The mirror's device paths run here
with ref_cols in the device's place (FakeCtx); tests/test_gpu_causal_reverse.py
runs them on the device."""
import json
import os

import pytest

from conftest import GOLD
from jepsen_amd import _abi as A
from jepsen_amd import causal_reverse as CR
from jepsen_amd import checker, independent
from jepsen_amd.history import tuple_
from causal_reverse_cases import CASES, QUIRK_AS_SETS, QUIRK_HOST, edge, op, random_key, rd, seq, wi, wo
from causal_reverse_ref import FakeCtx, clj_check, ref_cols

GOLDEN = json.load(open(os.path.join(GOLD, "causal_reverse.json")))["cases"]
ALL = dict(CASES, **{f"edge-{c}-{d}": edge(c, d) for c in (31, 32, 33, 64, 65) for d in (0, c - 1)},
           **{f"random-{s}": random_key(s) for s in range(300)})


def closed_form_map(h):
    """The result map that ref_cols' raw answer stands for."""
    r = ref_cols(CR.encode(h))
    assert r["rc"] == A.JH_OK
    res = dict(r, errors=r["errors"], missing=r["missing"])
    return {"valid?": r["valid"] == A.VALID, "errors": [m for _, m in CR.error_maps(res, lambda row: h[row])]}


@pytest.fixture
def fake(monkeypatch):
    f = FakeCtx()
    monkeypatch.setattr(checker, "_ctx", lambda: f)
    return f


@pytest.mark.parametrize("name", list(ALL))
def test_closed_form_equals_the_clojure_loop(name):
    h = ALL[name]
    want = clj_check(h, as_sets=True)
    assert closed_form_map(h) == want
    assert CR.check_host(h, vectors_as_sets=True) == want


@pytest.mark.parametrize("name", list(ALL))
def test_host_implementation_keeps_the_vector_quirk(name, fake):
    h = ALL[name]
    assert CR.check_host(h) == clj_check(h)
    assert CR.checker().check({}, h, {}) == clj_check(h)
    vector = any(o["type"] == "ok" and o["f"] == "read" and isinstance(o["value"], list) for o in h)
    assert fake.calls == (0 if vector else 1)                     # a vector read: no device involved


def test_some_random_keys_fail_and_some_show_the_quirk():
    """The random keys are worth their name: both verdicts occur, and the index
    test changes some answers."""
    verdicts = {clj_check(ALL[f"random-{s}"], as_sets=True)["valid?"] for s in range(300)}
    assert verdicts == {True, False}
    assert any(clj_check(ALL[f"random-{s}"]) != clj_check(ALL[f"random-{s}"], as_sets=True) for s in range(300))


def test_graph_and_errors_mirror_the_namespace():
    h = seq(1, 2) + [wi(3), rd([3]), wo(3)]
    g = CR.graph(h)
    assert dict(g.items()) == {1: frozenset(), 2: frozenset({1}), 3: frozenset({1, 2})}
    assert g.get(9) is None
    errs = CR.errors(h, g)
    assert errs == [{"process": 1, "type": "ok", "f": "read", "missing": [1, 2], "expected-count": 2}]
    assert CR.errors(h, dict(g.items())) == errs                  # a plain map of sets works too
    assert CR.r() == {"type": "invoke", "f": "read", "value": None}
    assert CR.w(4) == {"type": "invoke", "f": "write", "value": 4}
    assert isinstance(CR.workload({})["checker"], checker.Compose)
    assert checker.causal_reverse is CR


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_golden_histories(case, fake):
    h, want = case["history"], case["valid?"]
    assert clj_check(h)["valid?"] is want
    assert CR.checker().check({}, h, {})["valid?"] is want and fake.calls == 0
    # as sets: the host implementation, the closed form, and the mirror's device path over the closed form
    assert CR.check_host(h, vectors_as_sets=True)["valid?"] is want
    assert closed_form_map(h)["valid?"] is want
    for path in (A.CR_PATH_AUTO, A.CR_PATH_LDS, A.CR_PATH_GLOBAL):
        assert CR.checker(vectors_as_sets=True, path=path).check({}, h, {}) == clj_check(h, as_sets=True)
    assert fake.calls == 3


def test_vector_quirk_changes_the_answer(fake):
    h = CASES["vector-quirk"]
    assert CR.checker().check({}, h, {}) == QUIRK_HOST == clj_check(h)
    assert CR.checker(vectors_as_sets=True).check({}, h, {}) == QUIRK_AS_SETS == clj_check(h, as_sets=True)
    assert CR.check_host(h, vectors_as_sets=True) == QUIRK_AS_SETS
    # a set read of the same elements is the device's business by default
    hs = h[:-1] + [rd(frozenset([5, 3]))]
    calls = fake.calls
    assert CR.checker().check({}, hs, {}) == QUIRK_AS_SETS and fake.calls == calls + 1


def test_encode_decode_round_trip():
    h = CASES["fail-and-info-writes"] + CASES["reads-of-other-types"] + [op("ok", "read", None), op("info", "start", None, "nemesis")]
    cols = CR.encode(h)
    assert cols.n == len(h) and cols.n_keys == 0
    back = CR.decode(cols)
    want = [dict(o, value=None) if o["f"] == "read" and o["type"] != "ok" else o for o in h]   # only :ok reads keep :value
    assert back == want
    assert CR.decode(CR.encode(back)) == back
    # sets are stored ascending; repeated elements of a vector stay
    c2 = CR.encode([rd({3, 1, 2}), rd([2, 2, 1])])
    assert c2.aux.tolist() == [1, 2, 3, 2, 2, 1] and c2.value.tolist() == [0, 3] and c2.value2.tolist() == [3, 3]
    # keyed: independent tuples give the key column
    hk = [dict(o, value=tuple_("a" if i % 2 else "b", o["value"])) for i, o in enumerate(seq(1, 2) + [rd([1, 2])])]
    ck = CR.encode(hk, keyed=True)
    assert ck.keys == ["b", "a"] and ck.key.tolist() == [0, 1, 0, 1, 0] and CR.decode(ck) == hk


def test_values_without_an_encoding_run_on_the_host(fake):
    h = [wi("a"), wo("a"), wi("b"), wo("b"), rd({"b"})]
    with pytest.raises(TypeError):
        CR.encode(h)
    for bad in ([wi(None)], [wi(1 << 63)], [wi(-(1 << 63))], [rd({1.5})], [rd(7)]):
        with pytest.raises((TypeError, OverflowError)):
            CR.encode(bad)
    got = CR.checker().check({}, h, {})
    assert got == clj_check(h) and got["valid?"] is False and got["errors"][0]["missing"] == ["a"]
    assert fake.calls == 0


def test_unsupported_falls_back_to_the_host(fake):
    """JH_EUNSUPPORTED from the device (here: a keyless write inside a keyed
    history, through Columns) is answered by check_host."""
    h = seq(1, 2) + [rd({2})]
    cols = CR.encode([dict(o, value=tuple_(0, o["value"])) for o in h], keyed=True)
    cols.key[0] = -1
    assert ref_cols(cols)["rc"] == A.JH_EUNSUPPORTED
    got = CR.checker().check({}, cols, {})
    assert fake.calls == 1 and got["valid?"] is False and got["errors"][0]["missing"] == [1]


def test_device_refusing_a_nil_write_is_answered_by_the_host(fake):
    """Columns with a write of nil: the device says JH_EUNSUPPORTED, check_host
    answers on the decoded ops (no re-encoding is involved)."""
    h = seq(1, 2, 3) + [rd([3, 2]), rd([1])]
    cols = CR.encode(h)
    cols.value[2] = A.NIL
    assert ref_cols(cols)["rc"] == A.JH_EUNSUPPORTED
    ops = [CR.decode_op(cols, i, unwrap=True) for i in range(cols.n)]
    assert ops[2]["value"] is None
    assert CR.checker().check({}, cols, {}) == clj_check(ops, as_sets=True) and fake.calls == 1


def test_lifting_falls_back_on_any_device_error(fake, monkeypatch):
    """JH_ENOMEM, JH_EINVAL ... from the batched call: every key through the
    inner checker, as the per-key path does (check_safe makes what it raises an
    :unknown result)."""
    from jepsen_amd import _native
    h = keyed_history(4)

    def refuse(*a, **k):
        fake.calls += 1
        if fake.calls == 1:
            raise _native.JhError(A.JH_ENOMEM, "scratch")
        return FakeCtx.check_causal_reverse(fake, *a, **k)
    monkeypatch.setattr(fake, "check_causal_reverse", refuse)
    got = independent.checker(CR.checker()).check({}, h, {})
    assert fake.calls > 1 and got["results"] == {k: clj_check(independent.subhistory(k, h)) for k in got["results"]}


def keyed_history(n_keys, seed=0):
    """Keys interleaved row by row; reads are sets, so the batched path takes them."""
    subs = [[dict(o, value=frozenset(o["value"])) if o["f"] == "read" and isinstance(o["value"], list) else o
             for o in random_key(1000 * seed + k, 30)] + seq(1, 2) + [rd(frozenset([2]) if k % 3 else frozenset([1, 2]))]
            for k in range(n_keys)]
    out = []
    for i in range(max(len(s) for s in subs)):
        for k, s in enumerate(subs):
            if i < len(s):
                out.append(dict(s[i], value=tuple_(f"k{k}", s[i]["value"])))
    return out


def generic_map(inner, h):
    """The per-key path: the lifting does not recognise a checker behind a function."""
    return independent.checker(checker._Fn(lambda t, hh, o: inner.check(t, hh, o))).check({}, h, {})


def test_independent_lifting_equals_the_per_key_path(fake):
    h = keyed_history(16)
    lifted = independent.checker(CR.checker()).check({}, h, {})
    assert fake.calls == 1                                       # one call for all keys
    per_key = generic_map(CR.checker(), h)
    assert fake.calls == 1 + 16
    assert lifted == per_key
    assert list(lifted["results"]) == [f"k{k}" for k in range(16)] == list(per_key["results"])
    assert lifted["valid?"] is False and lifted["failures"] and set(lifted["failures"]) < set(lifted["results"])
    for k, r in lifted["results"].items():
        assert r == clj_check(independent.subhistory(k, h))
    # composed: the causal-reverse member is batched, the others run per key
    comp = checker.compose({"sequential": CR.checker(), "noop": checker.unbridled_optimism()})
    calls = fake.calls
    got = independent.checker(comp).check({}, h, {})
    assert fake.calls == calls + 1
    for k, r in got["results"].items():
        assert r == {"sequential": lifted["results"][k], "noop": {"valid?": True}, "valid?": lifted["results"][k]["valid?"]}
    assert got["failures"] == lifted["failures"]


def test_lifting_leaves_what_the_device_does_not_judge_to_the_per_key_path(fake):
    # vector reads (the default keeps the quirk), and a keyless write that belongs to every key
    hv = [dict(o, value=tuple_(k, o["value"])) for k in range(3) for o in CASES["vector-quirk"]]
    assert independent.checker(CR.checker()).check({}, hv, {}) == generic_map(CR.checker(), hv)
    assert fake.calls == 0
    assert independent.checker(CR.checker())._results_map({})["valid?"] is True
    hu = [wi(1), wo(1)] + [dict(o, value=tuple_(k, o["value"])) for k in range(2) for o in seq(2) + [rd(frozenset([2]))]]
    got = independent.checker(CR.checker()).check({}, hu, {})
    assert got == generic_map(CR.checker(), hu) and got["valid?"] is False
    assert [len(r["errors"]) for r in got["results"].values()] == [1, 1]


def test_synthetic_workload_is_valid_until_violated():
    from jepsen_amd import synth
    for seed in range(3):
        cols = synth.causal_reverse_history(n_keys=8, ops_per_key=60, seed=seed)
        r = ref_cols(cols)
        assert cols.n == 8 * 120 and r["rc"] == A.JH_OK and r["valid"] == A.VALID and r["read_count"] > 0
        bad = ref_cols(synth.causal_reverse_history(n_keys=8, ops_per_key=60, violations=5, seed=seed))
        assert bad["valid"] == A.INVALID and 1 <= bad["error_count"] <= 5
    big = synth.causal_reverse_history(n_keys=4, ops_per_key=20, violations=1, seed=1, tile=3)
    assert big.n_keys == 12 and ref_cols(big)["error_count"] == 3
    ops = synth.causal_reverse_columns_to_ops(big)
    enc = CR.encode(ops, keyed=True)
    assert [enc.keys[k] for k in enc.key.tolist()] == big.key.tolist() and enc.value2.tolist() == big.value2.tolist()
