"""jepsen.tests.causal without a GPU: the literal transcription of the Clojure
(causal_ref.clj_check), the numpy closed form of include/jh.h (ref_cols) and
the mirror's host path (causal.check_host) agree on the hand cases and on
seeded adversarial keys; the mirror's device paths run with ref_cols in the
device's place (FakeCtx); tests/test_gpu_causal.py holds the device to ref_cols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from jepsen_amd import _abi as A
from jepsen_amd import _native, checker, independent, synth
from jepsen_amd import causal as CM
from jepsen_amd.history import tuple_
from causal_cases import CASES, ERRORS, EXPECT, HOST_ONLY, I64_MIN, INIT, GOOD5, keyed, op, rd
from causal_ref import FakeCtx, NoMatchingClause, clj_check, clj_verdict, ref_cols

CODE = {True: A.VALID, False: A.INVALID, "unknown": A.UNKNOWN}


@pytest.fixture
def fake(monkeypatch):
    f = FakeCtx()
    monkeypatch.setattr(checker, "_ctx", lambda: f)
    return f


def want_map(h):
    """clj_check's map, or the string "throws"."""
    try:
        return clj_check(h)
    except NoMatchingClause:
        return "throws"


def got_map(fn):
    try:
        return fn()
    except ValueError:
        return "throws"


def record_map(cols, rec):
    """A jh_causal_key record as the mirror reads it."""
    row = int(rec["row"])
    o = CM.decode_op(cols, row, unwrap=True) if row >= 0 else {}
    m = CM.key_result(rec, o.get("value"), o.get("link"))
    return "throws" if m is None else m


@pytest.mark.parametrize("name", list(CASES))
def test_hand_written_cases(fake, name):
    h = CASES[name]
    v = clj_verdict(h)
    assert v == EXPECT[name] and type(v) is type(EXPECT[name])
    want = want_map(h)
    if name in ERRORS:
        assert want["error"] == ERRORS[name]
    assert got_map(lambda: CM.check_host(CM.causal_register(), h)) == want
    assert got_map(lambda: CM.check(CM.causal_register()).check({}, h, {})) == want
    if name in HOST_ONLY:
        with pytest.raises((TypeError, OverflowError)):
            CM.encode(h)
        assert fake.calls == 0
        return
    assert fake.calls == 1
    cols = CM.encode(h)
    r = ref_cols(cols)
    assert r["rc"] == A.JH_OK and r["valid"] == CODE[v] and len(r["keys"]) == 1
    assert record_map(cols, r["keys"][0]) == want
    assert CM.decode(cols) == [dict(o) for o in CM.decode(CM.encode(CM.decode(cols)))]


def test_valid_models():
    assert clj_check(GOOD5) == {"valid?": True, "model": CM.CausalRegister(2, 2, 14)}
    assert clj_check(CASES["only-invokes"]) == {"valid?": True, "model": CM.CausalRegister(0, 0, None)}
    assert clj_check(CASES["absent-position-then-nil-link"])["model"] == CM.CausalRegister(1, 1, 8)
    assert CM.causal_register() == CM.CausalRegister(0, 0, None) and CM.CausalRegister(0, 0, None) != CM.CausalRegister(0, 0, 1)
    assert CM.inconsistent("x").step({}) == CM.Inconsistent("x") and CM.is_inconsistent(CM.inconsistent("x"))
    assert [g()["f"] for g in (CM.ri, CM.cw1, CM.r, CM.cw2, CM.r)] == ["read-init", "write", "read", "write", "read"]
    assert CM.cw1()["value"] == 1 and CM.cw2()["value"] == 2


def adversarial_key(rng):
    """One key's ops: mostly a correct causal order, with random faults in f,
    value, position, link and type."""
    out, last, w = [], INIT, 0
    for _ in range(int(rng.integers(0, 9))):
        f = ["read-init", "write", "read", "write", "read", "cas"][int(rng.integers(6))] if rng.random() < 0.4 else \
            ["read-init", "write", "read"][int(rng.integers(3))]
        t = "ok" if rng.random() < 0.8 else ["invoke", "fail", "info"][int(rng.integers(3))]
        v = w + 1 if f == "write" else w
        if rng.random() < 0.2:
            v = [None, 0, 1, 2, 3, w + 2, I64_MIN + 2][int(rng.integers(7))]
        pos = None if rng.random() < 0.1 else int(rng.integers(1, 6))
        link = last if rng.random() < 0.8 else [None, INIT, 1, 2, 3, 4, 5][int(rng.integers(7))]
        out.append(op(f, v, pos, None if link is None else link, type=t))
        if t == "ok":
            last = pos
            if f == "write" and v == w + 1:
                w += 1
    return out


def adversarial(seed, n_keys):
    rng = np.random.default_rng(seed)
    return {k: adversarial_key(rng) for k in range(n_keys)}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_adversarial_keys(fake, seed):
    subs = adversarial(seed, 120)                       # 360 keys over the seeds
    h = keyed(subs)
    cols = CM.encode(h, keyed=True)
    r = ref_cols(cols)
    assert r["rc"] == A.JH_OK
    kid = {key: i for i, key in enumerate(cols.keys)}
    seen = set()
    for k, sub in subs.items():
        want = want_map(sub)
        seen.add("throws" if want == "throws" else want["valid?"])
        assert got_map(lambda: CM.check_host(CM.causal_register(), sub)) == want, k
        if k in kid:
            assert want_map(independent.subhistory(k, h)) == want
            assert record_map(cols, r["keys"][kid[k]]) == want, (k, sub)
        else:
            assert sub == []
        one = CM.encode(sub)                              # the same key alone, un-keyed
        assert record_map(one, ref_cols(one)["keys"][0]) == want, k
    assert seen == {True, False, "throws"}
    merged = A.INVALID if r["invalid_keys"] else A.UNKNOWN if r["unknown_keys"] else A.VALID
    assert r["valid"] == merged and r["invalid_keys"] > 0 and r["unknown_keys"] > 0
    # the lifted checker against the generic per-key path
    inner = CM.check(CM.causal_register())
    lifted = independent.checker(inner).check({}, h, {})
    calls = fake.calls
    generic = independent.checker(checker._Fn(lambda t, hh, o: inner.check(t, hh, o))).check({}, h, {})
    assert fake.calls >= calls + len(cols.keys)           # one call per key there, one in all above
    strip = lambda res: {k: ("unknown" if m["valid?"] == "unknown" else m) for k, m in res["results"].items()}  # noqa: E731
    assert strip(lifted) == strip(generic) and lifted["valid?"] is False and lifted["failures"] == generic["failures"]
    for k, m in strip(lifted).items():
        want = want_map(subs[k])
        assert m == ("unknown" if want == "throws" else want)


def test_lifting_inside_compose_and_fallbacks(fake, monkeypatch):
    subs = {"a": GOOD5, "b": CASES["read-stale"], "c": CASES["unknown-f-good-link"], "d": CASES["only-invokes"]}
    h = keyed(subs) + [{"process": "nemesis", "type": "info", "f": "start", "value": None}]
    comp = checker.compose({"causal": CM.check(CM.causal_register()), "optimism": checker.unbridled_optimism()})
    got = independent.checker(comp).check({}, h, {})
    assert got["valid?"] is False and got["failures"] == ["b"]            # :unknown is truthy: no failure
    assert got["results"]["a"] == {"causal": clj_check(GOOD5), "optimism": {"valid?": True}, "valid?": True}
    assert got["results"]["b"]["causal"] == clj_check(subs["b"])
    assert got["results"]["c"]["causal"]["valid?"] == "unknown" and got["results"]["c"]["valid?"] == "unknown"
    assert got["results"]["d"]["causal"] == {"valid?": True, "model": CM.CausalRegister(0, 0, None)}
    # another model, a value without an encoding, an un-keyed :ok op: key by key on the host
    calls = fake.calls
    other = independent.checker(CM.check(CM.CausalRegister(0, 0, 9))).check({}, keyed({"a": GOOD5}), {})
    assert other["results"]["a"] == {"valid?": True, "model": CM.CausalRegister(2, 2, 14)} and fake.calls == calls
    hf = keyed({"a": GOOD5, "f": CASES["float-write"]})
    assert independent.checker(CM.check(CM.causal_register())).check({}, hf, {})["results"] == \
        {"a": clj_check(GOOD5), "f": clj_check(CASES["float-write"])}
    hu = keyed({"a": GOOD5}) + [rd(None, 99, 14)]
    assert independent.checker(CM.check(CM.causal_register())).check({}, hu, {})["results"] == \
        {"a": clj_check(GOOD5 + [rd(None, 99, 14)])}
    # a refusal of the batched call: key by key
    def refuse(*a, **k):
        raise _native.JhError(A.JH_EUNSUPPORTED, "refused")
    monkeypatch.setattr(fake, "check_causal", refuse)
    assert independent.checker(CM.check(CM.causal_register())).check({}, keyed({"a": GOOD5}), {})["results"] == \
        {"a": clj_check(GOOD5)}


def test_ref_cols_return_codes_and_forms():
    h = keyed({"a": GOOD5, "b": CASES["read-stale"]})
    cols = CM.encode(h, keyed=True)
    assert ref_cols(cols)["rc"] == A.JH_OK

    def mod(**over):
        c = CM.encode(h, keyed=True)
        for name, (i, v) in over.items():
            getattr(c, name)[i] = v
        return c
    assert ref_cols(mod(key=(1, 2)))["rc"] == A.JH_EINVAL                 # row 1 is :ok
    assert ref_cols(mod(key=(1, -1)))["rc"] == A.JH_EUNSUPPORTED
    assert ref_cols(mod(key=(1, -1), process=(1, -1)))["rc"] == A.JH_OK   # skipped
    assert ref_cols(mod(key=(1, 2), type=(1, A.TYPE_FAIL)))["rc"] == A.JH_OK
    c = mod()
    c.aux = c.aux[:-1]
    assert ref_cols(c)["rc"] == A.JH_EINVAL
    e = ref_cols(CM.encode([]))
    assert e["rc"] == A.JH_OK and e["valid"] == A.VALID and e["keys"].tolist() == [(A.VALID, 0, -1, 0, A.NIL)]


@pytest.mark.parametrize("violations", [0, 5])
def test_synthetic_history(violations):
    cols = synth.causal_history(n_keys=64, violations=violations, seed=4)
    assert cols.n == 640 and len(cols.aux) == 2 * cols.n
    r = ref_cols(cols)
    assert r["rc"] == A.JH_OK and r["invalid_keys"] == violations and r["unknown_keys"] == 0
    h = synth.causal_columns_to_ops(cols)
    again = CM.encode(h, keyed=True)
    ok = cols.type == A.TYPE_OK                                              # encode keeps the values of :ok rows only
    for name in ("type", "f", "aux"):
        assert np.array_equal(getattr(again, name), getattr(cols, name)), name
    assert np.array_equal(again.value[ok], cols.value[ok]) and (again.value[~ok] == A.NIL).all()
    assert np.array_equal(np.asarray(again.keys)[again.key], cols.key)      # ids by first appearance there
    for k in range(64):
        assert record_map(cols, r["keys"][k]) == clj_check(independent.subhistory(k, h))
    kinds = sorted(int(x) for x in r["keys"]["kind"] if x)
    assert kinds == ([1, 2, 3, 4, 4] if violations else [])       # CAUSAL_VIOLATIONS in turn, the first one twice


def test_ctypes_layout_matches_header(tmp_path):
    prog = tmp_path / "szc.c"
    prog.write_text(f'''#include <stdio.h>
#include <stddef.h>
#include "{os.path.join(ROOT, "include", "jh.h")}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %lld\\n", sizeof(jh_causal_opts), sizeof(jh_causal_key),
         sizeof(jh_causal_result), offsetof(jh_causal_key, last_pos), offsetof(jh_causal_result, first_event_row),
         sizeof(jh_g2_opts), sizeof(jh_g2_result), offsetof(jh_g2_result, first_illegal_row), JH_F_INSERT,
         JH_F_READ_INIT, (long long)JH_CAUSAL_INIT);
  return 0; }}''')
    exe = tmp_path / "szc"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(A.JhCausalOpts), C.sizeof(A.JhCausalKey), C.sizeof(A.JhCausalResult),
                   A.JhCausalKey.last_pos.offset, A.JhCausalResult.first_event_row.offset, C.sizeof(A.JhG2Opts),
                   C.sizeof(A.JhG2Result), A.JhG2Result.first_illegal_row.offset, A.F_INSERT, A.F_READ_INIT, A.CAUSAL_INIT]
    assert A.CAUSAL_KEY_DTYPE.itemsize == C.sizeof(A.JhCausalKey)
    assert tuple_(1, 2).key == 1
