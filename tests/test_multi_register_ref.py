"""The multi-register reference against itself and the host path against the
reference; no device. The normal form is held against the literal step on
every state, the reference WGL against a brute force over every permitted
order, and jepsen_amd.multi_register's host path against the reference on
verdict, cause, failing row and explored."""
import ctypes as C
import os
import random
import re

import pytest

import multi_register_ref as ref
from multi_register_cases import CASES, UNSUPPORTED
from jepsen_amd import _abi as A
from jepsen_amd import _native, checker, independent, multi_register as M, synth
from jepsen_amd.model import MultiRegister, is_inconsistent, multi_register

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_histories():
    """The seeded tiny set: 200 keys of 6 ops on 3 threads, 2 registers, 2
    values, a fault on every second key."""
    return synth.multi_register_history(n_keys=200, ops_per_key=6, threads=3, regs=2, values=2, p_info=0.15,
                                        faulted_keys=range(0, 200, 2), seed=11)


@pytest.fixture(scope="module")
def tiny():
    h = tiny_histories()
    return h, ref.check_history(h, {})


def assert_mix(verdicts):
    """The condition on a seeded set, by the reference's verdicts."""
    n = len(verdicts)
    valid = sum(v[0] == A.VALID for v in verdicts.values())
    invalid = sum(v[0] == A.INVALID for v in verdicts.values())
    assert valid + invalid == n, "an :unknown key in the seeded set"
    assert valid >= 0.2 * n and invalid >= 0.1 * n, (valid, invalid, n)


def test_model_step_is_the_literal_reduce():
    m = multi_register({0: 1})
    assert isinstance(m, MultiRegister) and m.step({"value": [["r", 0, 1], ["r", 1, None]]}) is m
    assert m.step({"value": [["w", 1, 2], ["read", 1, 2], ["write", 0, None]]}) == MultiRegister({0: None, 1: 2})
    r = m.step({"value": [["w", 0, 2], ["r", 0, 1]]})
    assert is_inconsistent(r) and r.msg == "2≠1"
    assert m.step({"value": [["r", 5, "a"]]}).msg == 'nil≠"a"'
    assert m.step({"value": None}) is m
    with pytest.raises(ValueError):
        m.step({"value": [["cas", 0, 1]]})
    rng = random.Random(3)
    for _ in range(500):
        txn = [[rng.choice("rw"), rng.randrange(2), rng.choice([None, 0, 1])] for _ in range(rng.randrange(5))]
        st = {k: v for k, v in ((0, rng.choice([None, 0, 1])), (1, rng.choice([None, 0, 1]))) if v is not None}
        got, want = MultiRegister(st).step({"value": txn}), ref.step(st, txn)
        assert is_inconsistent(got) == (want is None)
        if want is not None:
            assert ref.skey(got.values) == ref.skey(want)


def test_normal_form_is_the_literal_step_on_every_state():
    rng = random.Random(5)
    reg_id, val_id, bits = {0: 0, 1: 1}, {0: 1, 1: 2}, 2
    unpack = {0: None, 1: 0, 2: 1}
    for _ in range(3000):
        txn = [[rng.choice("rw"), rng.randrange(2), rng.choice([None, 0, 1])] for _ in range(rng.randrange(5))]
        nf = ref.normal_form(txn, bits, reg_id, val_id)
        for a in range(3):
            for b in range(3):
                st = {k: v for k, v in ((0, unpack[a]), (1, unpack[b])) if v is not None}
                want = ref.step(st, txn)
                got = ref.nf_step(nf, a | b << bits)
                assert (got is None) == (want is None), (txn, st)
                if want is not None:
                    assert {0: unpack[got & 3], 1: unpack[got >> 2]} == {0: want.get(0), 1: want.get(1)}, (txn, st)


def test_reference_wgl_is_the_brute_force(tiny):
    h, verdicts = tiny
    assert_mix(verdicts)
    per = {}
    for row, op in enumerate(h):
        per.setdefault(op["value"].key, []).append((row, dict(op, value=op["value"].val)))
    for key, rows in per.items():
        cause, ops = ref.prepare(rows)
        assert cause == 0 and len(ops) <= 7
        assert (verdicts[key][0] == A.VALID) == ref.brute(ops, {}), key


def test_host_path_is_the_reference(tiny):
    h, verdicts = tiny
    assert M.host_verdicts(h, multi_register({}), keyed=True) == verdicts
    # a budget at and just below a key's cache size
    key, v = max(verdicts.items(), key=lambda kv: kv[1][3])
    sub = [op for op in h if op["value"].key == key]
    v = ref.check_history(sub, {})[key]
    assert v[3] >= 10 and M.host_verdicts(sub, multi_register({}), budget=v[3], keyed=True)[key] == v
    assert M.host_verdicts(sub, multi_register({}), budget=v[3] - 1, keyed=True)[key] == (A.UNKNOWN, 1, -1, v[3] - 1)
    assert ref.check_history(sub, {}, budget=v[3] - 1)[key] == (A.UNKNOWN, 1, -1, v[3] - 1)


@pytest.mark.parametrize("name,init,history", CASES + UNSUPPORTED, ids=[c[0] for c in CASES + UNSUPPORTED])
def test_host_path_on_the_hand_cases(name, init, history):
    want = ref.check_history(history, init)
    if name == "65-crashed-writers-open-at-one-return":
        assert want[0] == (A.UNKNOWN, 2, -1, 0)           # the device's window rule; the host path has none
        want[0] = ref.wgl(ref.prepare([(r, dict(op, value=op["value"].val)) for r, op in enumerate(history)
                                       if op["value"].key == 0])[1], init)
    assert M.host_verdicts(history, multi_register(init), keyed=True) == want


def test_hand_cases_say_what_their_names_say():
    by = {c[0]: ref.check_history(c[2], c[1]) for c in CASES + UNSUPPORTED}
    valid = lambda n, k=0: by[n][k][0] == A.VALID
    assert valid("reads-own-write") and valid("own-write-from-any-state") and not valid("reads-other-than-own-write")
    assert not valid("two-different-reads-of-one-register") and valid("two-equal-reads-of-one-register")
    assert valid("nil-read-of-never-written") and not valid("non-nil-read-of-never-written")
    assert valid("nil-write-then-read-nil") and not valid("nil-write-then-non-nil-read")
    assert valid("init-read") and not valid("init-read-wrong") and valid("completion-fills-reads") is False
    assert valid("concurrent-writes-either-order") and not valid("torn-read")
    assert valid("valid-only-if-crashed-write-took-effect") and valid("valid-only-if-crashed-write-never-did")
    assert not valid("crashed-write-after-the-read")
    assert by["crashed-read-and-failed-write-dropped"][0] == (A.VALID, 0, -1, 2)
    assert by["no-ok-op"][0] == (A.VALID, 0, -1, 0) and by["only-identity-ops"][0] == (A.VALID, 0, -1, 0)
    assert list(by["nemesis-only-key"]) == [0] and by["empty"] == {}
    assert by["double-invoke-in-one-key-of-three"][1][:2] == (A.UNKNOWN, 3)
    assert by["orphan-completion-in-one-key-of-three"][1][:2] == (A.UNKNOWN, 4)
    assert valid("double-invoke-in-one-key-of-three", 0) and not valid("double-invoke-in-one-key-of-three", 2)
    assert by["orphan-then-double-invoke"][0][:2] == (A.UNKNOWN, 4)
    assert valid("64-crashed-writers-open-at-one-return") and valid("64-crashed-writers-one-needed")
    assert by["65-crashed-writers-open-at-one-return"] == {0: (A.UNKNOWN, 2, -1, 0), 1: (A.VALID, 0, -1, 2)}
    assert not valid("packed-state-32-bits") and not valid("packed-state-33-bits")
    assert valid("64-micro-op-txn") and not valid("65-micro-op-txn")
    _, meta = M.encode(dict((c[0], c) for c in CASES)["packed-state-32-bits"][2], multi_register({}), keyed=True)
    assert meta["n_regs"] * meta["bits"] == 32
    _, meta = M.encode(UNSUPPORTED[0][2], multi_register({}), keyed=True)
    assert meta["n_regs"] * meta["bits"] == 33


def test_encode_layout():
    h = [{"process": 0, "type": "invoke", "f": "read", "value": independent.tuple_("a", [["r", "x", None], ["r", "y", None]])},
         {"process": "nemesis", "type": "info", "f": "start", "value": None},
         {"process": 0, "type": "ok", "f": "read", "value": independent.tuple_("a", [["r", "x", 7], ["r", "y", None]])},
         {"process": 1, "type": "invoke", "f": "write", "value": independent.tuple_("b", [["w", "y", "s"]])},
         {"process": 1, "type": "info", "f": "write", "value": independent.tuple_("b", None)}]
    cols, meta = M.encode(h, multi_register({"z": 7}), keyed=True)
    assert meta["regs"] == ["z", "x", "y"] and meta["values"] == [7, "s"] and meta["bits"] == 2 and meta["init"] == [1, 0, 0]
    assert cols.keys == ["a", "b"] and cols.key.tolist() == [0, -1, 0, 1, 1] and cols.process.tolist() == [0, -1, 0, 1, 1]
    assert cols.value.tolist() == [0, A.NIL, 2, 4, A.NIL] and cols.value2.tolist()[:4] == [2, 0, 2, 1]
    assert cols.aux.tolist() == [A.F_READ, 1, A.NIL, A.F_READ, 2, A.NIL, A.F_READ, 1, 1, A.F_READ, 2, A.NIL, A.F_WRITE, 2, 2]
    with pytest.raises(ValueError):
        M.encode([{"process": 0, "type": "invoke", "f": "x", "value": [["cas", 0, 1]]}], multi_register({}))
    with pytest.raises(TypeError):
        M.encode([{"process": 0, "type": "invoke", "f": "x", "value": [["w", 0, [1, 2]]]}], multi_register({}))


def test_unhashable_values_take_the_host_path():
    h = [{"process": 0, "type": "invoke", "f": "w", "value": [["w", 0, [1, 2]]]},
         {"process": 0, "type": "ok", "f": "w", "value": [["w", 0, [1, 2]]]},
         {"process": 0, "type": "invoke", "f": "r", "value": [["r", 0, None]]},
         {"process": 0, "type": "ok", "f": "r", "value": [["r", 0, [1, 3]]]}]
    r = checker.linearizable({"model": multi_register({})}).check({}, h, {})
    assert r["valid?"] is False and r["op"]["index"] == 3 and r.explored == 1 and r["configs"] == []
    assert checker.linearizable({"model": multi_register({})}).check({}, h[:2], {})["valid?"] is True


def test_checker_surface_and_abi():
    assert checker.linearizable({"model": multi_register({})}).supported()
    r = checker.check_safe(checker.linearizable({"model": multi_register({})}),
                           {}, [{"process": 0, "type": "invoke", "f": "x", "value": [["cas", 0, 1]]}])
    assert r["valid?"] == "unknown" and "No matching clause" in r["error"]
    src = open(os.path.join(ROOT, "include", "jh.h")).read()
    assert re.search(r"^int\s+jh_check_multi_register\s*\(", src, re.M)
    assert "jh_check_multi_register" in src[:src.index("Plain pointers and sizes only")]
    assert hasattr(C.CDLL(_native.LIB_PATH), "jh_check_multi_register")
    assert "jh_check_multi_register" in _native.EXPORTED_SYMBOLS
    assert C.sizeof(A.JhMultiRegisterOpts) == 64 and A.JhMultiRegisterOpts.init.offset == 16
    assert A.JhMultiRegisterOpts.waves.offset == 24 and A.JhMultiRegisterOpts.reserved.offset == 32
