"""jepsen.tests.bank/checker without a GPU: the two CPU restatements
(tests/bank_ref.py) against hand-written answers (tests/bank_cases.py) and
against each other, the host half of the mirror (jepsen_amd/bank.py: check_op,
err_badness, the float emulation, encode / decode), and the ctypes layout of
the new structs. The reference tree has no bank test: parity is unpinned
against the reference's own tests."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bank_cases import CASES, RAISING, T, inv, rd
from bank_ref import (check_op, err_badness, points_ref, ref_cols, ref_ops, rows_of, wrong_total_badness)
from conftest import ROOT
from jepsen_amd import _abi as A
from jepsen_amd import bank, checker, synth

HEADER = os.path.join(ROOT, "include", "jh.h")


def n_accounts(test):
    return len(set(test["accounts"]))


@pytest.mark.parametrize("name", list(CASES))
def test_hand_written_answers(name):
    test, opts, h, want = CASES[name]
    negb = bool(opts.get("negative-balances?"))
    got = ref_ops(test, h, negb)
    assert got == want
    cols, table = bank.encode(h, test["accounts"])
    by_cols = ref_cols(cols, n_accounts(test), test["total-amount"], negb)
    by_cols.pop("triples")
    assert by_cols == rows_of(want)
    # the same answer from the op maps the columns decode to
    assert rows_of(ref_ops(test, bank.decode(cols, table), negb)) == rows_of(want)


@pytest.mark.parametrize("name", list(RAISING))
def test_raising_cases(name):
    test, opts, h = RAISING[name]
    negb = bool(opts.get("negative-balances?"))
    with pytest.raises(ArithmeticError):
        ref_ops(test, h, negb)
    cols, _ = bank.encode(h, test["accounts"])
    assert ref_cols(cols, n_accounts(test), test["total-amount"], negb)["raises"] is ArithmeticError


def test_float_badness_emulation():
    """Two implementations of (float (/ diff total-amount)) agree, integers
    below 2^22 never collapse, and 2^24 does."""
    for ta in (1, 3, 7, 100, 1000, -100):
        for d in (1, 2, 99, 100, 12345, (1 << 22) - 1, 1 << 22, (1 << 24) + 1, (1 << 31) + 1, (1 << 53) + 1,
                  (1 << 62) + 12345, -5, -(1 << 40) - 1):
            assert float(abs(bank.ratio_float(d, ta))) == wrong_total_badness(ta + d, ta), (ta, d)
    rng = np.random.default_rng(0)
    for ta in (1, 3, 100, 1 << 20):
        for d in rng.integers(1, (1 << 22) - 1, 300).tolist():
            assert wrong_total_badness(ta + d, ta) < wrong_total_badness(ta + d + 1, ta), (ta, d)
    assert wrong_total_badness(1 + (1 << 24), 1) == wrong_total_badness(2 + (1 << 24), 1)
    assert wrong_total_badness(100 + (1 << 31), 100) == wrong_total_badness(101 + (1 << 31), 100)
    with pytest.raises(ArithmeticError):
        bank.ratio_float(5, 0)


def test_mirror_host_functions_follow_the_restatement():
    """bank.check_op / bank.err_badness (what the mirror rebuilds :first,
    :worst, ... with) give the restatement's error maps and the same order."""
    accts = set(T["accounts"])
    for name, (test, opts, h, want) in CASES.items():
        negb = bool(opts.get("negative-balances?"))
        for i, op in enumerate(h):
            if op["type"] == "ok" and op["f"] == "read":
                op = dict(op, index=i)
                a, b = bank.check_op(accts, test["total-amount"], negb, op), check_op(accts, test["total-amount"], negb, op)
                assert a == b
                if a and not (a["type"] == "wrong-total" and test["total-amount"] <= 0):
                    assert float(bank.err_badness(test, a)) == float(err_badness(test, b))
    with pytest.raises(ArithmeticError):
        bank.check_op(accts, 10, True, rd({0: (1 << 63) - 1, 1: 1, 2: -1}))


SYNTH = [dict(seed=0), dict(seed=1, unexpected=[0, 7, 40], nils=[3, 41], wrong=[5, 6, 90, 91], negative=[9, 200]),
         dict(seed=2, read_sizes=[0, 1, 2, 5, 8], wrong=[4, 17], nil_values=[3, 50], unexpected=[8]),
         dict(seed=3, n_accounts=40, read_sizes=[2, 40, 33], negative=[1, 2, 3], nils=[0])]


@pytest.mark.parametrize("kw", SYNTH)
@pytest.mark.parametrize("negb", [False, True])
def test_restatements_agree_on_synth(kw, negb):
    cols = synth.bank_history(1500, **kw)
    na = kw.get("n_accounts", 8)
    test = {"accounts": list(range(na)), "total-amount": 100}
    ops = synth.bank_columns_to_ops(cols)
    a, b = ref_ops(test, ops, negb), ref_cols(cols, na, 100, negb)
    tri = b.pop("triples")
    assert rows_of(a) == b
    assert a["read-count"] == len(tri) > 500
    planted = sum(len(kw.get(k, ())) for k in ("unexpected", "nils", "wrong", "nil_values")) + \
        (0 if negb else len(kw.get("negative", ())))
    assert a["error-count"] >= planted and (planted == 0) == (a["valid?"] and 0 not in kw.get("read_sizes", [1]))
    # the triples' total is the sum of the non-nil balances
    reads = [op for op in ops if op["type"] == "ok" and op["f"] == "read"]
    for (row, tot, cls), op in list(zip(tri.tolist(), reads))[:400]:
        assert row == op["index"] and tot == sum(x for x in (op["value"] or {}).values() if x is not None)


def test_encode_decode_round_trip():
    test, _, h, _ = CASES["valid"]
    h = h + CASES["cond-priority"][2] + CASES["nil-value"][2] + [inv(1), rd({"x": 1, 0: None, 2: -7}, 1)]
    cols, table = bank.encode(h, [0, 1, 2, 1, 0])                 # duplicates in :accounts are interned once
    assert table[:3] == [0, 1, 2] and table[3:] == [9, "x"]
    assert len(cols.aux) % 2 == 0 and cols.n == len(h)
    back = bank.decode(cols, table)
    for i, (a, b) in enumerate(zip(h, back)):
        assert b["index"] == i and (a["process"], a["type"], a["f"]) == (b["process"], b["type"], b["f"])
        if a["type"] == "ok" and a["f"] == "read":
            assert b["value"] == a["value"] and (a["value"] is None or list(b["value"]) == list(a["value"]))
            if a["value"] is None:
                assert (cols.value[i], cols.value2[i]) == (A.NIL, 0)
        else:
            assert (cols.value[i], cols.value2[i]) == (A.NIL, A.NIL)      # never read by the device
    again, table2 = bank.encode(back, [0, 1, 2])
    assert table2 == table
    for k in ("process", "type", "f", "value", "value2", "aux"):
        assert (getattr(again, k) == getattr(cols, k)).all()
    # history.encode is untouched: a map :value stays one opaque interned value there
    from jepsen_amd import history as H
    assert H.encode(h[:2], keyed=False).values_interned


def test_non_integer_balances_are_a_type_error():
    for v in ({0: 1.5}, {0: "7"}, {0: True}, [[0, 1]]):
        with pytest.raises(TypeError):
            bank.encode([inv(), rd(v)], [0])
    with pytest.raises(OverflowError):
        bank.encode([inv(), rd({0: 1 << 63})], [0])
    bank.encode([inv(), {"process": 0, "type": "fail", "f": "read", "value": {0: 1.5}}], [0])   # not an :ok :read


def test_points_restatement_and_test_map():
    h = [dict(op, time=1_000_000_000 * i) for i, op in enumerate(CASES["first-error"][2])]
    h.append(dict(rd({0: 4}, "nemesis"), time=5))
    assert points_ref(T, h) == {"n1": [[1.0, 10], [3.0, 10], [5.0, 1], [7.0, 0], [9.0, 0]]}
    assert points_ref(T, []) is None
    t = bank.test()
    assert (t["max-transfer"], t["total-amount"], t["accounts"]) == (5, 100, list(range(8)))
    assert isinstance(t["checker"], checker.Compose) and set(t["checker"].checker_map) == {"SI", "plot"}
    assert checker.bank is bank


def test_ctypes_layout_bank(tmp_path):
    prog = tmp_path / "sz4.c"
    prog.write_text(f'''#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(jh_bank_opts),
         offsetof(jh_bank_opts, n_accounts), offsetof(jh_bank_opts, negative_balances),
         offsetof(jh_bank_opts, reserved), sizeof(jh_bank_err), offsetof(jh_bank_err, worst_badness),
         offsetof(jh_bank_err, highest_row), sizeof(jh_bank_result), offsetof(jh_bank_result, read_count),
         offsetof(jh_bank_result, entries), offsetof(jh_bank_result, errors), offsetof(jh_bank_result, device_ms),
         JH_ABI_VERSION);
  return 0; }}''')
    exe = tmp_path / "sz4"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    O, E, R = A.JhBankOpts, A.JhBankErr, A.JhBankResult
    want = [C.sizeof(O), O.n_accounts.offset, O.negative_balances.offset, O.reserved.offset, C.sizeof(E),
            E.worst_badness.offset, E.highest_row.offset, C.sizeof(R), R.read_count.offset, R.entries.offset,
            R.errors.offset, R.device_ms.offset, A.JH_ABI_VERSION]
    assert got == want
    assert A.JH_ABI_VERSION == 8                      # additive: the version does not move
    assert (C.sizeof(O), C.sizeof(E), C.sizeof(R)) == (56, 56, 272)
    assert [n for n, _ in E._fields_] == ["count", "first_row", "last_row", "worst_row", "worst_badness",
                                          "lowest_row", "highest_row"]
    assert A.BANK_TYPES == ("unexpected-key", "nil-balance", "wrong-total", "negative-value")
