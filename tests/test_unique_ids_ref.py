"""(checker/unique-ids) without a GPU: the two CPU restatements
(tests/unique_ids_ref.py) against each other and against a hand-written
answer, the ctypes layout of the ABI 8 structs, and the mirror's rank remap
of interned ids."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from jepsen_amd import _abi as A
from jepsen_amd import checker, synth
from unique_ids_ref import ref_cols, ref_ops

HEADER = os.path.join(ROOT, "include", "jh.h")


@pytest.mark.parametrize("kind", ["counter", "flake", "string"])
@pytest.mark.parametrize("dups,nil_acks", [((), 0), ([(5, 2), (2, 7), (60, 2)], 0), ([(3, 3)], 1), ((), 4),
                                           ([(55, 2), (1, 4)], 3)])
def test_restatements_agree(kind, dups, nil_acks):
    cols = synth.unique_ids_history(3000, kind=kind, dups=dups, nil_acks=nil_acks, seed=len(dups) + nil_acks)
    ops = synth.unique_ids_columns_to_ops(cols)
    a, b = ref_ops(ops), ref_cols(cols)
    assert a == b
    assert list(a["duplicated"]) == list(b["duplicated"])          # the same (ascending id) order
    n_dup = sum(h for h, _ in dups) + (nil_acks >= 2)
    assert a["duplicated-count"] == n_dup and a["valid?"] == (n_dup == 0)
    assert len(a["duplicated"]) == min(n_dup, 48)
    assert a["attempted-count"] == 3000
    if nil_acks:
        assert a["range"][0] is None and a["range"][1] is not None
    if nil_acks >= 2:
        assert a["duplicated"][None] == nil_acks


def g(t, v, p=0, f="generate"):
    return {"process": p, "type": t, "f": f, "value": v}


def test_hand_written_history():
    h = [g("invoke", None), g("ok", 7),
         g("invoke", None, 1), g("ok", 3, 1),
         g("invoke", None), g("fail", 3),                 # a failed generate carrying an acked id
         g("invoke", None, 1), g("ok", 7, 1),             # 7 again
         g("invoke", None, 2, "read"), g("ok", 3, 2, "read"),      # a read of 3: not an id
         g("invoke", None), g("ok", None)]                # a nil id
    want = {"valid?": False, "attempted-count": 5, "acknowledged-count": 4, "duplicated-count": 1,
            "duplicated": {7: 2}, "range": [None, 7]}
    assert len(h) == 12
    assert ref_ops(h) == want
    from jepsen_amd import history as H
    assert ref_cols(H.encode(h, keyed=False)) == want


def test_tie_break_keeps_the_larger_ids():
    """More than 48 duplicated ids with equal counts: sort-by is stable over
    the ascending ids and the result is reversed, so (take 48) keeps the 48
    LARGEST ids: of 0..59 each twice, 12..59."""
    h = []
    for rep in range(2):
        for i in range(60):
            h += [g("invoke", None, i % 5), g("ok", i, i % 5)]
    want = {"valid?": False, "attempted-count": 120, "acknowledged-count": 120, "duplicated-count": 60,
            "duplicated": {i: 2 for i in range(12, 60)}, "range": [0, 59]}
    got = ref_ops(h)
    assert got == want and list(got["duplicated"]) == list(range(12, 60))
    from jepsen_amd import history as H
    got = ref_cols(H.encode(h, keyed=False))
    assert got == want and list(got["duplicated"]) == list(range(12, 60))
    # a larger count beats every tie: id 3 a third time stays, 12 goes
    h += [g("invoke", None), g("ok", 3)]
    got = ref_ops(h)
    assert list(got["duplicated"]) == [3] + list(range(13, 60)) and got["duplicated"][3] == 3
    assert ref_cols(H.encode(h, keyed=False)) == got


def test_ctypes_layout_unique_ids(tmp_path):
    prog = tmp_path / "sz3.c"
    prog.write_text(f'''#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(jh_unique_ids_opts), offsetof(jh_unique_ids_opts, path),
         offsetof(jh_unique_ids_opts, reserved), sizeof(jh_unique_ids_result),
         offsetof(jh_unique_ids_result, path), offsetof(jh_unique_ids_result, attempted_count),
         offsetof(jh_unique_ids_result, nil_count), offsetof(jh_unique_ids_result, device_ms), JH_ABI_VERSION);
  return 0; }}''')
    exe = tmp_path / "sz3"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    O, R = A.JhUniqueIdsOpts, A.JhUniqueIdsResult
    want = [C.sizeof(O), O.path.offset, O.reserved.offset, C.sizeof(R), R.path.offset, R.attempted_count.offset,
            R.nil_count.offset, R.device_ms.offset, A.JH_ABI_VERSION]
    assert got == want
    assert A.JH_ABI_VERSION == 8
    assert [n for n, _ in R._fields_] == ["valid", "path", "attempted_count", "acknowledged_count",
                                          "duplicated_count", "range_lo", "range_hi", "nil_count", "device_ms"]


def test_rank_remap_round_trips():
    table = [5, "pear", -3, None, "apple", 0, -(1 << 40), "Pear", 1 << 62]
    rank, order, cls = checker.rank_table(table)
    assert sorted(rank.tolist()) == list(range(len(table)))               # injective
    assert [table[i] for i in order[rank].tolist()] == table              # back and forth
    by_rank = [table[i] for i in order.tolist()]
    assert by_rank == [None, -(1 << 40), -3, 0, 5, 1 << 62, "Pear", "apple", "pear"]
    names = [c[1] for c in cls]
    assert names == ["nil"] + ["number"] * 5 + ["string"] * 3             # classes contiguous
    # the remap the mirror applies to a value column, and its inverse
    codes = np.asarray([1, 0, 4, 8, 2], np.int64)
    assert [table[int(order[r])] for r in rank[codes]] == [table[int(c)] for c in codes]


def test_f_code_lookup():
    cols = synth.unique_ids_history(50, seed=3)
    assert checker._f_code(cols, "generate") == 16 and checker._f_code(cols, "read") == A.F_READ
    cols.f_names = ["start"]
    assert checker._f_code(cols, "generate") == 17                        # unused code
