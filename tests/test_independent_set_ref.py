"""(independent/checker (checker/set)) without a GPU: the literal transcription
of the two Clojure functions (tests/independent_set_ref.py clj_check) against
the pinned C oracle key by key and against the closed-form numpy restatement
of the batched call (ref_cols, what the device must return), the C layout of
the new structs, and the checker's batched and per-key paths with ref_cols in
the device's place (FakeCtx); tests/test_gpu_independent_set.py runs them on
the device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from jepsen_amd import _abi as A
from jepsen_amd import _native, checker, independent, synth
from jepsen_amd import history as H
from jepsen_amd.history import tuple_
from independent_set_cases import CASES, UNKEYED, added, ia, ir, keyed, nem, oa, rd
from independent_set_ref import FakeCtx, clj_check, clj_set, ref_cols
from oracle import oracle

HEADER = os.path.join(ROOT, "include", "jh.h")
SYNTH = synth.independent_set_columns_to_ops(
    synth.independent_set_history(n_keys=16, adds_per_key=40, threads_per_key=5, p_fail=0.1, p_info=0.1, n_lost_keys=3,
                                  n_unexpected_keys=3, seed=11))
ALL = dict(CASES, synth=SYNTH)


def oracle_map(cols):
    """The (checker/set) map of the pinned oracle's answer on one sub-history."""
    r = oracle.check_set(cols)
    if r["valid"] == A.UNKNOWN:
        return {"valid?": checker.UNKNOWN, "error": "Set was never read"}
    m = {"valid?": r["valid"] == A.VALID}
    for name in ("attempt", "acknowledged", "ok", "lost", "recovered", "unexpected"):
        m[f"{name}-count"] = int(r[f"{name}_count"])
    for i, name in enumerate(checker.SET_NAMES):
        m[name] = checker._runs_str(r["runs"][i].tolist())
    return m


def ref_maps(cols, path=0):
    """{key: map} that ref_cols' raw answer stands for, through the checker's map builder."""
    r = ref_cols(cols, path)
    assert r["rc"] == A.JH_OK
    out = {}
    for kid, key in enumerate(cols.keys):
        rec = r["keys"][kid]
        if rec["rows"]:
            w0, nw = int(rec["word_off"]), int(rec["n_words"])
            out[key] = checker.set_result(rec, [b[w0:w0 + nw] for b in r["bits"]], rec["base"])
    return out


@pytest.mark.parametrize("name", list(ALL))
def test_transcription_oracle_and_closed_form_agree(built, name):
    h = ALL[name]
    want = clj_check(h)
    assert list(want["results"]) == independent.history_keys(h)
    for k in want["results"]:
        sub = independent.subhistory(k, h)
        assert want["results"][k] == oracle_map(H.encode(sub, keyed=False)), k
    for path in (0, 2):
        assert ref_maps(H.encode(h, keyed=True), path) == want["results"]


def test_cases_cover_the_verdicts():
    r = clj_check(CASES["all"])
    assert r["valid?"] is False
    assert {x["valid?"] for x in r["results"].values()} == {True, False, "unknown"}
    assert "never-read/a" not in r["failures"] and "lost/a" in r["failures"]
    assert r["results"]["failed-add-read/a"]["recovered"] == "#{4}"
    assert r["results"]["empty-read/a"]["lost"] == "#{1..2}"
    assert r["results"]["adds-after-the-read/a"]["lost"] == "#{3}"
    assert {True, False} == {x["valid?"] for x in clj_check(SYNTH)["results"].values()}


@pytest.mark.parametrize("name", list(UNKEYED))
def test_unkeyed_history_is_key_zero(built, name):
    h = UNKEYED[name]
    cols = H.encode(h, keyed=True)
    assert cols.n_keys == 0
    r = ref_cols(cols)
    rec = r["keys"][0]
    assert checker.set_result(rec, [b[:int(rec["n_words"])] for b in r["bits"]], rec["base"]) == clj_set(h)
    assert clj_set(h) == oracle_map(cols)
    assert clj_check(h) == {"valid?": True, "results": {}, "failures": []}


# -- the C boundary -----------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry(built):
    src = open(HEADER).read()
    assert re.search(r"^int\s+jh_check_set_independent\s*\(", src, re.M)
    assert "jh_check_set_independent" in src[:src.index("Plain pointers and sizes only")]     # the entry list
    assert hasattr(C.CDLL(_native.LIB_PATH), "jh_check_set_independent")
    assert "jh_check_set_independent" in _native.EXPORTED_SYMBOLS
    consts = dict(re.findall(r"^#define\s+JH_(SI_\w+)\s+\(1(?:LL)?\s*<<\s*(\d+)\)", src, re.M))
    assert {k: 1 << int(v) for k, v in consts.items()} == {"SI_LDS_SPAN": A.SI_LDS_SPAN, "SI_WORDS_MAX": A.SI_WORDS_MAX}
    assert re.search(r"^#define\s+JH_ABI_VERSION\s+8\s*$", src, re.M) and A.JH_ABI_VERSION == 8


def test_ctypes_layout_of_the_new_structs(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text(f'''#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(jh_set_indep_opts), sizeof(jh_set_key),
         sizeof(jh_set_indep_result), offsetof(jh_set_indep_opts, reserved), offsetof(jh_set_key, rows),
         offsetof(jh_set_key, first_fail_entry), offsetof(jh_set_key, n_words),
         offsetof(jh_set_indep_result, keys_valid), offsetof(jh_set_indep_result, total_words),
         offsetof(jh_set_indep_result, device_ms));
  return 0; }}''')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-o", str(exe), str(prog)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(A.JhSetIndepOpts), C.sizeof(A.JhSetKey), C.sizeof(A.JhSetIndepResult),
            A.JhSetIndepOpts.reserved.offset, A.JhSetKey.rows.offset, A.JhSetKey.first_fail_entry.offset,
            A.JhSetKey.n_words.offset, A.JhSetIndepResult.keys_valid.offset, A.JhSetIndepResult.total_words.offset,
            A.JhSetIndepResult.device_ms.offset]
    assert got == want
    assert A.SET_KEY_DTYPE.itemsize == C.sizeof(A.JhSetKey)
    for name in A.SET_KEY_DTYPE.names:
        assert A.SET_KEY_DTYPE.fields[name][1] == getattr(A.JhSetKey, name).offset, name


# -- the checker over a fake device -------------------------------------------------
def use(monkeypatch, fake):
    monkeypatch.setattr(_native, "default_context", lambda device=None: fake)
    return fake


class Noop(checker.Checker):
    def check(self, test, history, opts):
        return {"valid?": True, "rows": len(history)}


@pytest.mark.parametrize("name", list(ALL))
def test_checker_makes_one_batched_call(monkeypatch, name):
    h = ALL[name]
    want = clj_check(h)
    fake = use(monkeypatch, FakeCtx(per_key=False))
    assert independent.checker(checker.set()).check({}, h, {}) == want
    assert (fake.batched_calls, fake.per_key_calls) == (1, 0)
    got = independent.checker(checker.compose({"set": checker.set(), "other": Noop()})).check({}, h, {})
    assert (fake.batched_calls, fake.per_key_calls) == (2, 0)
    assert {k: r["set"] for k, r in got["results"].items()} == want["results"]
    assert got["failures"] == want["failures"] and got["valid?"] == want["valid?"]
    for k, r in got["results"].items():
        assert r["other"] == {"valid?": True, "rows": len(independent.subhistory(k, h))}
        assert r["valid?"] == want["results"][k]["valid?"]


@pytest.mark.parametrize("name", list(ALL))
def test_refused_batched_call_falls_back_to_the_per_key_path(monkeypatch, name):
    h = ALL[name]
    fake = use(monkeypatch, FakeCtx(refuse=A.JH_EUNSUPPORTED))
    got = independent.checker(checker.set()).check({}, h, {})
    n_keys = len(independent.history_keys(h))
    assert (fake.batched_calls, fake.per_key_calls) == (1, n_keys)
    per_key = independent.check_per_key(checker.set(), {}, h)
    assert got["results"] == per_key == clj_check(h)["results"]
    assert got == clj_check(h)


def test_histories_the_batched_path_does_not_take(monkeypatch):
    """Not ints only, and no keys at all: no batched call; an op the encoder
    refuses: the per-key path, which keeps what each key raises."""
    fake = use(monkeypatch, FakeCtx())
    h = keyed({"a": added([1]) + [ir(), rd({1})]}) + [dict(nem(), value="partitioned")]
    got = independent.checker(checker.set()).check({}, h, {})
    assert fake.batched_calls == 0 and fake.per_key_calls == 1
    assert got["results"] == independent.check_per_key(checker.set(), {}, h)
    assert independent.checker(checker.set()).check({}, [nem()], {}) == {"valid?": True, "results": {}, "failures": []}
    assert fake.batched_calls == 0
    # a linearizable member keeps its own batched path: the set member stays per key
    assert independent._set_member(checker.set())[1] is not None
    assert independent._set_member(checker.compose({"s": checker.set()}))[0] == "s"
    assert independent._set_member(Noop()) == (None, None)


# -- the refusals --------------------------------------------------------------------
def test_refusals_are_decided_by_the_closed_form():
    """What the header documents: in a keyed history an un-keyed :ok :read or
    :invoke / :ok :add belongs to every key, and a nil :add element prints in
    hash order: JH_EUNSUPPORTED, the shim falls back. Other un-keyed rows are
    nobody's business."""
    base = keyed({"a": added([1, 2]) + [ir(), rd({1, 2})], "b": added([5]) + [ir(), rd({5})]})
    assert ref_cols(H.encode(base, keyed=True))["rc"] == A.JH_OK
    for extra in (rd({1}), ia(7), oa(7)):
        assert ref_cols(H.encode(base + [extra], keyed=True))["rc"] == A.JH_EUNSUPPORTED
    for extra in (ir(), nem(), {"process": 0, "type": "fail", "f": "add", "value": 3},
                  {"process": 0, "type": "info", "f": "add", "value": 3},
                  {"process": 1, "type": "fail", "f": "read", "value": None}):
        assert ref_cols(H.encode(base + [extra], keyed=True))["rc"] == A.JH_OK
    nil_add = base + [dict(ia(None), value=tuple_("a", None))]
    assert ref_cols(H.encode(nil_add, keyed=True))["rc"] == A.JH_EUNSUPPORTED
    # the same rows in an un-keyed history are key 0's own
    assert ref_cols(H.encode(added([1]) + [ir(), rd({1})], keyed=True))["rc"] == A.JH_OK
    # malformed columns
    cols = H.encode(base, keyed=True)
    bad = H.Columns(**{**cols.__dict__, "key": np.where(cols.key == 1, 2, cols.key)})
    assert ref_cols(bad)["rc"] == A.JH_EINVAL
    last = int(np.nonzero((cols.type == A.TYPE_OK) & (cols.f == A.F_READ))[0][-1])
    for v, c in ((len(cols.aux), 1), (0, len(cols.aux) + 1), (-1, 1), (0, -1)):
        val, val2 = cols.value.copy(), cols.value2.copy()
        val[last], val2[last] = v, c
        assert ref_cols(H.Columns(**{**cols.__dict__, "value": val, "value2": val2}))["rc"] == A.JH_EINVAL
    wide = keyed({"a": added([0, A.SI_LDS_SPAN]) + [ir(), rd({0})]})
    assert ref_cols(H.encode(wide, keyed=True), path=1)["rc"] == A.JH_EINVAL
    assert ref_cols(H.encode(wide, keyed=True), path=0)["path"] == 2
    huge = keyed({"a": added([0, A.SI_SPAN_MAX]) + [ir(), rd({0})]})
    assert ref_cols(H.encode(huge, keyed=True))["rc"] == A.JH_EUNSUPPORTED
