"""The cases of lin_cases.py without a device: the plain reference
(lin_ref.py) and the oracle (oracle/jh_oracle.c) agree on every key's verdict,
cause and failing row, every case sits where its label says, and the families
do not degenerate. test_gpu_lin_edges.py holds the device against both."""
import numpy as np
import pytest

import lin_cases as C
import lin_ref as R
from jepsen_amd import _abi as A
from jepsen_amd import history as H

CASES = {c.name: c for c in C.all_cases()}


def _agree(case):
    ref = C.reference(case)
    orc = C.oracle_verdicts(case)
    for k, (r, lab) in enumerate(zip(ref, case.keys)):
        o = orc[k]
        ruled = r["cause"] == 8 or (r["cause"] == 2 and r["n_ok"] >= R.N_OK_LIMIT)
        if not ruled:
            assert (r["valid"], r["cause"], r["fail_entry"]) == (o["valid"], o["cause"], o["fail_entry"]), \
                (case.name, k, lab, r, o)
            assert o["explored"] < case.budget, (case.name, k, o)
        # the label: verdict, failing row, cause and the width it claims
        assert r["valid"] == lab["valid"], (case.name, k, lab, r)
        assert r["fail_entry"] == lab["fail_entry"], (case.name, k, lab, r)
        assert r["cause"] == lab.get("cause", 0), (case.name, k, lab, r)
        if (r["valid"] == A.INVALID) != (lab["fail_entry"] >= 0):
            raise AssertionError((case.name, k, lab, r))
        if "width" in lab and r["cause"] in (0, 2) and not ruled:
            assert r["width"] == lab["width"], (case.name, k, lab, r)
        if lab.get("absent"):
            assert o["explored"] == -1
        elif lab.get("n_ok") is not None:
            assert r["n_ok"] == lab["n_ok"], (case.name, k, lab, r)
    return ref, orc


@pytest.mark.parametrize("name", list(CASES))
def test_reference_equals_oracle(built, name):
    """Verdict, cause and failing row of every key, reference against oracle;
    every label holds; the oracle's search stays under the budget."""
    _agree(CASES[name])


@pytest.mark.parametrize("W", C.WIDTHS)
def test_width_cases_sit_on_their_width(built, W):
    """Both constructions reach exactly W, in valid and invalid keys; the
    concurrent keys' layers hold W + 1 configurations (the chain's prefixes:
    the search is live), the crashed keys' a handful; past 256 every wide key
    is UNKNOWN / window in reference and oracle alike."""
    case = C.width_case(W)
    ref, orc = _agree(case)
    wide = [k for k, lab in enumerate(case.keys) if lab.get("how") in ("crashed", "concurrent")]
    assert len(wide) == 6 and all(ref[k]["width"] == W for k in wide)
    if W > A.MAX_WINDOW:
        assert all(ref[k]["valid"] == A.UNKNOWN and ref[k]["cause"] == 2 for k in wide)
        return
    assert sorted(ref[k]["valid"] for k in wide) == [A.VALID] * 2 + [A.INVALID] * 4
    for k in wide:
        lab = case.keys[k]
        if lab["how"] == "concurrent" and not (lab["valid"] == A.INVALID and lab["place"] == "after"):
            assert ref[k]["layer"] == W + 1, (k, ref[k])
        if lab["how"] == "crashed" and W > 4 and lab["place"] != "after":
            assert 4 <= ref[k]["layer"] <= 64, (k, ref[k])
    # where the failing read sits: after the widest layer was reached, or before it
    for k in wide:
        lab = case.keys[k]
        if lab["valid"] != A.INVALID or W < 3:
            continue
        rows = R.key_rows(case.cols, k)
        _, _, ops = R.complete(rows)
        before = [o for o in ops if o["call"] < lab["fail_entry"]]
        w_before, _, _ = R.widest_window([o if (o["ret"] or 1 << 62) <= lab["fail_entry"] else dict(o, ret=None)
                                       for o in before])
        assert (w_before == W) == (lab["place"] == "before"), (k, lab, w_before)


@pytest.mark.parametrize("W", C.DROPPED_WIDTHS)
def test_dropped_members_do_not_widen(built, W):
    case = C.dropped_case(W)
    ref, _ = _agree(case)
    for k, lab in enumerate(case.keys):
        assert ref[k]["width"] == W and C.engine(case, lab) == C._engine(W)
        rows = R.key_rows(case.cols, k)
        # the dropped ops are invoked before the widest return and completed after it
        wide_row = next(r[0] for r in rows[::-1] if r[1] == 0 and r[2] == A.TYPE_OK and r[0] < rows[-2][0])
        for p in (50, 51, 52)[:lab["n_drop"]]:
            mine = [r[0] for r in rows if r[1] == p]
            assert len(mine) == 2 and mine[0] < wide_row < mine[1]
        assert sum(1 for r in rows if r[1] in (50, 51, 52) and r[2] == A.TYPE_INVOKE) == lab["n_drop"]


def test_span_cases_flip_the_call_not_the_keys(built):
    """One far-off value moves n_states across 256, 4096 and the per-key
    switch; the base keys give the same verdicts and the same WGL counts at
    every span, whichever way the span is set."""
    first = None
    seen = set()
    spans = [C.span_case(s, "high") for s in C.SPANS] + \
            [C.span_case(s, how) for s, how in ((254, "low"), (255, "low"), (4093, "init_high"), (4094, "init_low"),
                                                (65_530, "init_low"), (65_531, "init_high"), (65_531, "low"))] + \
            [C.wrap_case()]
    for case in spans:
        s = case.notes["span"]
        assert C.span(case.cols, case.init) == s
        ns = C.n_states(case)
        if s < 65_531:
            assert ns == s + 2 and not C.per_key_values(case.cols, case.init)
        else:
            assert C.per_key_values(case.cols, case.init) and ns < 256
        seen.add((ns <= 256, ns < 4096, C.per_key_values(case.cols, case.init)))
        o = C.oracle_verdicts(case)[:C.N_SPAN_BASE]
        fields = [tuple(int(o[f][k]) for f in ("valid", "cause", "explored")) for k in range(C.N_SPAN_BASE)]
        first = first or fields
        assert fields == first, case.name
        from oracle import oracle
        assert oracle.linear_states_ok(case.cols, case.init64) == (ns < 4096), case.name
        assert oracle.per_key_values(case.cols, case.init64) == C.per_key_values(case.cols, case.init), case.name
    assert seen == {(True, True, False), (False, True, False), (False, False, False), (True, True, True)}
    assert C.n_states(C.span_case(254, "high")) == 256 and C.n_states(C.span_case(255, "high")) == 257
    assert C.n_states(C.span_case(4093, "high")) == 4095 and C.n_states(C.span_case(4094, "high")) == 4096
    lo, _ = C.value_range(C.span_case(254, "low").cols)
    assert lo < 0


@pytest.mark.parametrize("n", C.VALUE_COUNTS)
def test_value_count_cases(built, n):
    for with_init in (False, True):
        case = C.values_case(n, with_init)
        ref, _ = _agree(case)
        assert C.per_key_values(case.cols, case.init)
        assert ref[1]["n_values"] == ref[1]["row_values"] == n and C.n_states(case) == n + 1
        assert (C.engine(case, case.keys[2]) == "lean") == (n <= 255)


@pytest.mark.parametrize("n", C.STATES_COUNTS)
def test_states_boundary(built, n):
    """65 531 / 65 532 / 65 533 distinct values in one key of about 131 k rows:
    the last is one past what a key may hold (UNKNOWN / states, by the rule:
    the oracle has none and calls the key valid); the neighbours are checked
    as usual. The reference searches the long key like any other."""
    case = C.states_case(n)
    ref, orc = _agree(case)
    assert ref[1]["row_values"] == n and C.per_key_values(case.cols, None)
    assert (ref[1]["valid"], ref[1]["cause"]) == ((A.UNKNOWN, 8) if n > R.MAX_VALUES else (A.VALID, 0))
    assert orc[1]["valid"] == A.VALID
    want = C.expected(case)
    assert (want[1]["valid"], want[1]["cause"]) == (ref[1]["valid"], ref[1]["cause"])
    assert ref[2]["valid"] == A.INVALID and ref[0]["valid"] == A.VALID


@pytest.mark.parametrize("n_ok", C.T_N_OK)
def test_t_limit_pair(built, n_ok):
    """n_ok = 2^20 - 2 and 2^20 - 1, one process, writes only: the rule
    (UNKNOWN / window from 2^20 - 1 on) and a sequential replay stand in for
    the reference's search here, and only here."""
    case = C.t_limit_case(n_ok)
    ref, orc = _agree(case)
    assert ref[0]["n_ok"] == n_ok and ref[0]["width"] == 1
    assert (ref[0]["valid"], ref[0]["cause"]) == ((A.UNKNOWN, 2) if n_ok >= R.N_OK_LIMIT else (A.VALID, 0))
    assert orc[0]["valid"] == A.VALID and orc[0]["explored"] < case.budget
    assert R.linear_analyzer(1, 7, n_ok) == A.ANALYZER_WGL and R.linear_analyzer(1, 7, n_ok - 2) == A.ANALYZER_LINEAR


def test_long_cases_sit_on_the_compact_limit(built):
    for n_ok in C.LONG_N_OK:
        for valid in (True, False):
            case = C.long_case(n_ok, valid)
            r = C.reference(case)[0]
            assert r["n_ok"] == n_ok and r["width"] == 1
            assert case.cols.n - r["fail_entry"] <= 10 if not valid else r["fail_entry"] == -1


def test_families_are_not_degenerate(built):
    """Every engine, verdict and cause the families are about occurs; the
    geometry cases have the sorted layout their docstrings claim."""
    engines, causes = set(), set()
    for case in C.all_cases():
        for lab, r in zip(case.keys, C.reference(case)):
            causes.add(r["cause"])
            if not lab.get("absent") and r["cause"] == 0 and r["n_ok"] > 0:
                engines.add(C._engine(r["width"], C.n_states(case) <= 256))
            if r["cause"] == 2:
                engines.add("window")
    assert engines == {"lean", "wide", "xw2", "xw4", "window"} and causes == {0, 2, 3, 4, 5}
    for which in C.ENGINE_LISTS:
        case = C.engines_case(which)
        got = sorted(C.engine(case, lab) or "none" for lab in case.keys)
        want = {"each": ["lean", "wide", "window", "xw2", "xw4"], "none": ["none"] * 5 + ["window"]}.get(which, [which] * 5)
        assert got == want, (which, got)
    seg = C.segments_case()
    sizes = [int((seg.cols.key == k).sum()) for k in range(seg.cols.n_keys)]
    assert sizes == list(C.SEGMENTS) + [65, 2] and seg.cols.n_keys % 4 != 0
    k = seg.cols.key
    # sorted position 63 is an invocation without a completion; 64 starts the next key with the same process
    order = np.argsort(k, kind="stable")
    assert seg.cols.type[order[63]] == A.TYPE_INVOKE and k[order[63]] == 1 and k[order[64]] == 2
    assert seg.cols.process[order[63]] == seg.cols.process[order[64]] == 0
    last129 = order[sum(sizes[:7]) - 1]
    first_orphan = order[sum(sizes[:7])]
    assert seg.cols.type[last129] == A.TYPE_INVOKE and seg.cols.type[first_orphan] == A.TYPE_OK
    assert seg.cols.process[last129] == seg.cols.process[first_orphan]
    gaps = C.gaps_case()
    for key, off in ((1, 62), (2, 62 + gaps.keys[1]["rows"])):
        rows = R.key_rows(gaps.cols, key)
        got = []
        for i, r in enumerate(rows):
            if r[1] == 7 and r[2] == A.TYPE_INVOKE:
                j = next(j for j in range(i + 1, len(rows)) if rows[j][1] == 7 and rows[j][2] == A.TYPE_OK)
                got.append(j - i)
                if j - i >= 65:
                    assert sum(1 for x in rows[i:j] if x[1] == 7 and x[2] == A.TYPE_INFO) >= 2
        assert got == ([1] + list(C.GAPS) if key == 1 else list(C.GAPS[::-1]))
    assert (62 + gaps.keys[1]["inv_at"][0]) % 64 == 63
    vio = C.violations_case()
    assert vio.cols.n_keys == 11 and [k for k, lab in enumerate(vio.keys) if lab.get("absent")] == [3, 8]
    assert C.one_key_case().cols.n_keys == 1


def test_hand_answers(built):
    """Answers worked out by hand, failing row included."""
    inv, ok, info, fail = H.invoke_op, H.ok_op, H.info_op, H.fail_op
    # 1: write 1, write 2 complete in turn; a later read of 1 is stale: invalid at its completion, row 5
    h = [inv(0, "write", 1), ok(0, "write", 1), inv(0, "write", 2), ok(0, "write", 2), inv(1, "read", None), ok(1, "read", 1)]
    # 2: the same read overlapping the second write: valid (it may precede it)
    h2 = [inv(0, "write", 1), ok(0, "write", 1), inv(0, "write", 2), inv(1, "read", None), ok(0, "write", 2), ok(1, "read", 1)]
    # 3: a crashed write of 3 (open to the end) explains the first read of 3; cas 3 -> 4 then holds, so the
    #    read of 3 at row 9 is stale: window = crashed write + the read = 2, invalid at row 9
    h3 = [inv(0, "write", 3), info(0, "write", 3), inv(1, "read", None), ok(1, "read", 3), inv(2, "cas", [3, 4]),
          ok(2, "cas", [3, 4]), inv(1, "read", None), ok(1, "read", 4), inv(1, "read", None), ok(1, "read", 3)]
    # 4: a failed write, a crashed read and a read of nil are dropped; process 5 invokes twice (row 7: the
    #    first :info does not close it): double invocation beats the orphan at row 8
    h4 = [inv(0, "write", 1), fail(0, "write", 1), inv(1, "read", None), info(1, "read", None), inv(2, "read", None),
          ok(2, "read", None), inv(5, "write", 2), inv(5, "write", 3), ok(6, "read", 1)]
    # 5: the :ok completion supplies the value its invocation left nil: cas [nil nil] -> [1 2] from write 1
    h5 = [inv(0, "write", 1), ok(0, "write", 1), inv(1, "cas", None), ok(1, "cas", [1, 2]), inv(0, "read", None), ok(0, "read", 2)]
    want = [(h, (A.INVALID, 0, 5), 1), (h2, (A.VALID, 0, -1), 2), (h3, (A.INVALID, 0, 9), 2),
            (h4, (A.UNKNOWN, 3, -1), 0), (h4[:7] + h4[8:], (A.UNKNOWN, 4, -1), 0), (h4[:6], (A.VALID, 0, -1), 0),
            (h5, (A.VALID, 0, -1), 1)]
    from oracle import oracle
    for hist, (valid, cause, row), width in want:
        cols = H.encode(hist, keyed=False)
        r = R.check(R.key_rows(cols))
        assert (r["valid"], r["cause"], r["fail_entry"], r["width"]) == (valid, cause, row, width), (hist, r)
        assert oracle.check_cas(cols)[:3] == (valid, cause, row), hist
    # the cap is a condition, not a tolerance: twenty concurrent writes of distinct values pass it
    k = C.Key()
    for p in range(20):
        k.inv(p, C.WR, p)
    for p in range(20):
        k.lin(p)
    for p in range(20):
        k.ok(p)
    with pytest.raises(R.CapExceeded):
        R.check(R.key_rows(C.single("cap", k).cols))
