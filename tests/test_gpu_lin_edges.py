"""The linearizability path (jh_lin.hip) on the boundaries where it switches
paths, against the oracle (every field of jh_key_verdict) and against the
plain reference of lin_ref.py (valid, cause, fail_entry). The cases come from
lin_cases.py; test_lin_cases.py checks the same cases between reference and
oracle without a device, and that they sit where their labels say.

Which boundary each family straddles, from the source: k_key_tables sends a
key to LEAN iff states8 && maxw <= 40, to WIDE up to 64, to k_lin_xw up to
JH_MAX_WINDOW = 256 (two mask slices up to 128, four above); the reachable-set
engine takes maxw <= 32 with n_states < 4096; states8 is n_states <= 256 with
n_states = vmax - vmin + 2 over the whole call; interning turns per-key at a
span of 65 531, where a key holds at most 65 532 values; long_key is n_ok >=
16 000; n_ok >= 2^20 - 1 is past the tables' t field. k_pair works on 64-row
groups of the sorted history that ignore the key segments.
"""
import ctypes

import numpy as np
import pytest

import lin_cases as C
from hipcols import DevCols
from jepsen_amd import _abi as A
from jepsen_amd.history import Columns

pytestmark = pytest.mark.gpu

REF_FIELDS = ("valid", "cause", "fail_entry")
CASES = {c.name: c for c in C.all_cases()}
FLAGS = (0, A.LIN_HELPERS_NOW, A.LIN_NO_HELPERS, A.LIN_NO_RESUME, A.LIN_BFS_ONLY, A.LIN_STREAM, A.LIN_INTERN_PER_KEY)
TUNINGS = [dict(quick_budget=q, flags=f) for q in (1, 40) for f in FLAGS] + \
          [dict(quick_budget=1, xw_waves=1), dict(quick_budget=1, wide_waves=1), dict(quick_budget=1, lean_waves=1)] + \
          [dict(quick_budget=1, p2_waves_per_cu=w) for w in (1, 3, 6)]
TUNED = [f"width{W}" for W in C.WIDTHS] + [f"dropped{W}" for W in C.DROPPED_WIDTHS] + \
        [f"span{s}-high" for s in C.SPANS] + ["span254-low", "span4094-init_low", "span65531-init_high", "span-wrap"] + \
        [f"engines-{w}" for w in C.ENGINE_LISTS]


def as_keyed(case):
    """An un-keyed single-key case as a keyed call of K = 1."""
    c = case.cols
    cols = Columns(n=c.n, process=c.process, type=c.type, f=c.f, key=np.zeros(c.n, np.int64), value=c.value,
                   value2=c.value2, n_keys=1, aux=c.aux)
    return C.Case(case.name, cols, case.init, case.keys, keyed=True, budget=case.budget)


def run(ctx, case, budget=None, **tune):
    """(verdicts by key id, summary or None) from the device."""
    if case.keyed:
        return ctx.check_cas_independent(case.cols, init=case.init, budget=budget or case.budget, **tune)
    d = ctx.check_cas_full(case.cols, init=case.init, budget=budget or case.budget, **tune)
    v = np.zeros(1, A.VERDICT_DTYPE)
    for f in A.VERDICT_FIELDS:
        v[f] = d[f]
    return v, None


def same(got, want, what, fields=A.VERDICT_FIELDS):
    for f in fields:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (what, f, bad[:10].tolist(), got[bad[:5]], want[bad[:5]])


def same_as_reference(case, got, what):
    for k, r in enumerate(C.reference(case)):
        assert tuple(int(got[f][k]) for f in REF_FIELDS) == tuple(r[f] for f in REF_FIELDS), (what, k, got[k], r)


@pytest.mark.parametrize("name", list(CASES))
def test_field_parity(ctx, name):
    """Every field of every key's verdict equals the oracle's, and verdict,
    cause and failing row the plain reference's. A single key goes through
    jh_check_cas and, as a keyed call of K = 1, through
    jh_check_cas_independent."""
    case = CASES[name]
    want = C.expected(case)
    got, _ = run(ctx, case)
    same(got, want, name)
    same_as_reference(case, got, name)
    if not case.keyed:
        got, s = run(ctx, as_keyed(case))
        same(got, want, name + " keyed")
        assert s.n_keys == 1


@pytest.mark.parametrize("shift", [0, 1])
def test_device_resident_columns(ctx, shift):
    """The same verdicts from columns already in HBM (jh_check_cas_independent_
    device), 16-byte and 8-byte aligned: one pass over a case of each family."""
    for name in ("width40", "width65", "dropped64", "span255-high", "span65531-high", "values256-init", "segments",
                 "gaps", "violations", "one-key", "engines-each", "engines-none"):
        case = CASES[name]
        d = DevCols(case.cols, shift)
        p = ctypes.c_void_p()
        nb = max(case.cols.n_keys, 1) * A.VERDICT_DTYPE.itemsize
        assert d._hip.hipMalloc(ctypes.byref(p), nb) == 0
        try:
            ctx.check_cas_independent_device(d, p.value, init=case.init, budget=case.budget)
            v = np.zeros(max(case.cols.n_keys, 1), dtype=A.VERDICT_DTYPE)
            assert d._hip.hipMemcpy(v.ctypes.data, p.value, nb, 2) == 0       # hipMemcpyDeviceToHost
        finally:
            d._hip.hipFree(p)
        same(v[:case.cols.n_keys], C.expected(case), name)


@pytest.mark.parametrize("name", TUNED)
def test_tunings_move_keys_not_verdicts(ctx, name):
    """Families A, B and F under the tunings that move keys between engines and
    phases -- quick budgets 1 and 40 (every search deferred / the short ones
    kept), each scheduling flag, per-key interning forced, one wave per engine,
    1 / 3 / 6 phase-2 waves per CU: every field identical under each."""
    case = CASES[name]
    want = C.expected(case)
    for tune in TUNINGS:
        got, _ = run(ctx, case, **tune)
        same(got, want, (name, tune))


def _searched(case):
    """(key id, engine, the oracle's explored) of the keys key_pass1 passes on:
    every key with an ok return of a kept op and no violation, unless its
    average window passes 256 (sum_w > 256 n_ok). A key whose widest window
    alone passes 256 is among them: k_lin_xw finds that."""
    orc = C.oracle_verdicts(case)
    out = []
    for k, (lab, r) in enumerate(zip(case.keys, C.reference(case))):
        if lab.get("absent") or r["cause"] not in (0, 2) or r["n_ok"] == 0 or r["sum_w"] > A.MAX_WINDOW * r["n_ok"]:
            continue
        out.append((k, C._engine(r["width"], C.n_states(case) <= 256), int(orc["explored"][k])))
    return out


ROUTED = [f"width{W}" for W in C.WIDTHS] + [f"dropped{W}" for W in C.DROPPED_WIDTHS] + \
         [f"span{s}-high" for s in (253, 254, 255, 65_530, 65_531)] + ["span254-low", "span255-low"] + \
         [f"values{n}-{i}" for n in C.VALUE_COUNTS for i in ("nil", "init")] + [f"engines-{w}" for w in C.ENGINE_LISTS]


@pytest.mark.parametrize("name", ROUTED)
def test_routing(ctx, name):
    """Where the summary shows the routing, it is the one the boundaries say:
    n_xw counts the keys wider than 64 (those past 256 too, unless their
    average window passes 256 and key_pass1 settles them); with a quick budget of 1 every LEAN /
    WIDE key whose search makes more than one insert is deferred, and
    n_deferred_wide counts the WIDE ones: width 40 with n_states <= 256 is
    LEAN, the same key with one far-off value elsewhere in the call (n_states
    257) or width 41 is WIDE, width 65 goes to k_lin_xw. A boundary that
    moves by one fails here."""
    case = CASES[name]
    keys = _searched(case)
    got, s = run(ctx, case, quick_budget=1)
    same(got, C.expected(case), name)
    n_xw = sum(1 for _, e, _ in keys if e in ("xw2", "xw4", "window"))
    n_wide = sum(1 for _, e, x in keys if e == "wide" and x > 1)
    n_lean = sum(1 for _, e, x in keys if e == "lean" and x > 1)
    stats = dict(n_xw=s.n_xw, n_deferred=s.n_deferred, n_deferred_wide=s.n_deferred_wide, waves=list(s.waves),
                 wide_entries=s.wide_entries, lean_entries=s.lean_entries, xw_entries=s.xw_entries, xw_ms=s.xw_ms)
    print(name, stats, "want xw / wide / lean", n_xw, n_wide, n_lean)
    assert s.n_xw == n_xw, stats
    assert s.n_deferred_wide == n_wide and s.n_deferred - s.n_deferred_wide == n_lean, stats
    assert (s.waves[1] > 0) == (n_wide > 0) and (s.waves[0] > 0) == (n_lean > 0), stats
    assert (s.wide_entries > 0) == (n_wide > 0) and (s.lean_entries > 0) == (n_lean > 0), stats
    assert (s.waves[3] > 0) == (n_xw > 0) and (s.xw_entries > 0) == (n_xw > 0) and (s.xw_ms > 0) == (n_xw > 0), stats
    assert s.n_keys == sum(1 for lab in case.keys if not lab.get("absent"))


@pytest.mark.parametrize("n_ok", C.LONG_N_OK)
def test_long_key_routing(ctx, n_ok):
    """long_key = n_ok >= 16 000: the sequential key of 15 999 ok ops keeps the
    compact tables (LEAN, deferred at a quick budget of 1), the one of 16 000
    takes k_lin_xw's 32-bit tables; the verdicts are the oracle's either way."""
    for valid in (True, False):
        case = as_keyed(C.long_case(n_ok, valid))
        got, s = run(ctx, case, quick_budget=1)
        same(got, C.expected(C.long_case(n_ok, valid)), case.name)
        assert (s.n_xw, s.n_deferred, s.n_deferred_wide) == ((1, 0, 0) if n_ok >= 16_000 else (0, 1, 0)), \
            (s.n_xw, s.n_deferred, s.n_deferred_wide)


LINEAR = [f"width{W}" for W in C.WIDTHS] + [f"span{s}-high" for s in C.SPANS] + \
         ["span4093-init_high", "span4094-init_low", "span-wrap"]


@pytest.mark.parametrize("name", LINEAR)
def test_linear_algorithm_edges(ctx, name):
    """{:algorithm :linear} on families A and B: every field equals the
    oracle's; a searched key's analyzer is LINEAR exactly when its widest
    window is at most 32 and the call's n_states below 4096 -- it flips
    between W = 32 and 33 and between spans 4 093 and 4 094; :valid? equals
    the WGL run's on every key."""
    import lin_ref as R
    case = CASES[name]
    got, _ = run(ctx, case, algorithm="linear")
    same(got, C.expected(case, algorithm="linear"), name)
    wgl, _ = run(ctx, case)
    assert (got["valid"] == wgl["valid"]).all() and (wgl["analyzer"] == A.ANALYZER_WGL).all()
    ns = C.n_states(case)
    n = 0
    for k, r in enumerate(C.reference(case)):
        if case.keys[k].get("absent") or r["cause"] or r["n_ok"] == 0:
            continue
        assert got["analyzer"][k] == R.linear_analyzer(r["width"], ns, r["n_ok"]), (name, k, r, ns, got[k])
        n += 1
    assert n >= (6 if name != "width257" else 1)
    if name in ("width32", "span4093-high", "span4093-init_high"):
        assert (got["analyzer"] == A.ANALYZER_LINEAR).sum() >= 3
    if name in ("width33", "span4094-high", "span4094-init_low"):
        assert all(got["analyzer"][k] == A.ANALYZER_WGL for k, r in enumerate(C.reference(case))
                   if not r["cause"] and r["n_ok"] and r["width"] >= (33 if name == "width33" else 1))


@pytest.mark.parametrize("W", [32, 33, 64, 65, 128, 129, 256])
def test_frontier_configs_edges(ctx, W):
    """jh_lin_configs on the invalid keys of family A around every engine
    edge: the frontier configurations equal the oracle's, key by key."""
    from oracle import oracle
    case = C.width_case(W)
    bad = np.array([k for k, lab in enumerate(case.keys) if lab["valid"] == A.INVALID])
    assert len(bad) == 4
    g = ctx.lin_configs(case.cols, bad, init=case.init, budget=case.budget)
    o = oracle.lin_configs(case.cols, bad, init=case.init64, budget=case.budget)
    assert g == o
    assert all(g[int(k)] for k in bad)


@pytest.mark.parametrize("eng", list(C.BUDGET_ENGINES))
def test_budget_edge(ctx, eng):
    """One key per engine whose search the budget cuts: with E the oracle's
    count, the device decides it at budget E and gives UNKNOWN / budget with
    explored = E - 1 at budget E - 1, as the oracle does; the summary shows the
    key ran in the engine meant."""
    from oracle import oracle
    case = C.budget_case(eng)
    E = int(C.oracle_verdicts(case)["explored"][0])
    ref = C.reference(case)[0]
    assert ref["valid"] == A.INVALID and E > 40 and C.engine(case, case.keys[0]) == eng
    for keyed in (case, as_keyed(case)):
        got, s = run(ctx, keyed, budget=E, quick_budget=1)
        same(got, C.expected(case), (eng, E))
        same_as_reference(case, got, eng)
        got, _ = run(ctx, keyed, budget=E - 1, quick_budget=1)
        o = oracle.check_cas_full(case.cols, init=case.init64, budget=E - 1)
        assert (o["valid"], o["cause"], o["explored"]) == (A.UNKNOWN, 1, E - 1)
        assert tuple(int(got[f][0]) for f in A.VERDICT_FIELDS) == tuple(o[f] for f in A.VERDICT_FIELDS), (eng, got, o)
    assert s.n_xw == (1 if eng in ("xw2", "xw4") else 0)
    assert s.n_deferred_wide == (1 if eng == "wide" else 0) and s.n_deferred == (1 if eng in ("lean", "wide") else 0)


@pytest.mark.parametrize("n", C.STATES_COUNTS)
def test_states_boundary(ctx, n):
    """65 531 / 65 532 / 65 533 distinct values in one key: the last is
    UNKNOWN / states (JH_CAUSE_STATES; the rule is the reference's, the oracle
    has none), the others are searched; the neighbours in the same call are
    decided as usual, on either side."""
    case = C.states_case(n)
    got, s = run(ctx, case)
    same(got, C.expected(case), case.name)
    same_as_reference(case, got, case.name)
    assert got["cause"][1] == (8 if n > 65_532 else 0) and s.n_unknown == (1 if n > 65_532 else 0)
    got, _ = run(ctx, case, algorithm="linear")
    searched = got["cause"] == 0                                # n_states = n + 1 >= 4096 for the whole call
    assert (got["analyzer"][searched] == A.ANALYZER_WGL).all() and searched.sum() >= 2


@pytest.mark.parametrize("n_ok", C.T_N_OK)
def test_t_limit_pair(ctx, n_ok):
    """n_ok = 2^20 - 2 is searched (k_lin_xw's 32-bit tables: a long key) and
    valid; 2^20 - 1 is UNKNOWN / window, this key alone (the reference's rule;
    the oracle has none). The neighbour is decided as usual."""
    case = C.t_limit_case(n_ok)
    got, s = run(ctx, case)
    same(got, C.expected(case), case.name)
    same_as_reference(case, got, case.name)
    assert s.n_xw == (1 if n_ok < (1 << 20) - 1 else 0)
