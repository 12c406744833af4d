"""Call-order parity: no result may depend on what the context ran before.

Every device checker keeps its scratch in grow-only workspace slots of the
context (jh_ctx::ws), hipMalloc does not zero, and only the linearizability
memo tables ask for zero-on-allocation: a flat-scan checker has to rewrite, on
every call, each counter, histogram, bitmap, ballot word, tile count, atomicMin
cell and meta struct it reads. The session context of conftest.py runs every
other GPU test in one fixed order, each checker after similar cases of its own;
these tests run, on private contexts, the sequences a user with one context
and many histories runs: a large invalid history and then small valid ones
through one entry point, an empty history after a full one, another forced
path, device-resident columns after host-staged ones, every entry point after
every other, two contexts interleaved.

Every call, primers included, is compared with the CPU reference of
call_order_cases.py field by field (never with another device call); lists
whole, with their lengths; `device_ms` is the only field left out. A target is
called with caps a little above its own list lengths, below the primers'.
The linearizability entry points have a contract of their own (generation
tags, test_memo_generation_wrap) and are never called on these contexts.
"""
import types

import numpy as np
import pytest

import call_order_cases as K
from jepsen_amd import _abi as A
from jepsen_amd import _native

pytestmark = pytest.mark.gpu

WITH_PATHS = [(e.name, p) for e in K.ENTRIES for p in e.paths]
SWITCHES = [(e.name, a, b) for e in K.ENTRIES for a in e.paths for b in e.paths if a != b]
HISTORIES = [e.name for e in K.ENTRIES if e.on_device]
ids = lambda v: str(v)          # noqa: E731


@pytest.fixture(scope="module")
def pctx(built):
    """One private context for the module, closed when it ends: the session
    context has the device to itself again."""
    c = _native.Context(0)
    yield c
    c.close()


def path_for(e, case, path):
    """The forced path, or auto where the case cannot take it (a region of the
    cycle search too large for the on-chip tier)."""
    return path if path in e.paths_of(case) else e.paths_of(case)[0]


def run(e, ctx, case, path, dev=None, what=""):
    try:
        return e.check(ctx, case, path_for(e, case, path), dev, what)
    except _native.JhError as err:
        if err.code == A.JH_EDEVICE:             # a HIP error: nothing more is started on this device
            pytest.exit(f"device error in {e.name} / {case.name} ({what}): {err.msg}", returncode=3)
        raise


def run_targets(e, ctx, path, what):
    for t in e.cases()["targets"]:
        run(e, ctx, t, path, what=what)


def device_inputs(case, shift):
    """(DevCols, device :time or None): the case's columns in device memory,
    each `shift` int64s into its allocation."""
    from hipcols import DevCols
    c = case.cols
    z = np.zeros(0, np.int64)
    d = DevCols(types.SimpleNamespace(n=c.n, n_keys=c.n_keys, process=c.process, type=c.type, f=c.f,
                                      key=z if c.key is None else c.key, value=c.value, value2=c.value2,
                                      aux=z if c.aux is None else c.aux), shift)
    if c.key is None:
        d.key = 0
    if getattr(case, "time", None) is None:
        return d, None
    t = np.ascontiguousarray(case.time, np.int64)
    dt = DevCols(types.SimpleNamespace(n=len(t), n_keys=0, process=t, type=z, f=z, key=z, value=z, value2=z, aux=z), shift)
    d.time_cols = dt                                            # kept alive with the columns
    return d, dt.process


# -- one entry point, one context ---------------------------------------------------
@pytest.mark.parametrize("name,path", WITH_PATHS, ids=ids)
def test_targets_on_a_fresh_context(built, name, path):
    e = K.BY_NAME[name]
    ctx = _native.Context(0)
    try:
        run_targets(e, ctx, path, "fresh context")
    finally:
        ctx.close()


@pytest.mark.parametrize("primer", ["dirty", "clean"])
@pytest.mark.parametrize("name,path", WITH_PATHS, ids=ids)
def test_targets_after_a_primer(pctx, name, path, primer):
    e = K.BY_NAME[name]
    run(e, pctx, e.cases()[primer], path, what="primer")
    run_targets(e, pctx, path, f"after the {primer} primer")


@pytest.mark.parametrize("name,path", WITH_PATHS, ids=ids)
def test_empty_history_directly_after_the_dirty_primer(pctx, name, path):
    """The all-zero result: every count 0, every list empty."""
    e = K.BY_NAME[name]
    run(e, pctx, e.cases()["dirty"], path, what="primer")
    want = run(e, pctx, e.target("n0"), path, what="n = 0 after the dirty primer")
    assert all(len(want[k]) == 0 for k in e.capped)


@pytest.mark.parametrize("name,path", WITH_PATHS, ids=ids)
def test_dirty_primer_again_after_the_smallest_targets(pctx, name, path):
    """The buffers a small call may have left short grow again."""
    e = K.BY_NAME[name]
    dirty = e.cases()["dirty"]
    for small in ("n1", "n0"):
        run(e, pctx, e.target(small), path, what="small")
        run(e, pctx, dirty, path, what=f"the dirty primer after {small}")


# -- forced paths ---------------------------------------------------------------------
@pytest.mark.parametrize("name,primer_path,path", SWITCHES, ids=ids)
def test_path_switch(pctx, name, primer_path, path):
    e = K.BY_NAME[name]
    for primer in ("dirty", "clean"):
        run(e, pctx, e.cases()[primer], primer_path, what="primer")
        run_targets(e, pctx, path, f"path {path} after the {primer} primer on path {primer_path}")


# -- host-staged and device-resident columns ---------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("name", HISTORIES)
def test_device_columns_after_a_host_staged_primer(pctx, name, shift):
    e = K.BY_NAME[name]
    path = e.paths[0]
    targets = [t for t in e.cases()["targets"] if t.name in ("n0", "n1", "T-1", "T+0", "T", "T+1")]
    devs = [(t, device_inputs(t, shift)) for t in targets]
    for primer in ("dirty", "clean"):
        run(e, pctx, e.cases()[primer], path, what="host primer")
        for t, dev in devs:
            run(e, pctx, t, path, dev, f"device columns (shift {shift}) after the host-staged {primer} primer")


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("name", HISTORIES)
def test_host_columns_after_a_device_resident_primer(pctx, name, shift):
    e = K.BY_NAME[name]
    path = e.paths[0]
    for primer in ("dirty", "clean"):
        p = e.cases()[primer]
        run(e, pctx, p, path, device_inputs(p, shift), "device primer")
        run_targets(e, pctx, path, f"host columns after the device-resident {primer} primer (shift {shift})")


# -- every entry point after every other ---------------------------------------------------
def test_cross_checker_chain(built):
    """Every entry point once from host columns in the order of include/jh.h,
    then in reverse, on one context, large and small inputs alternating (the
    staging columns WS_COL_* are shared: a checker that stages no key or no
    aux follows one that staged larger ones). Twice, so that the second round
    meets the buffers of the first."""
    ctx = _native.Context(0)
    try:
        for lap in range(2):
            for reverse in (False, True):
                for e, case in K.chain(reverse):
                    run(e, ctx, case, e.paths_of(case)[0], what=f"chain lap {lap} {'reversed' if reverse else 'forward'}")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", K.HANDOFFS, ids=ids)
def test_after_a_larger_staged_key_and_aux(pctx, name):
    """jh.h's order gives few checkers a neighbour that staged what they do
    not: here every checker that stages no key (no aux) directly follows each
    large call that staged one."""
    e = K.BY_NAME[name]
    targets = [t for t in e.cases()["targets"] if t.name in ("n1", "T+1")]
    for s in K.HANDOFFS[name]:
        se = K.BY_NAME[s]
        for t in targets:
            run(se, pctx, se.cases()["dirty"], se.paths[0], what="stager")
            run(e, pctx, t, e.paths[0], what=f"directly after {s} staged its key and aux")


# -- two contexts ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g2", "bank", "cycle"])
def test_two_contexts_interleaved(built, name):
    """Dirty primer on A, target on B, target on A."""
    e = K.BY_NAME[name]
    a = b = None
    try:
        a, b = _native.Context(0), _native.Context(0)
        dirty = e.cases()["dirty"]
        path = e.paths[0]
        for t in e.cases()["targets"]:
            run(e, a, dirty, path, what="dirty primer on A")
            run(e, b, t, path, what="target on B")
            run(e, a, t, path, what="target on A")
        run(e, b, dirty, path, what="dirty primer on B")
        run(e, a, e.target("n0"), path, what="n = 0 on A")
        run(e, b, e.target("n0"), path, what="n = 0 on B")
    finally:
        for c in (a, b):
            if c is not None:
                c.close()
