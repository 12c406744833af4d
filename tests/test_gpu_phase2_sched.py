"""Round 7, phase 2's scheduling: the late helpers' pick by the sequential
search's published stall (helper_stall_min), the reserved board servers, and
the dense LEAN instance (p2_waves_per_cu = 6). Scheduling only: on every
history and under every policy each verdict field -- WGL's count included --
equals the oracle's. Parity only; no test here asserts a time."""
import numpy as np
import pytest

from jepsen_amd import _abi as A
from jepsen_amd import synth
from oracle import oracle

pytestmark = pytest.mark.gpu

BUDGETS = (1 << 22, 20000)
C3_KEYS = {0: [1086, 8979, 4457, 8190, 932, 3101], 4: [1631, 4356]}


def _same(gpu, cpu):
    for f in A.VERDICT_FIELDS:
        bad = np.nonzero(gpu[f] != cpu[f])[0]
        assert len(bad) == 0, (f, bad[:10], gpu[bad[:5]], cpu[bad[:5]])


@pytest.fixture(scope="module")
def hists():
    """name -> (history, call options, {budget: the oracle's verdicts}); built
    once and left unchanged.
    c3r0 / c3r4: the C3 keys that end the step on ranks 0 and 4, one big dead
    subtree each, cut out of the rank's history (as test_takeover does).
    q300 / q2000: 150 keys x 300 ops at 12 threads per key, deferred at 300 and
    2 000 inserts: records with the stack below and above the 32-frame ring,
    with and without HBM entries.
    wide: 20 keys x 200 ops at 50 threads per key: WIDE keys share the grid."""
    from bench import WORKLOADS
    from jepsen_amd import shard
    wl = WORKLOADS["c3"]
    out = {}
    for rank, keys in C3_KEYS.items():
        cols, _ = synth.cas_register(n_keys=wl["keys"], ops_per_key=500, seed=wl["seed"] + 7919 * rank, **wl["gen"])
        own = np.ones(cols.n_keys, np.int64)
        own[keys] = 0
        sub, _, _ = shard.shard_history(cols, own, 0)
        out[f"c3r{rank}"] = (sub, {}, BUDGETS)
    b, _ = synth.cas_register(n_keys=150, ops_per_key=300, threads_per_key=12, readers=6, groups=10,
                              p_info=0.0, p_invalid=0.05, nemesis_every=0, init_nil=True, seed=21)
    out["q300"] = (b, dict(quick_budget=300), BUDGETS)
    out["q2000"] = (b, dict(quick_budget=2000), BUDGETS)
    w, _ = synth.cas_register(n_keys=20, ops_per_key=200, threads_per_key=50, readers=25,
                              process_limit=100, p_info=0.1, p_invalid=0.1, seed=71)
    out["wide"] = (w, dict(quick_budget=300), (40000,))
    ref = {}
    for name, (cols, kw, budgets) in out.items():
        for budget in budgets:
            if (id(cols), budget) not in ref:
                ref[(id(cols), budget)] = oracle.check_cas_independent(cols, budget=budget, threads=8)[0]
        out[name] = (cols, kw, {budget: ref[(id(cols), budget)] for budget in budgets})
    return out


@pytest.mark.parametrize("flags", [0, A.LIN_NO_SPEC, A.LIN_NO_RESUME], ids=["spec", "no_spec", "no_resume"])
@pytest.mark.parametrize("stall_min", [0, 256, 1024])
@pytest.mark.parametrize("name", ["c3r0", "c3r4", "q300", "q2000"])
def test_pick_by_stall(ctx, hists, name, stall_min, flags):
    """The default pick (helpers take the key whose search has stalled for
    helper_stall_min inserts, the smallest stall first; 0: the default, 4 096)
    and forced minimums that send helpers to keys early: every field equals
    the oracle's at the full budget and at one the searches run into, with
    the board, without it, and with the deferred searches restarted from the
    root (JH_LIN_NO_RESUME)."""
    cols, kw, want = hists[name]
    for budget, c in want.items():
        g, s = ctx.check_cas_independent(cols, budget=budget, flags=flags, helper_stall_min=stall_min, **kw)
        print(name, "budget", budget, "stall_min", stall_min, "flags", flags, "deferred", s.n_deferred,
              "resumed", s.resumed, "spec jobs / dead / merges", s.spec_jobs, s.spec_dead, s.spec_merges)
        _same(g, c)
        assert s.n_deferred > 0
        if flags & A.LIN_NO_SPEC:
            assert s.spec_jobs == 0 and s.spec_merges == 0
        if flags & A.LIN_NO_RESUME:
            assert s.resumed == 0
        else:
            assert s.resumed > 0


def test_forced_minimum_reaches_the_board(ctx, hists):
    """With a forced minimum the helpers take the C3 tail keys while their
    sequential searches are inside the dead subtree: the helpers' searches
    post to the board, the servers enumerate, and dead results are merged."""
    merged = 0
    for name in ("c3r0", "c3r4"):
        cols, kw, want = hists[name]
        for stall_min in (256, 1024):
            for budget, c in want.items():
                g, s = ctx.check_cas_independent(cols, budget=budget, helper_stall_min=stall_min, **kw)
                _same(g, c)
                assert s.resumed > 0 and s.spec_dead >= s.spec_merges
                merged += s.spec_merges
    assert merged > 0


@pytest.mark.parametrize("per_cu", [0, 3, 6])
@pytest.mark.parametrize("name", ["c3r0", "c3r4", "q300", "q2000", "wide"])
def test_p2_waves_per_cu(ctx, hists, name, per_cu):
    """Phase 2's LEAN role at three waves per CU (32 KB memo, 16 KB Bloom
    filter), at six (the dense instance: 16 KB memo, 8 KB filter) and at the
    default; with WIDE keys in the grid the choice does not apply and the
    shared instance runs: every field equals the oracle's."""
    cols, kw, want = hists[name]
    for budget, c in want.items():
        g, s = ctx.check_cas_independent(cols, budget=budget, p2_waves_per_cu=per_cu, **kw)
        _same(g, c)
        assert s.n_deferred > 0
        if name == "wide":
            assert s.n_deferred_wide > 0
