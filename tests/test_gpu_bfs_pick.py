"""Round 8, phase 2's scheduling: the reachable-set BFS of the default race
takes keys by the stall their sequential search publishes (bfs_pick,
jh_lin_opts.bfs_stall_min; jh_summary.bfs_stall_picks counts them) instead of
list order. Scheduling only: every verdict field equals the oracle's whichever
engine settles a key. Every GPU case defers every searching key
(quick_budget=256). Parity and termination only; no test here asserts a time."""
import numpy as np
import pytest

from jepsen_amd import _abi as A
from jepsen_amd import synth
from oracle import oracle

pytestmark = pytest.mark.gpu

BUDGET = 1 << 20
# C3's generator settings (bench.py WORKLOADS["c3"]["gen"]) with p_invalid raised
GEN = dict(threads_per_key=10, readers=5, n_values=5, process_limit=20, groups=10,
           init_nil=True, p_info=0.02, nemesis_every=10000)
QUICK = dict(quick_budget=256)


def _same(gpu, cpu, skip=()):
    for f in A.VERDICT_FIELDS:
        if f in skip:
            continue
        bad = np.nonzero(gpu[f] != cpu[f])[0]
        assert len(bad) == 0, (f, bad[:10], gpu[bad[:5]], cpu[bad[:5]])


@pytest.fixture(scope="module")
def hist():
    """The 96-key history and the oracle's verdicts, built once and left
    unchanged. The oracle facts the cases rest on are asserted here, so a
    generator change cannot empty them: 91 426 entries, 18 invalid keys and no
    unknown one at budget 2^20, every invalid key past any stall minimum up to
    4 096 (at least 6 719 inserts each), 57 keys at 2 048 inserts or more."""
    cols, _ = synth.cas_register(n_keys=96, ops_per_key=500, seed=11, p_invalid=0.3, **GEN)
    want, _ = oracle.check_cas_independent(cols, budget=BUDGET, threads=8)
    assert cols.n == 91426
    invalid = want["valid"] == A.INVALID
    assert invalid.sum() == 18 and (want["valid"] == A.UNKNOWN).sum() == 0
    assert want["explored"][invalid].min() >= 6719
    assert (want["explored"] >= 2048).sum() == 57
    return cols, want


@pytest.fixture(scope="module")
def quiet():
    """32 keys with no invalid one: nothing stalls for long."""
    cols, _ = synth.cas_register(n_keys=32, ops_per_key=500, seed=12, p_invalid=0.0, **GEN)
    want, _ = oracle.check_cas_independent(cols, budget=BUDGET, threads=8)
    assert (want["valid"] == A.VALID).all()
    return cols, want


@pytest.mark.parametrize("bfs_wgs", [1, 2, 200])
def test_pick_exact_counts(ctx, hist, bfs_wgs):
    """One, two and more BFS workgroups than deferred keys, picking from a
    stall of 1 024: every field of every key equals the oracle's, and keys
    were taken by stall. (With one workgroup the 18 invalid keys are all still
    settled: _same compares them.)

    At 200 the grid is 96 workgroups for 96 deferred keys and the sequential
    queue is drained at once, so every workgroup starts with a list-order key
    (rule 2 of bfs_pick, which does not mark keys); the workgroups whose key
    the sequential search settles first then pick by stall. Measured on
    MI355X: the counter reads 8, 11 and 29."""
    cols, want = hist
    g, s = ctx.check_cas_independent(cols, budget=BUDGET, bfs_stall_min=1024, bfs_wgs=bfs_wgs, **QUICK)
    print("bfs_wgs", bfs_wgs, "deferred", s.n_deferred, "picked by stall", s.bfs_stall_picks)
    _same(g, want)
    assert (g["valid"] == A.INVALID).sum() == 18
    assert s.n_deferred > 0
    assert s.bfs_stall_picks >= 1


def test_pick_without_helpers(ctx, hist):
    """JH_LIN_NO_HELPERS: the stalls are published without the helpers that
    used to own the array, and the BFS picks by them."""
    cols, want = hist
    g, s = ctx.check_cas_independent(cols, budget=BUDGET, bfs_stall_min=1024, bfs_wgs=2, flags=A.LIN_NO_HELPERS,
                                     **QUICK)
    print("no helpers: deferred", s.n_deferred, "picked by stall", s.bfs_stall_picks)
    _same(g, want)
    assert s.bfs_stall_picks >= 1


def test_pick_uncounted(ctx, hist):
    """The timed path (no JH_LIN_EXACT_COUNT): every field but explored equals
    the oracle's; explored is equal, or JH_EXPLORED_UNCOUNTED (-3) on a key the
    oracle calls valid (a valid key the BFS settled)."""
    cols, want = hist
    g, s = ctx.check_cas_independent(cols, budget=BUDGET, exact_count=False, bfs_wgs=2, **QUICK)
    print("uncounted: picked by stall", s.bfs_stall_picks, "keys at -3", int((g["explored"] == -3).sum()))
    _same(g, want, skip=("explored",))
    diff = g["explored"] != want["explored"]
    assert (g["explored"][diff] == -3).all() and (want["valid"][diff] == A.VALID).all()


def test_bfs_only_keeps_list_order(ctx, hist):
    """JH_LIN_BFS_ONLY: no sequential search publishes a stall, the BFS takes
    keys in list order (the counter stays 0), the call ends, and the BFS's
    verdicts carry WGL's exact counts (as test_gpu_lin.test_bfs_exact_counts)."""
    cols, want = hist
    g, s = ctx.check_cas_independent(cols, budget=BUDGET, flags=A.LIN_BFS_ONLY, bfs_stall_min=1024, **QUICK)
    assert s.bfs_stall_picks == 0
    _same(g, want)


def test_nothing_stalls(ctx, quiet):
    """The exit rule: no key reaches the minimum for long, so the workgroups
    wait for the sequential queue, run the list-order pass and leave when the
    sequential waves have: the call ends and every field equals the oracle's."""
    cols, want = quiet
    g, s = ctx.check_cas_independent(cols, budget=BUDGET, bfs_stall_min=4096, **QUICK)
    print("quiet: deferred", s.n_deferred, "picked by stall", s.bfs_stall_picks)
    _same(g, want)
    assert s.n_deferred > 0


def test_one_deferred_key(ctx, hist):
    """One deferred key (an invalid one cut out of the 96-key history), four
    workgroups asked for: every field equals the oracle's."""
    from jepsen_amd import shard
    cols, want = hist
    key = int(np.nonzero(want["valid"] == A.INVALID)[0][0])
    own = np.ones(cols.n_keys, np.int64)
    own[key] = 0
    sub, _, _ = shard.shard_history(cols, own, 0)
    assert sub.n_keys == 1
    c, _ = oracle.check_cas_independent(sub, budget=BUDGET, threads=1)
    assert c["valid"][0] == A.INVALID and c["explored"][0] == want["explored"][key]
    g, s = ctx.check_cas_independent(sub, budget=BUDGET, bfs_stall_min=1024, bfs_wgs=4, **QUICK)
    print("one key: deferred", s.n_deferred, "picked by stall", s.bfs_stall_picks)
    _same(g, c)
    assert s.n_deferred == 1
