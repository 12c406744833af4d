"""jh_check_multi_register on the device against the reference
(multi_register_ref.py: the literal model step and the literal WGL), key by
key on valid, cause, fail_entry and explored; the result maps of
checker.linearizable and independent.checker against the per-key generic path
over the host checker."""
import pytest

import multi_register_ref as ref
from multi_register_cases import CASES, UNSUPPORTED, W, R, inv, ok, seq
from test_multi_register_ref import assert_mix
from jepsen_amd import _abi as A
from jepsen_amd import _native, checker, independent, multi_register as M, synth
from jepsen_amd.model import multi_register

pytestmark = pytest.mark.gpu


def device(history, init, ctx=None, **kw):
    got, path = M.verdicts(history, multi_register(init), keyed=True, ctx=ctx, **kw)
    assert path == "device"
    return got


@pytest.mark.parametrize("name,init,history", CASES, ids=[c[0] for c in CASES])
def test_hand_cases(name, init, history):
    assert device(history, init) == ref.check_history(history, init)


@pytest.mark.parametrize("name,init,history", UNSUPPORTED, ids=[c[0] for c in UNSUPPORTED])
def test_unsupported_falls_back_to_the_host_path(name, init, history):
    cols, meta = M.encode(history, multi_register(init), keyed=True)
    with pytest.raises(_native.JhError) as e:
        _native.default_context().check_multi_register(cols, meta["n_regs"], meta["bits"], meta["init"])
    assert e.value.code == A.JH_EUNSUPPORTED
    got, path = M.verdicts(history, multi_register(init), keyed=True)
    assert path == "host" and got == ref.check_history(history, init)
    # the same map as a key the device does take gives: the host path over one key's subhistory
    sub = independent.subhistory(0, history)
    r = checker.linearizable({"model": multi_register(init)}).check({}, sub, {})
    want = M.result_map(ref.check_history(history, init)[0], sub)
    assert r == want and r.explored == want.explored and r["valid?"] is False and r["op"] == dict(sub[r.fail_entry], index=r.fail_entry)


def test_invalid_arguments():
    ctx = _native.default_context()
    h = seq([W(0, 1)], [R(0, 1)])
    cols, meta = M.encode(h, multi_register({}), keyed=True)
    for n_regs, bits, init in ((0, 1, []), (1, 0, [0]), (1, 1, [2])):     # reg >= n_regs, a value id >= 2^bits, init
        with pytest.raises(_native.JhError) as e:
            ctx.check_multi_register(cols, n_regs, bits, init)
        assert e.value.code == A.JH_EINVAL
    bad = M.encode(h, multi_register({}), keyed=True)[0]
    bad.aux[0] = 5                                                         # an f that is neither read nor write
    with pytest.raises(_native.JhError) as e:
        ctx.check_multi_register(bad, 1, 1, [0])
    assert e.value.code == A.JH_EINVAL
    bad = M.encode(h, multi_register({}), keyed=True)[0]
    bad.value2[3] = 2                                                      # the last txn's triples leave aux
    with pytest.raises(_native.JhError) as e:
        ctx.check_multi_register(bad, 1, 1, [0])
    assert e.value.code == A.JH_EINVAL
    assert device(h, {}) == ref.check_history(h, {})                       # the context is whole after the refusals


def test_unkeyed_history_is_one_key():
    h = [dict(op, value=op["value"].val) for op in seq([W(0, 1), W(1, 2)], [R(1, 2)], [R(0, 2)])]
    got, path = M.verdicts(h, multi_register({}), keyed=False)
    assert path == "device" and got == ref.check_history(h, {}, keyed=False) and got[None][:3] == (A.INVALID, 0, 5)
    r = checker.linearizable({"model": multi_register({})}).check({}, h, {})
    assert r["valid?"] is False and r["op"] == dict(h[5], index=5) and r["configs"] == [] and r["final-paths"] == []
    assert checker.linearizable({"model": multi_register({})}).check({}, [], {})["valid?"] is True


@pytest.fixture(scope="module")
def heavy():
    """One key of a few hundred to a few thousand configurations."""
    h = synth.multi_register_history(n_keys=1, ops_per_key=60, threads=10, p_info=0.05, seed=5)
    return h, ref.check_history(h, {})[0]


def test_budget_at_and_below_explored(heavy):
    h, want = heavy
    assert 200 <= want[3] <= 20000 and want[0] != A.UNKNOWN
    assert device(h, {})[0] == want
    assert device(h, {}, budget=want[3])[0] == want
    assert device(h, {}, budget=want[3] - 1)[0] == (A.UNKNOWN, 1, -1, want[3] - 1)


def small_keys(n):
    """n keys of at most 8 rows, a third of them invalid."""
    h = []
    for k in range(n):
        a, b = 1 + k % 3, 1 + (k // 3) % 3
        h += [inv(2 * k, [W(0, a)], k), inv(2 * k + 1, [W(0, b), W(1, a)], k), ok(2 * k + 1, [W(0, b), W(1, a)], k),
              ok(2 * k, [W(0, a)], k)] + seq([R(0, None), R(1, None)], k=k, p=2 * k)[:1] + [ok(2 * k, [R(0, 1 + k % 2), R(1, a)], k)]
    return h


def test_more_keys_than_waves():
    h = small_keys(3000)
    want = ref.check_history(h, {})
    assert len({v[0] for v in want.values()}) == 2 and len(want) == 3000
    assert device(h, {}) == want
    # two waves pull the whole queue; the memo generations wrap on the way
    assert device(h, {}, waves=2, budget=64, flags=A.MR_GEN_JUMP) == want
    assert device(h, {}, waves=2, budget=64) == want


def test_call_order(heavy):
    """The same context after a cas-register check, and two multi-register
    calls with different `bits` (and table sizes) back to back: as fresh
    contexts answer."""
    h2 = small_keys(40)                                                    # 3 values: 2 bits
    h3, _ = heavy                                                          # 5 values: 3 bits
    want2, want3 = ref.check_history(h2, {}), ref.check_history(h3, {})
    fresh = []
    for h in (h2, h3):
        ctx = _native.Context(0)
        fresh.append(device(h, {}, ctx=ctx))
        ctx.close()
    assert fresh == [want2, want3]
    ctx = _native.Context(0)
    cas, _ = synth.cas_register(n_keys=16, ops_per_key=50, seed=3)
    before = ctx.check_cas_independent(cas)[0].copy()
    assert device(h3, {}, ctx=ctx) == want3
    assert device(h2, {}, ctx=ctx) == want2
    assert device(h3, {}, ctx=ctx, budget=want3[0][3]) == want3            # another table size
    assert device(h2, {}, ctx=ctx, budget=want3[0][3]) == want2
    assert device(h3, {}, ctx=ctx) == want3
    assert (ctx.check_cas_independent(cas)[0] == before).all()
    ctx.close()


@pytest.fixture(scope="module")
def seeded():
    h = synth.multi_register_history(n_keys=200, ops_per_key=18, threads=5, p_info=0.1, faulted_keys=range(0, 200, 2),
                                     seed=21)
    per = {}
    for op in h:
        per[op["value"].key] = per.get(op["value"].key, 0) + 1
    assert max(per.values()) <= 40
    return h, ref.check_history(h, {})


def test_seeded_histories(seeded):
    h, want = seeded
    assert_mix(want)
    assert device(h, {}) == want


def test_independent_checker_maps(seeded):
    h, want = seeded
    # indexed as core.clj:441 leaves a history: an :op keeps its row of the whole history on either path
    h = [dict(op, index=i) for i, op in enumerate(h + [{"process": "nemesis", "type": "info", "f": "start", "value": None}])]
    inner = lambda: checker.compose({"linear": checker.linearizable({"model": multi_register({})}), "other": checker.unbridled_optimism()})
    got = independent.checker(inner()).check({}, h, {})
    # the per-key generic path over the host checker ((checker/noop) answers nil, which merge-valid -- here and in
    # checker.clj:33-47 -- cannot rank: the other member is unbridled-optimism)
    results = {}
    for key, sub in independent.subhistories(h).items():
        lin = M.result_map(M.host_verdicts(sub, multi_register({}))[None], sub)
        results[key] = {"linear": lin, "other": {"valid?": True}, "valid?": lin["valid?"]}
    assert got["results"] == results and list(got["results"]) == list(results)
    assert got["failures"] == [k for k, v in want.items() if v[0] != A.VALID] and got["valid?"] is False
    for key, r in got["results"].items():
        assert (r["linear"].explored, r["linear"].fail_entry) == (want[key][3], want[key][2])
    alone = independent.checker(checker.linearizable({"model": multi_register({})})).check({}, h, {})
    assert alone["results"] == {k: r["linear"] for k, r in results.items()} and alone["failures"] == got["failures"]
