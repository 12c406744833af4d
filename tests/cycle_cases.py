"""Seeded random histories and hand-written graphs shared by the cycle tests."""
import random

from jepsen_amd import _abi as A

N = A.CY_LDS_VERTICES


def inv(p, v=None):
    return {"process": p, "type": "invoke", "f": "txn", "value": v}


def done(p, t, v=None):
    return {"process": p, "type": t, "f": "txn", "value": v}


def txn_ops(*txns):
    """cycle_test.clj:248-252: every txn as an invoke and an :ok of process 0."""
    return [o for t in txns for o in (inv(0, t), done(0, "ok", t))]


def random_history(seed, n_procs, n_ops, txns=False, healthy=True, n_keys=3, nemesis=True):
    """Well-paired ops of n_procs processes, completions :ok / :fail / :info,
    every invoke completed. txns: completions carry [f k v] micro-ops; writes
    take a fresh value per key; a healthy read sees a value some earlier :ok
    wrote (or nil), an unhealthy one a value around the key's counter, which may
    be written later (back edges, cycles) or never."""
    rng = random.Random(seed)
    h, open_, counter, committed = [], {}, {}, {}

    def complete(p):
        t = rng.choice(["ok", "ok", "ok", "ok", "fail", "info"])
        v, mine = None, []
        if txns:
            v = []
            for _ in range(rng.randint(0, 4)):
                k = rng.randrange(n_keys)
                if rng.random() < 0.5:
                    counter[k] = counter.get(k, 0) + 1
                    v.append(["w", k, counter[k]])
                    mine.append((k, counter[k]))
                elif healthy:
                    v.append(["r", k, rng.choice(committed.get(k, []) + [None])])
                else:
                    v.append(["r", k, max(0, counter.get(k, 0) + rng.randint(-2, 2)) or None])
            if t == "ok":
                for k, x in mine:
                    committed.setdefault(k, []).append(x)
        h.append(done(p, t, v))
        del open_[p]

    while len(h) < n_ops:
        if nemesis and rng.random() < 0.05:
            h.append({"process": "nemesis", "type": "info", "f": "start", "value": None})
            continue
        p = rng.randrange(n_procs)
        if p in open_:
            complete(p)
        else:
            open_[p] = True
            h.append(inv(p))
    for p in list(open_):
        complete(p)
    return h


def ring(n, first=0):
    return [(first + i, first + (i + 1) % n) for i in range(n)]


def chain_of_cycles(k):
    """k two-cycles (2i, 2i+1), each linked back to the one before: every pivot's
    backward reach is all that is left, about 1.5 k^2 edge visits in all."""
    e = []
    for i in range(k):
        e += [(2 * i, 2 * i + 1), (2 * i + 1, 2 * i)]
        if i:
            e.append((2 * i, 2 * i - 1))
    return e


# name -> (n, edges): the edge shapes of the region decomposition and of the region kernel
GRAPHS = {
    "ring-N": (N, ring(N)),
    "ring-N+1": (N + 1, ring(N + 1)),
    "chain-no-back-edge": (300, [(i, i + 1) for i in range(299)]),
    "regions-stay-two": (8, [(3, 0), (0, 3), (7, 4), (4, 7), (3, 4)]),
    "regions-merge": (8, [(4, 0), (0, 4), (7, 4), (4, 7)]),
    "nested-intervals": (10, [(9, 0), (0, 9), (6, 3), (3, 6), (5, 4), (4, 5), (1, 2)]),
    "only-self-loops": (5, [(i, i) for i in range(5)]),
    "repeated-edges": (4, [(0, 1), (0, 1), (1, 0), (1, 0), (1, 0), (2, 3)]),
    # region [1, 3] from the back edge 3 -> 1, and no cycle in it
    "trims-to-nothing": (6, [(0, 1), (3, 1), (1, 2), (2, 4), (4, 5)]),
    # region [0, 4]: {3, 4} -> 0 -> {1, 2}; vertex 0 survives the trimming and is an SCC of one
    "two-sccs-trivial-between": (7, [(3, 4), (4, 3), (1, 2), (2, 1), (4, 0), (0, 1), (2, 5), (5, 6)]),
    "two-cycles-63-64-255-256": (300, [(63, 64), (64, 63), (255, 256), (256, 255)]),
    "back-edge-chain-100": (200, chain_of_cycles(100)),
}


def wr_history(seed):
    """The seeded random txn history of the wr closed-form tests."""
    rng = random.Random(1000 + seed)
    return random_history(seed, rng.randint(1, 5), rng.randint(4, 60), txns=True, healthy=seed % 3 == 0)


def _unknown_cases():
    a, a2, b = inv(0), done(0, "ok"), inv(1)
    two = txn_ops([["w", "x", 1]], [["r", "y", 0], ["r", "x", 1]], [["w", "x", 1], ["w", "x", 3], ["w", "x", 1]], [["r", "x", 1]])
    nem = {"process": "nemesis", "type": "info", "f": "start", "value": None}
    return {
        # name: (history, analyzers, cause, unknown row, (key, value, writer rows) of a multiple-writes error)
        "two-writers-read": (two, ("wr",), A.CAUSE_MULTIPLE_WRITES, 3, ("x", 1, [1, 5])),
        "two-writers-read-after-nemesis": ([nem] + two, ("wr", "realtime"), A.CAUSE_MULTIPLE_WRITES, 4, ("x", 1, [2, 6])),
        "double-invoke": ([a, a, a2], ("realtime",), A.CAUSE_DOUBLE_INVOKE, 1, None),
        "orphan-completion": ([a, a2, a2], ("realtime", "process"), A.CAUSE_ORPHAN, 2, None),
        "unmatched-invoke": ([a, a2, nem, b], ("wr", "realtime"), A.CAUSE_UNMATCHED_INVOKE, 3, None),
    }


UNKNOWN_CASES = _unknown_cases()


def checker_raises(CY, chk, name):
    """chk (a cycle checker over the case's analyzers) raises what the reference
    raises for UNKNOWN_CASES[name], with the row and pair the device names."""
    import pytest
    h, _, cause, row, detail = UNKNOWN_CASES[name]
    with pytest.raises((CY.IllegalArgument, CY.IllegalHistory)) as e:
        chk.check({}, h, {})
    if cause == A.CAUSE_MULTIPLE_WRITES:
        assert isinstance(e.value, CY.IllegalArgument) and isinstance(e.value, ValueError)
        assert (e.value.row, e.value.key, e.value.value, list(e.value.rows)) == (row,) + tuple(detail)
        assert str(e.value).startswith(f"Key :{detail[0]} had value {detail[1]} written by more than one op: ")
    else:
        assert isinstance(e.value, CY.IllegalHistory) and isinstance(e.value, AssertionError)
        assert (e.value.cause, e.value.row) == (A.CAUSES[cause], row)


def analyzers_of(CY, names):
    fns = [getattr(CY, n + "_graph") for n in names]
    return fns[0] if len(fns) == 1 else CY.combine(*fns)
