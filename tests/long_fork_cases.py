"""Small long-fork histories with answers written by hand
(jepsen/src/jepsen/tests/long_fork.clj:158-324). CASES: name -> (n, history,
expected map with :forks as [row_a, row_b]); RAISING: name -> (n, history,
illegal kind, row named). HOST_ONLY: the cases whose reads are not group-for's
aligned key sets: the device answers JH_EUNSUPPORTED and the mirror's host
implementation takes over."""


def R(*kv):
    """A read txn from (key, value) pairs."""
    return [["r", k, v] for k, v in kv]


def W(k, v=1):
    return [["w", k, v]]


def inv(value, p=0, f=None):
    return {"process": p, "type": "invoke", "f": f or ("write" if value and value[0][0] == "w" else "read"),
            "value": value}


def ok(value, p=0, f=None):
    return dict(inv(value, p, f), type="ok")


def counts(reads, early, late, **kw):
    return dict({"reads-count": reads, "early-read-count": early, "late-read-count": late}, **kw)


_N3 = R((0, None), (1, None), (2, None))

CASES = {
    # jepsen/test/jepsen/tests/long_fork_test.clj: r1 sees 1 1 nil, r2 sees 1 nil 1
    "golden": (3, [inv(_N3), inv(R((2, None), (0, None), (1, None)), 1),
                   ok(R((0, 1), (1, 1), (2, None))), ok(R((2, 1), (0, 1), (1, None)), 1)],
               counts(2, 0, 0, **{"valid?": False, "forks": [[2, 3]]})),
    # masks 00 01 01 11 11: a chain with duplicates
    "chain-duplicate-masks": (2, [inv(W(0)), ok(W(0)), ok(R((0, None), (1, None))), ok(R((0, 1), (1, None))),
                                  ok(R((1, None), (0, 1)), 1), inv(W(1), 1), ok(R((0, 1), (1, 1))),
                                  ok(R((1, 1), (0, 1)), 2)],
                              counts(5, 1, 2, **{"valid?": True})),
    # three equal partial masks and nothing else
    "equal-masks": (3, [ok(R((3, 7), (4, None), (5, None))), ok(R((5, None), (3, 7), (4, None)), 1),
                        ok(R((4, None), (5, None), (3, 7)), 2)],
                    counts(3, 0, 0, **{"valid?": True})),
    "early-only": (2, [ok(R((0, None), (1, None))), ok(R((3, None), (2, None)), 1), ok(R((0, None), (1, None)))],
                   counts(3, 3, 0, **{"valid?": True})),
    "late-only": (2, [ok(R((0, 1), (1, 1))), ok(R((3, 1), (2, 1)), 1)], counts(2, 0, 2, **{"valid?": True})),
    # writes of 5, 6, 6, 5: the second 6 (row 3) comes before the second 5 (row 4); :ok and :fail writes do not count
    "repeated-write-earlier-wins": (2, [inv(W(5)), ok(W(5)), inv(W(6), 1), inv(W(6), 2), inv(W(5), 3),
                                        ok(R((4, None), (5, 1)))],
                                    counts(1, 0, 0, **{"valid?": "unknown", "error": ["multiple-writes", 6]})),
    # the repeated write is found first: the wrong-size read (row 2) is never reached
    "repeated-write-hides-wrong-size": (2, [inv(W(0)), ok(W(0)), ok(R((0, 1))), ok(R((0, 1), (1, None))), inv(W(0), 1)],
                                        counts(2, 0, 1, **{"valid?": "unknown", "error": ["multiple-writes", 0]})),
    # an :ok write and a :fail write of a written key are no second invocation
    "completions-are-not-writes": (2, [inv(W(0)), ok(W(0)), {"process": 1, "type": "fail", "f": "write", "value": W(0)},
                                       {"process": 2, "type": "info", "f": "write", "value": W(0)}],
                                   counts(0, 0, 0, **{"valid?": True})),
    # :f is never looked at: a read txn under :f :write, a write txn under :f :read; a mixed txn is neither
    "shape-not-f": (2, [inv(W(0), f="read"), ok(R((0, 1), (1, None)), f="write"), inv(W(0), 1, f="txn"),
                        ok([["r", 0, 1], ["w", 1, 2]], 2, f="read")],
                    counts(1, 0, 0, **{"valid?": "unknown", "error": ["multiple-writes", 0]})),
    "negative-keys": (3, [ok(R((-3, 1), (-2, None), (-1, None))), ok(R((-1, 1), (-3, None), (-2, None)), 1),
                          ok(R((-6, None), (-5, 1), (-4, 1)), 2), ok(R((-4, 1), (-6, None), (-5, None)), 3)],
                      counts(4, 0, 0, **{"valid?": False, "forks": [[0, 1]]})),
    # every read names its keys in another order; masks 011, 110 (keys 9 10 11) fork, 111 is above both
    "shuffled-keys": (3, [ok(R((10, 1), (9, 1), (11, None))), ok(R((11, 1), (9, None), (10, 1)), 1),
                          ok(R((9, 1), (11, 1), (10, 1)), 2)],
                      counts(3, 0, 1, **{"valid?": False, "forks": [[0, 1]]})),
    # two broken groups, the higher keys first in the history: forks come by group, then rows
    "two-groups-in-key-order": (2, [ok(R((4, 1), (5, None))), ok(R((4, None), (5, 1)), 1), ok(R((0, None), (1, 1)), 2),
                                    ok(R((2, 1), (3, 1)), 3), ok(R((1, None), (0, 1)), 4), ok(R((0, None), (1, 1)), 5)],
                                counts(6, 0, 1, **{"valid?": False, "forks": [[2, 4], [4, 5], [0, 1]]})),
    "empty-history": (2, [], counts(0, 0, 0, **{"valid?": True})),
    # non-aligned key sets: the host implementation
    "non-aligned-fork": (2, [ok(R((1, 1), (2, None))), ok(R((2, 1), (1, None)), 1), ok(R((1, 1), (2, 1)), 2)],
                         counts(3, 0, 1, **{"valid?": False, "forks": [[0, 1]]})),
    "non-aligned-valid": (2, [ok(R((1, 1), (7, None))), ok(R((7, 1), (1, 1)), 1)], counts(2, 0, 1, **{"valid?": True})),
}

HOST_ONLY = {"non-aligned-fork", "non-aligned-valid"}

RAISING = {
    "wrong-size": (2, [ok(R((0, 1), (1, None))), ok(R((2, 1), (3, None), (4, None)), 1), ok(R((0, 1)), 2)], 1, 1),
    # an empty txn and a nil :value are reads of no key (early and late at once): a group of size 0
    "empty-read": (2, [ok(R((0, 1), (1, None))), ok([], 1)], 1, 1),
    "nil-read": (2, [ok(R((0, 1), (1, None))), ok(None, 1, f="read"), ok([], 2)], 1, 1),
    # key 0 is 1 in rows 1 and 3 and 2 in row 2 -- the first read holding a value for it is named
    "distinct-values": (2, [ok(R((0, None), (1, 5))), ok(R((0, 1), (1, 5)), 1), ok(R((0, 2), (1, 5)), 2),
                            ok(R((1, 5), (0, 1)), 3)], 2, 1),
}

# the counts of the :multiple-writes case over an empty and a nil read, which the error hides
CASES["repeated-write-over-empty-reads"] = (
    2, [inv(W(3)), ok([], 1), ok(None, 2, f="read"), inv(W(3), 1)],
    counts(2, 2, 2, **{"valid?": "unknown", "error": ["multiple-writes", 3]}))
