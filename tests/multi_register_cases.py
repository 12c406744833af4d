"""Hand cases for linearizability over the multi-register model (not a test
module): (name, initial map, keyed op maps). test_multi_register_ref.py holds
the host path against the reference on every one, test_gpu_multi_register.py
the device."""
from jepsen_amd.history import tuple_


def inv(p, txn, k=0, f="txn"):
    return {"process": p, "type": "invoke", "f": f, "value": tuple_(k, txn)}


def ok(p, txn, k=0, f="txn"):
    return {"process": p, "type": "ok", "f": f, "value": tuple_(k, txn)}


def fail(p, txn, k=0, f="txn"):
    return {"process": p, "type": "fail", "f": f, "value": tuple_(k, txn)}


def info(p, txn, k=0, f="txn"):
    return {"process": p, "type": "info", "f": f, "value": tuple_(k, txn)}


def seq(*txns, k=0, p=0):
    """Ops one after the other on one process, each :ok with its own txn."""
    out = []
    for t in txns:
        out += [inv(p, t, k), ok(p, t, k)]
    return out


def W(r, v):
    return ["w", r, v]


def R(r, v):
    return ["r", r, v]


def crashed_writers(n, k=0, reg=0, first_p=100):
    return [inv(first_p + i, [W(reg, 1 + i % 2)], k) for i in range(n)]


def _cases():
    c = []
    # txn forms
    c.append(("reads-own-write", {}, seq([W(0, 1), R(0, 1)], [W(0, 2)], [W(0, 1), R(0, 1)])))
    c.append(("reads-other-than-own-write", {}, seq([W(0, 1), R(0, 2)])))
    c.append(("own-write-from-any-state", {0: 2}, seq([R(0, 2)], [W(0, 1), R(0, 1)], [R(0, 1)])))
    c.append(("two-different-reads-of-one-register", {}, seq([W(0, 1)], [R(0, 1), R(0, 2)])))
    c.append(("two-equal-reads-of-one-register", {}, seq([W(0, 1)], [R(0, 1), R(0, 1)])))
    c.append(("nil-read-of-never-written", {}, seq([R(0, None)], [W(1, 3)], [R(0, None), R(1, 3)])))
    c.append(("non-nil-read-of-never-written", {}, seq([R(0, 1)])))
    c.append(("nil-write-then-read-nil", {}, seq([W(0, 1)], [W(0, None)], [R(0, None)], [W(0, None), R(0, None)])))
    c.append(("nil-write-then-non-nil-read", {}, seq([W(0, 1)], [W(0, None)], [R(0, 1)])))
    c.append(("nil-write-then-own-non-nil-read", {}, seq([W(0, None), R(0, 1)])))
    c.append(("init-read", {0: 4, 2: 1}, seq([R(0, 4), R(2, 1), R(1, None)], [W(0, 1)], [R(0, 1), R(2, 1)])))
    c.append(("init-read-wrong", {0: 4, 2: 1}, seq([R(0, 4)], [R(2, 4)])))
    c.append(("init-only-register", {7: 3}, seq([W(0, 1)], [R(0, 1)])))
    c.append(("completion-fills-reads", {}, [inv(0, [W(0, 1)]), ok(0, [W(0, 1)]), inv(1, [R(0, None)]), ok(1, [R(0, 1)]),
                                              inv(1, [R(0, None)]), ok(1, [R(0, 2)])]))
    c.append(("nil-completion-keeps-invocation", {}, [inv(0, [W(0, 1)]), ok(0, None), inv(1, [R(0, 2)]), ok(1, None)]))
    # concurrency
    c.append(("concurrent-writes-either-order", {},
              [inv(0, [W(0, 1), W(1, 1)]), inv(1, [W(0, 2), W(1, 2)]), ok(0, [W(0, 1), W(1, 1)]), ok(1, [W(0, 2), W(1, 2)]),
               inv(2, [R(0, None), R(1, None)]), ok(2, [R(0, 1), R(1, 1)])]))
    c.append(("torn-read", {},
              [inv(0, [W(0, 1), W(1, 1)]), inv(1, [W(0, 2), W(1, 2)]), ok(0, [W(0, 1), W(1, 1)]), ok(1, [W(0, 2), W(1, 2)]),
               inv(2, [R(0, None), R(1, None)]), ok(2, [R(0, 1), R(1, 2)])]))
    # crashed and dropped ops
    c.append(("valid-only-if-crashed-write-took-effect", {}, [inv(0, [W(0, 1)]), info(0, [W(0, 1)])] + seq([R(0, 1)], p=1)))
    c.append(("valid-only-if-crashed-write-never-did", {},
              [inv(0, [W(0, 1)]), info(0, None)] + seq([W(0, 2)], [R(0, 2)], [W(1, 1)], [R(0, 2), R(1, 1)], p=1)))
    c.append(("crashed-txn-that-can-never-step", {},
              seq([W(0, 2)], p=1) + [inv(0, [W(0, 1), R(0, 2)]), info(0, None)] + seq([R(0, 2)], p=1)))
    c.append(("crashed-write-after-the-read", {}, seq([W(0, 2)], [R(0, 1)], p=1) + [inv(0, [W(0, 1)])]))
    c.append(("crashed-read-and-failed-write-dropped", {},
              [inv(0, [R(0, 5)]), info(0, [R(0, 5)]), inv(1, [W(0, 3)]), fail(1, [W(0, 3)])] + seq([R(0, None)], p=2) +
              seq([W(0, 1)], [R(0, 1)], p=2)))
    c.append(("failed-op-with-another-f", {}, [inv(1, [["x", 0, 3]]), fail(1, [["x", 0, 3]])] + seq([W(0, 1)], [R(0, 1)], p=2)))
    c.append(("no-ok-op", {}, [inv(0, [W(0, 1)]), info(0, [W(0, 1)]), inv(1, [W(0, 2)]), fail(1, [W(0, 2)]), inv(2, [W(1, 1)])]))
    c.append(("only-identity-ops", {}, seq([R(0, None)], [R(1, None), R(0, None)], [])))
    c.append(("nemesis-only-key", {},
              seq([W(0, 1)], k=0) + [{"process": "nemesis", "type": "info", "f": "start", "value": tuple_(5, None)},
                                     {"process": "nemesis", "type": "info", "f": "stop", "value": None}]))
    c.append(("empty", {}, []))
    # illegal histories: one key of three
    c.append(("double-invoke-in-one-key-of-three", {},
              seq([W(0, 1)], [R(0, 1)], k=0) + [inv(3, [W(0, 1)], 1), inv(3, [W(0, 2)], 1), ok(3, [W(0, 2)], 1)] +
              seq([W(0, 1)], [R(0, 2)], k=2)))
    c.append(("orphan-completion-in-one-key-of-three", {},
              seq([W(0, 1)], [R(0, 1)], k=0) + [ok(3, [W(0, 2)], 1)] + seq([W(0, 1)], k=1) + seq([W(0, 1)], [R(0, 2)], k=2)))
    c.append(("orphan-then-double-invoke", {}, [ok(3, [W(0, 2)]), inv(4, [W(0, 1)]), inv(4, [W(0, 1)])]))
    # limits
    for n in (63, 64, 65):
        c.append((f"{n}-crashed-writers-open-at-one-return", {},
                  crashed_writers(n, k=0) + seq([W(1, 1)], [R(1, 1)], k=0) + seq([W(0, 1)], [R(0, 1)], k=1)))
    c.append(("64-crashed-writers-one-needed", {}, crashed_writers(64, reg=1) + seq([W(0, 3)], [R(1, 2), R(0, 3)], [R(1, 1)])))
    c.append(("packed-state-32-bits", {},
              seq(*[[W(r, 1 + (r + i) % 15)] for r in range(8) for i in range(15)]) +
              seq([R(r, 1 + (r + 14) % 15) for r in range(8)], [R(7, 1)])))
    c.append(("64-micro-op-txn", {}, seq([W(i % 3, 1 + i % 4) for i in range(63)] + [R(2, 1 + 62 % 4)], [R(0, 1 + 60 % 4)])))
    return c


CASES = _cases()
# what the device answers JH_EUNSUPPORTED to: the host path gives the map
UNSUPPORTED = [
    ("packed-state-33-bits", {},       # 11 registers of 3 bits
     seq(*[[W(r, 1 + (r + i) % 7)] for r in range(11) for i in range(7)]) + seq([R(10, 1 + 16 % 7), R(0, 7)], [R(10, 2)])),
    ("65-micro-op-txn", {}, seq([W(i % 3, 1 + i % 4) for i in range(64)] + [R(0, 1 + 63 % 4)], [R(0, 2)])),
]
