"""Hand-written bank histories and their answers (jepsen.tests.bank/checker,
tests/bank.clj:46-121), shared by the CPU restatement tests and the device
tests. Each case: (test map, checker opts, history, the result map written out
by hand). Accounts are 0, 1, 2 and total-amount is 10 unless a case says
otherwise."""

T = {"accounts": [0, 1, 2], "total-amount": 10, "nodes": ["n1", "n2"]}


def inv(p=0, f="read", v=None):
    return {"process": p, "type": "invoke", "f": f, "value": v}


def rd(v, p=0, t="ok"):
    return {"process": p, "type": t, "f": "read", "value": v}


def err(h, i, typ, key, payload):
    """The error map of the read at row i."""
    return {"type": typ, key: payload, "op": dict(h[i], index=i)}


def one(e, **more):
    return dict({"count": 1, "first": e, "worst": e, "last": e}, **more)


CASES = {}

# a valid history: transfers, a failed and a crashed read, a nemesis read of nonsense
h = [inv(), rd({0: 10, 1: 0, 2: 0}), inv(1, "transfer", {"from": 0, "to": 1, "amount": 3}),
     {"process": 1, "type": "ok", "f": "transfer", "value": {"from": 0, "to": 1, "amount": 3}},
     inv(1), rd({0: 7, 1: 3, 2: 0}, 1), inv(2), rd({0: 99}, 2, "fail"), inv(3), rd({0: 99}, 3, "info"),
     {"process": "nemesis", "type": "info", "f": "start", "value": None}, inv(0), rd({2: 4, 0: 3, 1: 3})]
CASES["valid"] = (T, {}, h, {"valid?": True, "read-count": 3, "error-count": 0, "first-error": None, "errors": {}})

CASES["empty"] = (T, {}, [], {"valid?": True, "read-count": 0, "error-count": 0, "first-error": None, "errors": {}})

h = [inv(), rd({0: 5, 7: 5, 1: 0, "x": 0})]
e = err(h, 1, "unexpected-key", "unexpected", [7, "x"])
CASES["unexpected-key"] = (T, {}, h, {"valid?": False, "read-count": 1, "error-count": 1, "first-error": e,
                                       "errors": {"unexpected-key": one(e)}})

h = [inv(), rd({0: 10, 1: None, 2: 0})]
e = err(h, 1, "nil-balance", "nils", {1: None})
CASES["nil-balance"] = (T, {}, h, {"valid?": False, "read-count": 1, "error-count": 1, "first-error": e,
                                    "errors": {"nil-balance": one(e)}})

h = [inv(), rd({0: 5, 1: 4, 2: 0})]
e = err(h, 1, "wrong-total", "total", 9)
CASES["wrong-total"] = (T, {}, h, {"valid?": False, "read-count": 1, "error-count": 1, "first-error": e,
                                    "errors": {"wrong-total": one(e, lowest=e, highest=e)}})

h = [inv(), rd({0: 15, 1: -2, 2: -3})]
e = err(h, 1, "negative-value", "negative", [-2, -3])
CASES["negative-value"] = (T, {}, h, {"valid?": False, "read-count": 1, "error-count": 1, "first-error": e,
                                       "errors": {"negative-value": one(e)}})
CASES["negative-allowed"] = (T, {"negative-balances?": True}, h,
                             {"valid?": True, "read-count": 1, "error-count": 0, "first-error": None, "errors": {}})
# negative balances allowed: the sum is still checked
h = [inv(), rd({0: 15, 1: -2, 2: -4})]
e = err(h, 1, "wrong-total", "total", 9)
CASES["negative-allowed-wrong-total"] = (T, {"negative-balances?": True}, h,
                                         {"valid?": False, "read-count": 1, "error-count": 1, "first-error": e,
                                          "errors": {"wrong-total": one(e, lowest=e, highest=e)}})

# cond priority: an unexpected key, a nil and a wrong sum in one read is an unexpected-key only;
# a nil and a wrong sum (and a negative) is a nil-balance only; a wrong sum with a negative a wrong-total
h = [inv(), rd({9: None, 0: 3}), inv(), rd({0: None, 1: -3}), inv(), rd({0: 12, 1: -3})]
e0, e1, e2 = (err(h, 1, "unexpected-key", "unexpected", [9]), err(h, 3, "nil-balance", "nils", {0: None}),
              err(h, 5, "wrong-total", "total", 9))
CASES["cond-priority"] = (T, {}, h, {"valid?": False, "read-count": 3, "error-count": 3, "first-error": e0,
                                      "errors": {"unexpected-key": one(e0), "nil-balance": one(e1),
                                                 "wrong-total": one(e2, lowest=e2, highest=e2)}})

# a nil :value behaves as the empty map: total 0
h = [inv(), rd(None), inv(1), rd({}, 1)]
e0, e1 = err(h, 1, "wrong-total", "total", 0), err(h, 3, "wrong-total", "total", 0)
CASES["nil-value"] = (T, {}, h, {"valid?": False, "read-count": 2, "error-count": 2, "first-error": e0,
                                  "errors": {"wrong-total": {"count": 2, "first": e0, "worst": e0, "last": e1,
                                                             "lowest": e0, "highest": e0}}})
CASES["nil-value-total-0"] = (dict(T, **{"total-amount": 0}), {}, h,
                              {"valid?": True, "read-count": 2, "error-count": 0, "first-error": None, "errors": {}})

# ties go to the earlier read: worst (|diff| 2 twice, then 1), lowest (8 twice), highest (12 twice);
# unexpected-key badness 2, 1, 2; negative-value badness 4, 4
h = [inv(), rd({0: 8}), inv(), rd({0: 12}), inv(), rd({0: 11}), inv(), rd({0: 12}), inv(), rd({0: 8}),
     inv(), rd({5: 1, 6: 1}), inv(), rd({5: 1}), inv(), rd({7: 1, 8: 1}),
     inv(), rd({0: 14, 1: -4}), inv(), rd({0: 14, 1: -3, 2: -1})]
w = [err(h, i, "wrong-total", "total", t) for i, t in ((1, 8), (3, 12), (5, 11), (7, 12), (9, 8))]
u = [err(h, 11, "unexpected-key", "unexpected", [5, 6]), err(h, 13, "unexpected-key", "unexpected", [5]),
     err(h, 15, "unexpected-key", "unexpected", [7, 8])]
n = [err(h, 17, "negative-value", "negative", [-4]), err(h, 19, "negative-value", "negative", [-3, -1])]
CASES["ties"] = (T, {}, h, {"valid?": False, "read-count": 10, "error-count": 10, "first-error": w[0],
                             "errors": {"wrong-total": {"count": 5, "first": w[0], "worst": w[0], "last": w[4],
                                                        "lowest": w[0], "highest": w[1]},
                                        "unexpected-key": {"count": 3, "first": u[0], "worst": u[0], "last": u[2]},
                                        "negative-value": {"count": 2, "first": n[0], "worst": n[0], "last": n[1]}}})

# :first-error is the error with the smallest :index over all types; worst by count
h = [inv(), rd({0: 10}), inv(), rd({0: 10, 1: None}), inv(), rd({0: 1}), inv(), rd({3: 0}),
     inv(), rd({0: None, 1: None})]
e1, e2, e3, e4 = (err(h, 3, "nil-balance", "nils", {1: None}), err(h, 5, "wrong-total", "total", 1),
                  err(h, 7, "unexpected-key", "unexpected", [3]), err(h, 9, "nil-balance", "nils", {0: None, 1: None}))
CASES["first-error"] = (T, {}, h, {"valid?": False, "read-count": 5, "error-count": 4, "first-error": e1,
                                    "errors": {"nil-balance": {"count": 2, "first": e1, "worst": e4, "last": e4},
                                               "wrong-total": one(e2, lowest=e2, highest=e2),
                                               "unexpected-key": one(e3)}})

# the float badness: |diff| 2^24 and 2^24 + 1 (total-amount 1: an exact long quotient) are one
# float, and so are 2^31 and 2^31 + 1 over 100 (a Ratio); max-by keeps the EARLIER read although
# the later one is further off. :highest still is the larger total.
for name, ta, d in (("float-tie-long", 1, 1 << 24), ("float-tie-ratio", 100, 1 << 31)):
    h = [inv(), rd({0: ta + d}), inv(), rd({0: ta + d + 1}), inv(), rd({0: ta + 5})]
    e0, e1, e2 = (err(h, 1, "wrong-total", "total", ta + d), err(h, 3, "wrong-total", "total", ta + d + 1),
                  err(h, 5, "wrong-total", "total", ta + 5))
    CASES[name] = (dict(T, **{"total-amount": ta}), {}, h,
                   {"valid?": False, "read-count": 3, "error-count": 3, "first-error": e0,
                    "errors": {"wrong-total": {"count": 3, "first": e0, "worst": e0, "last": e2, "lowest": e2,
                                               "highest": e1}}})
# below 2^22 a difference of one is never a tie
h = [inv(), rd({0: 10 + (1 << 22) - 2}), inv(), rd({0: 10 + (1 << 22) - 1})]
e0, e1 = err(h, 1, "wrong-total", "total", 10 + (1 << 22) - 2), err(h, 3, "wrong-total", "total", 10 + (1 << 22) - 1)
CASES["float-no-tie"] = (T, {}, h, {"valid?": False, "read-count": 2, "error-count": 2, "first-error": e0,
                                     "errors": {"wrong-total": {"count": 2, "first": e0, "worst": e1, "last": e1,
                                                                "lowest": e0, "highest": e1}}})

I64_MAX = (1 << 63) - 1
# cases where the reference throws (check-safe turns that into :unknown)
RAISING = {
    # total-amount 0 and two wrong-totals: err-badness divides by zero
    "divide-by-zero": (dict(T, **{"total-amount": 0}), {}, [inv(), rd({0: 1}), inv(), rd({0: 2})]),
    # total - total-amount leaves the longs
    "diff-overflow": (dict(T, **{"total-amount": -10}), {}, [inv(), rd({0: I64_MAX}), inv(), rd({0: 2})]),
    # a prefix of the balances overflows, in map order
    "sum-overflow": (T, {"negative-balances?": True}, [inv(), rd({0: I64_MAX, 1: 1, 2: -1})]),
}
# ... and their neighbours where it does not: a single wrong-total never reaches err-badness
h = [inv(), rd({0: 1})]
e = err(h, 1, "wrong-total", "total", 1)
CASES["one-wrong-total-total-0"] = (dict(T, **{"total-amount": 0}), {}, h,
                                    {"valid?": False, "read-count": 1, "error-count": 1, "first-error": e,
                                     "errors": {"wrong-total": one(e, lowest=e, highest=e)}})
h = [inv(), rd({0: I64_MAX})]
e = err(h, 1, "wrong-total", "total", I64_MAX)
CASES["one-wrong-total-diff-overflow"] = (dict(T, **{"total-amount": -10}), {}, h,
                                          {"valid?": False, "read-count": 1, "error-count": 1, "first-error": e,
                                           "errors": {"wrong-total": one(e, lowest=e, highest=e)}})
# the same multiset in an order whose prefixes stay inside the longs
h = [inv(), rd({0: I64_MAX, 2: -1, 1: 1})]
e = err(h, 1, "wrong-total", "total", I64_MAX)
CASES["no-prefix-overflow"] = (T, {"negative-balances?": True}, h,
                               {"valid?": False, "read-count": 1, "error-count": 1, "first-error": e,
                                "errors": {"wrong-total": one(e, lowest=e, highest=e)}})
# an overflow inside a read that also has a nil (or an unexpected key) is not an error of this checker
h = [inv(), rd({0: I64_MAX, 1: 1, 2: None}), inv(), rd({0: I64_MAX, 1: I64_MAX, 9: 5})]
e0, e1 = err(h, 1, "nil-balance", "nils", {2: None}), err(h, 3, "unexpected-key", "unexpected", [9])
CASES["overflow-beside-nil"] = (T, {}, h, {"valid?": False, "read-count": 2, "error-count": 2, "first-error": e0,
                                            "errors": {"nil-balance": one(e0), "unexpected-key": one(e1)}})
