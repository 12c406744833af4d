"""Hand-written histories for (independent/checker (checker/set)) (not a test
module). CASES: name -> a keyed history, its keys interleaved row by row with
:nemesis :info rows between the rounds; every case carries a plain valid key
"v" next to the keys it is about. UNKEYED: name -> a history without tuples
(one key for the raw call, no key at all for independent/checker)."""
from jepsen_amd.history import tuple_

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def ia(x, p=0):
    return {"process": p, "type": "invoke", "f": "add", "value": x}


def oa(x, p=0):
    return {"process": p, "type": "ok", "f": "add", "value": x}


def fa(x, p=0):
    return {"process": p, "type": "fail", "f": "add", "value": x}


def na(x, p=0):
    return {"process": p, "type": "info", "f": "add", "value": x}


def ir(p=1):
    return {"process": p, "type": "invoke", "f": "read", "value": None}


def rd(v, p=1):
    return {"process": p, "type": "ok", "f": "read", "value": v}


def nem(f="start"):
    return {"process": "nemesis", "type": "info", "f": f, "value": None}


def added(xs):
    """Every element invoked and acknowledged."""
    out = []
    for x in xs:
        out += [ia(x), oa(x)]
    return out


def keyed(subs, nemesis=True):
    """{key: ops} -> one history: the keys interleaved row by row, a :nemesis
    :info row after every round."""
    out = []
    for i in range(max(len(s) for s in subs.values())):
        for k, s in subs.items():
            if i < len(s):
                out.append(dict(s[i], value=tuple_(k, s[i]["value"])))
        if nemesis:
            out.append(nem("start" if i % 2 == 0 else "stop"))
    return out


VALID = added([1, 2, 3]) + [ir(), rd({1, 2, 3})]

KEYS = {
    "valid": {"a": added(range(10)) + [ir(), rd(set(range(10)))]},
    "lost": {"a": added([1, 2]) + [ir(), rd({1})]},
    "unexpected": {"a": added([1]) + [ir(), rd({1, 9})]},
    "lost-and-unexpected": {"a": added([1, 2]) + [ir(), rd({2, 7})]},
    "recovered": {"a": added([1]) + [ia(5), na(5), ir(), rd({1, 5})]},
    "failed-add-read": {"a": added([1]) + [ia(4), fa(4), ir(), rd({1, 4})]},
    "never-read": {"a": added([1, 2]) + [ir(), {"process": 1, "type": "fail", "f": "read", "value": None}]},
    "nil-after-a-read": {"a": added([1, 2]) + [ir(), rd({1, 2}), ir(), rd(None)]},
    "empty-read": {"a": added([1, 2]) + [ir(), rd(set())]},
    "empty-read-no-adds": {"a": [ir(), rd([])]},
    "later-read-smaller": {"a": added([1, 2, 3]) + [ir(), rd({1, 2, 3}), ir(), rd({2})]},
    "adds-after-the-read": {"a": added([1]) + [ir(), rd({1, 2}), ia(2), oa(2), ia(3), oa(3)]},
    "only-a-fail": {"a": [fa(1)]},
    "repeated-element": {"a": added([1, 2]) + [ir(), rd([1, 1, 2, 1])]},
    "vector-descending": {"a": added([1, 2, 3, 4]) + [ir(), rd([4, 3, 1])]},
    "negative": {"a": added([-5, -4, -3, -1]) + [ir(), rd({-5, -3, -2})]},
    "base-not-word-aligned": {"a": added(range(37, 71)) + [ir(), rd(set(range(37, 70)) | {75})]},
    "extremes": {"lo": added([I64_MIN + 1]) + [ir(), rd({I64_MIN + 1})], "hi": added([I64_MAX]) + [ir(), rd(set())]},
    "invoke-by-one-ack-by-another": {"a": [ia(1, 0), oa(1, 3), ia(2, 0), ir(), rd({1})]},
}
CASES = {name: keyed(dict(subs, v=VALID)) for name, subs in KEYS.items()}
# every key of every case in one history
CASES["all"] = keyed({f"{name}/{k}": ops for name, subs in KEYS.items() for k, ops in subs.items()})
# key order and nemesis rows must not matter
CASES["valid-key-first"] = keyed({"v": VALID, "a": KEYS["lost"]["a"], "b": KEYS["unexpected"]["a"]}, nemesis=False)

UNKEYED = {
    "unkeyed-valid": VALID,
    "unkeyed-lost-and-unexpected": [nem()] + KEYS["lost-and-unexpected"]["a"] + [nem("stop")],
    "unkeyed-never-read": KEYS["never-read"]["a"],
    "unkeyed-base-not-word-aligned": KEYS["base-not-word-aligned"]["a"],
}
