"""Hand-written histories for the Adya G2 checker (jepsen.tests.adya/g2-checker),
shared by the CPU and the GPU tests. EXPECT pins each result map by hand."""
from jepsen_amd.history import tuple_


def ins(k, type="ok", process=0, ids=(None, 1)):
    return {"process": process, "type": type, "f": "insert", "value": tuple_(k, list(ids))}


def other(f, k=None, type="ok", process=0):
    return {"process": process, "type": type, "f": f, "value": None if k is None else tuple_(k, None)}


def pair(k, a, b, base=0):
    """A key's two inserts, invocations first, completing as a and b."""
    return [ins(k, "invoke", 0, (None, base + 1)), ins(k, "invoke", 1, (base + 2, None)),
            ins(k, a, 0, (None, base + 1)), ins(k, b, 1, (base + 2, None))]


CASES = {
    "empty": [],
    "no-inserts": [other("read", 3), other("start", None, "info", "nemesis")],
    "single-key-legal": pair(7, "ok", "fail"),
    "single-key-illegal": pair(7, "ok", "ok"),
    "ok-counts-0-1-2-3": pair(0, "fail", "info") + pair(1, "ok", "fail") + pair(2, "ok", "ok")
    + pair(3, "ok", "ok") + [ins(3, "ok", 2)],
    "invoke-only": [ins(5, "invoke")],
    "key-only-in-non-inserts": pair(1, "ok", "info") + [other("read", 9), other("delete", 9, "fail")],
    "nemesis-insert": [ins(4, "ok", "nemesis"), ins(4, "invoke", 0), ins(4, "ok", 0)],
    "nemesis-insert-info": [ins(4, "info", "nemesis")],
    # key ids follow first appearance (9, 2, 5): :illegal comes out in key order
    "unsorted-ids": pair(9, "ok", "ok") + pair(2, "ok", "ok") + pair(5, "ok", "ok") + pair(1, "ok", "fail"),
    "string-keys": pair("b", "ok", "ok") + pair("a", "ok", "ok"),
}

EXPECT = {
    "empty": {"valid?": True, "key-count": 0, "legal-count": 0, "illegal-count": 0, "illegal": {}},
    "no-inserts": {"valid?": True, "key-count": 0, "legal-count": 0, "illegal-count": 0, "illegal": {}},
    "single-key-legal": {"valid?": True, "key-count": 1, "legal-count": 1, "illegal-count": 0, "illegal": {}},
    "single-key-illegal": {"valid?": False, "key-count": 1, "legal-count": 0, "illegal-count": 1, "illegal": {7: 2}},
    "ok-counts-0-1-2-3": {"valid?": False, "key-count": 4, "legal-count": 1, "illegal-count": 2, "illegal": {2: 2, 3: 3}},
    "invoke-only": {"valid?": True, "key-count": 1, "legal-count": 0, "illegal-count": 0, "illegal": {}},
    "key-only-in-non-inserts": {"valid?": True, "key-count": 1, "legal-count": 1, "illegal-count": 0, "illegal": {}},
    "nemesis-insert": {"valid?": False, "key-count": 1, "legal-count": 0, "illegal-count": 1, "illegal": {4: 2}},
    "nemesis-insert-info": {"valid?": True, "key-count": 1, "legal-count": 0, "illegal-count": 0, "illegal": {}},
    "unsorted-ids": {"valid?": False, "key-count": 4, "legal-count": 1, "illegal-count": 3, "illegal": {2: 2, 5: 2, 9: 2}},
    "string-keys": {"valid?": False, "key-count": 2, "legal-count": 0, "illegal-count": 2, "illegal": {"a": 2, "b": 2}},
}

# an :insert whose :value is no map entry: the reference throws
UNKEYED = [pair(1, "ok", "fail") + [{"process": 0, "type": "ok", "f": "insert", "value": [3, [None, 9]]}],
           [{"process": 0, "type": "invoke", "f": "insert", "value": None}]]
