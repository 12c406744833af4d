"""Hand-written causal-reverse histories (op maps, one key each) shared by the
CPU and the GPU tests. Reads are Clojure vectors (lists) unless a case says
otherwise; what each must give is computed by the literal transcription
(causal_reverse_ref.clj_check), except where a test pins it by hand."""
import random

I64_MAX = (1 << 63) - 1
I64_MIN = -(1 << 63)


def op(t, f, v, p=0):
    return {"process": p, "type": t, "f": f, "value": v}


def wi(v, p=0): return op("invoke", "write", v, p)      # noqa: E704
def wo(v, p=0): return op("ok", "write", v, p)          # noqa: E704
def rd(v, p=1): return op("ok", "read", v, p)           # noqa: E704
def ri(p=1): return op("invoke", "read", None, p)       # noqa: E704


def seq(*vs):
    """Writes that complete one after the other."""
    out = []
    for v in vs:
        out += [wi(v), wo(v)]
    return out


CASES = {
    "empty": [],
    "no-reads": seq(1, 2, 3),
    "no-writes": [ri(), rd([1, 2]), rd([])],
    "read-nil": seq(1, 2) + [ri(), rd(None)],
    "read-empty": seq(1, 2) + [ri(), rd([])],
    # 7 and 8 complete without an invoke: a read of them alone expects nothing
    "never-invoked-only": [wo(7), wo(8)] + seq(1, 2) + [rd([7, 8]), rd([7])],
    # the last invoke of 9 comes after 1 completed: [9] misses 1; the first invoke alone would expect nothing
    "invoked-twice-last-counts": [wi(9), wi(1), wo(1), wi(9, 2), rd([9]), wo(9)],
    # the same graph, read with what the last invoke expects: valid
    "invoked-twice-satisfied": [wi(9), wi(1), wo(1), wi(9, 2), rd([9, 1]), wo(9)],
    # the max is over the seen values' last invokes: 9's first invoke must not hide behind 5's later one
    "invoked-twice-with-another": [wi(9), wi(1), wo(1), wi(5), wi(2), wo(2), wi(9, 2), rd([5]), rd([9, 5]), rd([9, 5, 1])],
    # 1 completes at row 1 and again at row 3, 2 is invoked between: the first ok counts, [2] misses 1
    "ok-twice-first-counts": [wi(1), wo(1), wi(2), wo(1), rd([2])],
    # the other way round: were the second ok the one that counts, [2] would miss 1
    "ok-twice-second-is-late": [wi(1), wi(2), wo(2), wo(1), wi(3), wo(1), rd([2]), rd([3])],
    "ok-never-invoked": [wo(7)] + seq(1) + [rd([1]), rd([1, 7])],
    "fail-and-info-writes": [wi(1), op("fail", "write", 1), wi(2), op("info", "write", 2), wi(3), wo(3), wi(4), wo(4),
                             rd([4]), rd([3, 4]), rd([4, 1, 2])],
    "write-by-nemesis": [wi(1, "nemesis"), wo(1, "nemesis"), wi(2), wo(2), rd([2]), rd([1, 2])],
    "reads-of-other-types": seq(1, 2) + [op("invoke", "read", [2]), op("fail", "read", [2]), op("info", "read", [2]), rd([2, 1])],
    "read-before-every-write": [rd([2]), rd([1])] + seq(1, 2),
    # strictness of first_ok < M: ok at row r, the deciding invoke at row r + 1
    "strict-ok-then-invoke": [wi(1), wo(1), wi(2), rd([2])],
    # ... and with the two rows swapped: not expected
    "strict-invoke-then-ok": [wi(1), wi(2), wo(1), rd([2])],
    # the index test of set/difference on a vector: seen = [5 3], expected = #{3}
    "vector-quirk": seq(3, 5) + [rd([5, 3])],
    # 3 three times and 1, missing 2: a set read of {1 3}; as a vector the index test hides 2
    "repeated-element": seq(1, 2, 3) + [rd([3, 3, 3, 1])],
    "extreme-values": seq(-1, I64_MAX, I64_MIN + 1, 0) + [rd([0]), rd([0, -1, I64_MAX]), rd([I64_MIN + 1, 0]),
                                                        rd([0, I64_MIN + 1, -1, I64_MAX])],
    "set-reads": seq(1, 2, 3) + [rd(frozenset([3])), rd({1, 2, 3}), rd(frozenset())],
}

# what the issue pins by hand for the quirk case
QUIRK_HOST = {"valid?": False, "errors": [{"process": 1, "type": "ok", "f": "read", "missing": [3], "expected-count": 1}]}
QUIRK_AS_SETS = {"valid?": True, "errors": []}


def edge(c, drop):
    """c writes 100 .. 100 + c - 1 complete in order, then 5 is written: reads
    of all of them with 5 (c + 1 elements, valid), and of all but the one of
    rank `drop` with 5 (c elements, expected-count c, one missing)."""
    vs = list(range(100, 100 + c))
    some = vs[:drop] + vs[drop + 1:]
    return seq(*vs) + seq(5) + [rd(vs + [5]), rd([5] + some[::-1]), rd(some + [5, 5])]


def random_key(seed, n_ops=40):
    """An adversarial key of at most n_ops rows: few values, so that repeated
    invokes and oks, oks without invokes, :fail / :info writes and reads of
    unknown and repeated values all occur; reads land anywhere."""
    rng = random.Random(seed)
    vals = list(range(rng.randint(1, 6)))
    out = []
    for _ in range(rng.randint(0, n_ops)):
        x = rng.random()
        p = rng.randint(0, 3)
        if x < 0.55:
            out.append(op(rng.choice(["invoke", "invoke", "ok", "ok", "ok", "fail", "info"]), "write", rng.choice(vals), p))
        elif x < 0.9:
            seen = [rng.choice(vals + [9]) for _ in range(rng.randint(0, 5))]
            out.append(rd(seen if rng.random() < 0.9 else None, p))
        else:
            out.append(op(rng.choice(["invoke", "fail", "info"]), "read", None, p))
    return out
