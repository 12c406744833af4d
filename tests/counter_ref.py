"""CPU restatement of (checker/counter), jepsen/src/jepsen/checker.clj:679-734,
written from its definition over op maps (dicts and lists only; not a test
module). The loop is the reference's loop: lower / upper, the pending reads
by process, the finished [lower value upper] triples.

knossos.history/complete is not vendored. Its part here follows the
conventions oracle/jh_oracle.c documents, which the device follows as well:

  - an invocation's completion is the next non-:info row of its process; the
    invocation takes (or its-own-value completion's-value), and :fails? when
    that completion is a :fail;
  - an :invoke by a process that still has an invocation open, and an :ok or
    :fail with none open, throw in knossos: {:valid? :unknown} (check-safe,
    checker.clj:77-88) with the cause double-invoke / orphan-completion;
  - an :ok :read with no pending read of its process, (+ n nil) and
    (<= a nil b) throw: :unknown with the cause orphan-completion / nil-value
    / nil-value; (+ a b) past a long throws: :unknown, cause overflow.

`check(ops)` returns the fields the C ABI returns (jh_check_counter):
valid, cause, reads, n_reads, n_errors, first_err_entry.
"""
from jepsen_amd import _abi as A

CAUSE = {name: code for code, name in A.CAUSES.items()}
LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1


class Unknown(Exception):
    def __init__(self, cause):
        super().__init__(cause)
        self.cause = cause


def complete(history):
    """history/complete as the counter uses it: a copy of the op maps, each
    with its :index; invocations carry the completed :value and :fails?."""
    out = [dict(op, index=i) for i, op in enumerate(history)]
    open_ = {}                                  # process -> its open invocation
    for op in out:
        p, t = op.get("process"), op.get("type")
        if t == "invoke":
            if p in open_:
                raise Unknown("double-invoke")
            open_[p] = op
        elif t in ("ok", "fail"):
            if p not in open_:
                raise Unknown("orphan-completion")
            inv = open_.pop(p)
            if inv.get("value") is None:
                inv["value"] = op.get("value")
            if t == "fail":
                inv["fails?"] = True
    return out


def _plus(a, b):
    if a is None or b is None:
        raise Unknown("nil-value")
    s = a + b
    if not LONG_MIN <= s <= LONG_MAX:
        raise Unknown("overflow")
    return s


def loop(history):
    """checker.clj:698-734. Returns (reads, the :ok :read row of each)."""
    history = [op for op in complete(history) if not op.get("fails?")]
    history = [op for op in history if op.get("type") != "fail"]
    lower, upper, pending, reads, rows = 0, 0, {}, [], []
    for op in history:
        case = (op.get("type"), op.get("f"))
        if case == ("invoke", "read"):
            pending[op.get("process")] = [lower, op.get("value")]
        elif case == ("ok", "read"):
            r = pending.pop(op.get("process"), None)
            if r is None:
                raise Unknown("orphan-completion")      # (conj nil upper): no [lower value] to finish
            if r[1] is None:
                r[1] = op.get("value")                  # a completed history's invocation has it already
            reads.append(r + [upper])
            rows.append(op["index"])
        elif case == ("invoke", "add"):
            upper = _plus(upper, op.get("value"))
        elif case == ("ok", "add"):
            lower = _plus(lower, op.get("value"))
    return reads, rows


def check(ops):
    out = {"valid": A.VALID, "cause": 0, "reads": [], "n_reads": 0, "n_errors": 0, "first_err_entry": -1}
    try:
        reads, rows = loop(ops)
    except Unknown as e:
        out.update(valid=A.UNKNOWN, cause=CAUSE[e.cause])
        return out
    out["reads"], out["n_reads"] = reads, len(reads)
    for (lo, v, hi), row in zip(reads, rows):
        if v is None:
            # (remove (partial apply <=) reads) throws at this triple
            out.update(valid=A.UNKNOWN, cause=CAUSE["nil-value"])
            return out
        if not lo <= v <= hi:
            if out["n_errors"] == 0:
                out["first_err_entry"] = row
            out["n_errors"] += 1
    out["valid"] = A.INVALID if out["n_errors"] else A.VALID
    return out


def result_map(ops):
    """The reference's result map ({:valid? :reads :errors}); raises Unknown
    where the reference throws."""
    reads, _ = loop(ops)
    if any(r[1] is None for r in reads):
        raise Unknown("nil-value")
    errors = [r for r in reads if not r[0] <= r[1] <= r[2]]
    return {"valid?": not errors, "reads": reads, "errors": errors}


def same(ref, c, what=""):
    """Asserts that every field of a counter result (the C oracle's or the
    device's) equals `ref`, a result of check()."""
    for k in ("valid", "cause", "n_reads", "n_errors", "first_err_entry"):
        assert ref[k] == c[k], (what, k, ref[k], c[k])
    nil = [[A.NIL if x is None else x for x in t] for t in ref["reads"]]      # a nil read value, as the ABI encodes it
    got = [[int(x) for x in t] for t in c["reads"]]
    assert nil == got, what
