"""jepsen.tests.bank on MI355X: the bank workload's checker (snapshot
isolation: every read of all accounts sums to :total-amount) and the data of
its plot.

Mirrors jepsen/src/jepsen/tests/bank.clj (names, argument meaning, result
maps, error behaviour). A read's :value is a dict {account: balance}; its
insertion order stands for (seq (:value op)).

Encoding (include/jh.h, "Bank reads"): an :ok :read row has value = the index
of its first pair in aux, value2 = its number of pairs; pair j is
aux[2*(value+j)] (account code) and aux[2*(value+j)+1] (balance, NIL = nil).
A nil :value is value = NIL, value2 = 0. Account code i is the i-th distinct
element of (:accounts test); any other key gets a code >= n_accounts in
first-appearance order. Rows of other f carry value = value2 = NIL.
Balances that are not integers or nil have no encoding: TypeError.

The reference tree has no bank test and no recorded bank result: parity is
unpinned against the reference's own tests.
"""
import decimal
from fractions import Fraction

import numpy as np

from . import _abi as A
from . import history as H

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TYPES = A.BANK_TYPES
PAYLOAD = {"unexpected-key": "unexpected", "nil-balance": "nils", "wrong-total": "total",
           "negative-value": "negative"}


def _long(x):
    """Clojure's checked long arithmetic: + and - throw on overflow."""
    if not I64_MIN <= x <= I64_MAX:
        raise ArithmeticError("integer overflow")
    return x


def _sum(xs):
    """(reduce + xs) on longs: sequential, throws as soon as a prefix overflows."""
    s = 0
    for x in xs:
        s = _long(s + x)
    return s


def _f32(q):
    """The 32-bit float nearest to a rational (ties to even), as a Fraction:
    what a narrowing conversion gives."""
    q = Fraction(q)
    if q == 0:
        return q
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    e = max(e, -126)                       # subnormals keep the smallest exponent
    ulp = Fraction(2) ** (e - 23)
    k = q / ulp
    n = k.numerator // k.denominator
    rem = k - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return sign * n * ulp                  # past 2^128 this is infinity in Java; never reached from longs


def ratio_float(num, den):
    """(float (/ num den)) on longs, as clojure.lang.Ratio does it: an exact
    quotient stays a long and narrows directly; otherwise Ratio.floatValue is
    (float) doubleValue, and doubleValue divides as BigDecimals under
    MathContext/DECIMAL64 (16 digits, half-even) before going to double."""
    if den == 0:
        raise ArithmeticError("Divide by zero")
    if num % den == 0:
        return _f32(num // den)
    with decimal.localcontext() as c:
        c.prec = 16
        c.rounding = decimal.ROUND_HALF_EVEN
        d = decimal.Decimal(num) / decimal.Decimal(den)
    return _f32(Fraction(float(d)))        # float(Decimal) is correctly rounded, as BigDecimal.doubleValue


def err_badness(test, err):
    """bank.clj:46-55: bigger numbers mean more egregious errors."""
    t = err["type"]
    if t == "unexpected-key":
        return len(err["unexpected"])
    if t == "nil-balance":
        return len(err["nils"])
    if t == "wrong-total":
        ta = test["total-amount"]
        return abs(ratio_float(_long(err["total"] - ta), ta))
    if t == "negative-value":
        return _long(-_sum(err["negative"]))
    raise ValueError(f"no bank error type {t!r}")


def check_op(accts, total, negative_balances, op):
    """bank.clj:57-82: the first matching error of one read, or None."""
    v = op.get("value") or {}
    ks, balances = list(v.keys()), list(v.values())
    if not all(k in accts for k in ks):
        return {"type": "unexpected-key", "unexpected": [k for k in ks if k not in accts], "op": op}
    if any(b is None for b in balances):
        return {"type": "nil-balance", "nils": {k: b for k, b in v.items() if b is None}, "op": op}
    s = _sum(balances)
    if total != s:
        return {"type": "wrong-total", "total": s, "op": op}
    if not negative_balances and any(b < 0 for b in balances):
        return {"type": "negative-value", "negative": [b for b in balances if b < 0], "op": op}
    return None


def _distinct(xs):
    out, seen = [], set()
    for x in xs:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return out


def encode(history, accounts):
    """Op maps -> (Columns, account table). table[code] is the account; the
    first len(distinct(accounts)) codes are (:accounts test) in order, the rest
    are the unexpected keys in first-appearance order. The table is also the
    Columns' value_table."""
    history = list(history)
    n = len(history)
    proc = np.empty(n, np.int64)
    typ = np.empty(n, np.int64)
    fcol = np.empty(n, np.int64)
    val = np.full(n, A.NIL, np.int64)
    val2 = np.full(n, A.NIL, np.int64)
    table = _distinct(accounts)
    code = {k: i for i, k in enumerate(table)}
    aux = []
    f_ids, f_names, other_procs = {}, [], {"nemesis": -1}
    for i, op in enumerate(history):
        p = op.get("process")
        if H._is_int(p) and p >= 0:
            proc[i] = int(p)
        else:
            if p not in other_procs:
                other_procs[p] = -1 - len(other_procs)
            proc[i] = other_procs[p]
        t = op.get("type")
        if t not in H.TYPES:
            raise ValueError(f"unknown :type {t!r} in op {op!r}")
        typ[i] = H.TYPES[t]
        f = op.get("f")
        if f in H.KNOWN_F:
            fcol[i] = H.KNOWN_F[f]
        else:
            if f not in f_ids:
                f_ids[f] = A.F_FIRST_INTERNED + len(f_names)
                f_names.append(f)
            fcol[i] = f_ids[f]
        if not (t == "ok" and f == "read"):
            continue
        v = op.get("value")
        if v is None:
            val2[i] = 0
            continue
        if not isinstance(v, dict):
            raise TypeError(f"bank: the :value of a read is a map of account to balance, not {v!r}")
        val[i] = len(aux) // 2
        val2[i] = len(v)
        for k, b in v.items():
            if k not in code:
                code[k] = len(table)
                table.append(k)
            if b is None:
                b = A.NIL
            elif not H._is_int(b):
                raise TypeError(f"bank: balance {b!r} of account {k!r} is not an integer or nil")
            elif not I64_MIN < b <= I64_MAX:
                raise OverflowError(f"bank: balance {b!r} is not a long (or collides with the nil sentinel)")
            aux += [code[k], int(b)]
    cols = H.Columns(n=n, process=proc, type=typ, f=fcol, key=np.full(n, -1, np.int64), value=val, value2=val2,
                     n_keys=0, aux=np.asarray(aux, np.int64).reshape(-1), f_names=f_names, value_table=table)
    return cols, table


def is_read(cols):
    return (np.asarray(cols.type) == A.TYPE_OK) & (np.asarray(cols.f) == A.F_READ)


def decode_op(cols, i, table=None):
    """One row back to an op map (:index included); a read gets its map back,
    any other row a nil :value (the encoding keeps nothing else)."""
    table = cols.value_table if table is None else table
    p, fi = int(cols.process[i]), int(cols.f[i])
    inv_f = {v: k for k, v in H.KNOWN_F.items()}
    op = {"process": p if p >= 0 else ("nemesis" if p == -1 else p), "type": H.TYPE_NAMES[int(cols.type[i])],
          "f": inv_f.get(fi, cols.f_names[fi - A.F_FIRST_INTERNED] if 0 <= fi - A.F_FIRST_INTERNED < len(cols.f_names)
                         else fi),
          "value": None, "index": int(i)}
    if op["type"] == "ok" and op["f"] == "read" and int(cols.value[i]) != A.NIL:
        s, c = int(cols.value[i]), int(cols.value2[i])
        pairs = np.asarray(cols.aux[2 * s:2 * (s + c)]).reshape(-1, 2).tolist()
        op["value"] = {(table[k] if 0 <= k < len(table) else ("unknown-account", k)): (None if b == A.NIL else b)
                       for k, b in pairs}
    return op


def decode(cols, table=None):
    return [decode_op(cols, i, table) for i in range(cols.n)]


def _prepare(test, history):
    """(cols, ops or None, n_accounts)."""
    accounts = _distinct(test["accounts"])
    if isinstance(history, H.Columns):
        return history, None, len(accounts)
    ops = list(history)
    cols, _ = encode(ops, accounts)
    return cols, ops, len(accounts)


def _op_at(cols, ops, row):
    if ops is not None:
        op = dict(ops[row])
        op.setdefault("index", int(row))
        return op
    return decode_op(cols, int(row))


class BankChecker:
    """(bank/checker checker-opts), bank.clj:84-121, through jh_check_bank.
    check(test, history, opts): test has "accounts" and "total-amount"; history
    is op maps, or Columns from `encode` (their value_table is the account
    table). :first / :worst / :last / :lowest / :highest / :first-error are
    rebuilt on the host by check_op from the few rows the device names."""

    def __init__(self, checker_opts=None):
        o = checker_opts or {}
        self.negative_balances = bool(o.get("negative-balances?"))

    def check(self, test, history, opts):
        from . import checker as K
        cols, ops, n_acc = _prepare(test, history)
        accts, total = set(test["accounts"]), test["total-amount"]
        ctx = K._ctx()
        r = ctx.check_bank(cols, n_acc, total, self.negative_balances, reads_cap=0)
        if r["valid"] == A.UNKNOWN:
            raise ArithmeticError(f"bank check failed: integer {A.CAUSES.get(r['cause'])}")

        def err(row):
            return check_op(accts, total, self.negative_balances, _op_at(cols, ops, row))

        errors = []
        for t, e in zip(TYPES, r["errors"]):
            if e["count"] == 0:
                continue
            m = {"count": int(e["count"]), "first": err(e["first_row"]), "worst": err(e["worst_row"]),
                 "last": err(e["last_row"])}
            if t == "wrong-total":
                if e["count"] >= 2:
                    m["worst"] = err(self._worst_total(ctx, cols, n_acc, total, e))
                m["lowest"], m["highest"] = err(e["lowest_row"]), err(e["highest_row"])
            errors.append((e["first_row"], t, m))
        errors.sort(key=lambda x: x[0])                    # group-by: types in order of first appearance
        return {"valid?": r["error_count"] == 0,
                "read-count": int(r["read_count"]),
                "error-count": int(r["error_count"]),
                "first-error": err(r["first_error_row"]) if r["error_count"] else None,
                "errors": {t: m for _, t, m in errors}}

    def _worst_total(self, ctx, cols, n_acc, total, e):
        """The row of :worst among two or more wrong-totals. max-by calls
        err-badness on every one of them, so a zero total-amount or a
        difference that is not a long throws. The device ranks by exact |diff|;
        from 2^22 on distinct diffs can share a float, so the float badness is
        recomputed from the triples, the earlier read winning a tie."""
        if total == 0:
            raise ArithmeticError("Divide by zero")
        worst = e["worst_badness"] & ((1 << 64) - 1)       # unsigned
        if worst < A.BANK_FLOAT_EXACT:
            return e["worst_row"]
        reads = ctx.check_bank(cols, n_acc, total, self.negative_balances)["reads"]
        best = best_row = None
        for row, tot, cls in reads[(reads[:, 2] & 7) == 3].tolist():
            b = abs(ratio_float(_long(tot - total), total))
            if best is None or b > best:
                best, best_row = b, row
        return best_row


def checker(checker_opts=None):
    return BankChecker(checker_opts)


def ok_reads(history):
    """bank.clj:123-130."""
    h = [op for op in history if op.get("type") == "ok" and op.get("f") == "read"]
    return h or None


def points(test, history):
    """The data of bank/plotter (bank.clj:132-177), from the device's triples:
    {node: [[seconds, total of the non-nil balances] ...]} over the :ok :read
    ops of numbered processes, node = (nth nodes (mod process (count nodes))).
    Returns None without reads (the plotter then draws nothing). Columns carry
    no :time: their points have None for the seconds."""
    from . import checker as K
    cols, ops, n_acc = _prepare(test, history)
    r = K._ctx().check_bank(cols, n_acc, test["total-amount"], True)
    reads = r["reads"]
    if len(reads) == 0:
        return None
    nodes = list(test["nodes"])
    out = {}
    for row, tot, cls in reads.tolist():
        p = int(cols.process[row])
        if p < 0:
            continue
        if cls & A.BANK_OVERFLOW:
            raise ArithmeticError("integer overflow")
        t = ops[row].get("time") if ops is not None else None
        out.setdefault(nodes[p % len(nodes)], []).append([None if t is None else t / 1e9, tot])
    return out


def plotter():
    """bank.clj:151-177 without the drawing: computes the series and answers
    as the reference's plotter does."""
    from . import checker as K

    def run(test, history, opts):
        return {"valid?": True} if points(test, history) is not None else None
    return K._Fn(run)


def test(opts=None):
    """bank.clj:179-192: the partial test map (the generator stays on the JVM)."""
    from . import checker as K
    opts = {"negative-balances?": False} if opts is None else opts
    return {"max-transfer": 5, "total-amount": 100, "accounts": list(range(8)),
            "checker": K.compose({"SI": checker(opts), "plot": plotter()})}
