"""CPU restatements of jepsen.tests.bank/checker, jepsen/src/jepsen/tests/bank.clj:46-121
(with util/min-by and util/max-by, util.clj:71-91, which keep the EARLIER
element on a tie), written from its definition (not a test module):

  ref_ops   over op maps, the reference's own shape: check-op's cond per read,
            group-by :type, first / max-by err-badness / peek, and the float
            badness of a wrong-total emulated (Ratio -> DECIMAL64 -> double ->
            float). Returns the checker's result map.
  ref_cols  over Columns, numpy: segment sums of the CSR pairs. Returns the
            same map with every error replaced by its row (`rows_of` projects a
            result map of op maps onto that), and `triples`, the [row, total,
            class] of jh_check_bank's reads_out. A history on which the
            reference throws gives {"raises": ArithmeticError, "triples": ...}.

The reference tree has no bank test and no recorded bank result: parity is
unpinned against the reference's own tests.
"""
import decimal
import struct

import numpy as np

from jepsen_amd import _abi as A

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TYPES = ("unexpected-key", "nil-balance", "wrong-total", "negative-value")


def checked(x):
    if not I64_MIN <= x <= I64_MAX:
        raise ArithmeticError("integer overflow")
    return x


def reduce_plus(xs):
    acc = 0
    for x in xs:
        acc = checked(acc + x)
    return acc


def int_to_f32(x):
    """(float x) of a long: nearest float, ties to even, from the integer
    itself (through a double it would round twice)."""
    s, m = (-1.0 if x < 0 else 1.0), abs(x)
    if m >> 24:
        sh = m.bit_length() - 24
        q, rem = m >> sh, m & ((1 << sh) - 1)
        half = 1 << (sh - 1)
        if rem > half or (rem == half and q & 1):
            q += 1
        m = q << sh
    return s * float(m)              # at most 25 significant bits: exact in a double


def f32(d):
    """(float d) of a double."""
    return struct.unpack("f", struct.pack("f", d))[0]


def wrong_total_badness(total, total_amount):
    """(Math/abs (float (/ (- total total-amount) total-amount)))."""
    num = checked(total - total_amount)
    if total_amount == 0:
        raise ArithmeticError("Divide by zero")
    if num % total_amount == 0:
        return abs(int_to_f32(num // total_amount))
    ctx = decimal.Context(prec=16, rounding=decimal.ROUND_HALF_EVEN)       # MathContext/DECIMAL64
    return abs(f32(float(ctx.divide(decimal.Decimal(num), decimal.Decimal(total_amount)))))


def check_op(accts, total, negative_balances, op):
    value = op.get("value") or {}
    ks, balances = list(value), list(value.values())
    if not all(k in accts for k in ks):
        return {"type": "unexpected-key", "unexpected": [k for k in ks if k not in accts], "op": op}
    if any(b is None for b in balances):
        return {"type": "nil-balance", "nils": {k: v for k, v in value.items() if v is None}, "op": op}
    if total != reduce_plus(balances):
        return {"type": "wrong-total", "total": reduce_plus(balances), "op": op}
    if not negative_balances and any(b < 0 for b in balances):
        return {"type": "negative-value", "negative": [b for b in balances if b < 0], "op": op}
    return None


def err_badness(test, err):
    t = err["type"]
    if t == "unexpected-key":
        return len(err["unexpected"])
    if t == "nil-balance":
        return len(err["nils"])
    if t == "wrong-total":
        return wrong_total_badness(err["total"], test["total-amount"])
    return checked(-reduce_plus(err["negative"]))


def max_by(f, coll):
    """util/max-by: reduce keeping m unless (f x) is strictly larger; f is not
    called on a single element."""
    coll = list(coll)
    if not coll:
        return None
    m = coll[0]
    if len(coll) == 1:
        return m
    fm = f(m)
    for x in coll[1:]:
        fx = f(x)
        if fx > fm:
            m, fm = x, fx
    return m


def min_by(f, coll):
    coll = list(coll)
    if not coll:
        return None
    m = coll[0]
    if len(coll) == 1:
        return m
    fm = f(m)
    for x in coll[1:]:
        fx = f(x)
        if fx < fm:
            m, fm = x, fx
    return m


def ref_ops(test, ops, negative_balances=False):
    ops = [dict(op, index=op.get("index", i)) for i, op in enumerate(ops)]
    accts, total = set(test["accounts"]), test["total-amount"]
    reads = [op for op in ops if op["type"] == "ok" and op["f"] == "read"]
    errors = {}
    for op in reads:
        e = check_op(accts, total, negative_balances, op)
        if e:
            errors.setdefault(e["type"], []).append(e)
    out = {}
    for t, errs in errors.items():
        m = {"count": len(errs), "first": errs[0], "worst": max_by(lambda e: err_badness(test, e), errs),
             "last": errs[-1]}
        if t == "wrong-total":
            m["lowest"] = min_by(lambda e: e["total"], errs)
            m["highest"] = max_by(lambda e: e["total"], errs)
        out[t] = m
    return {"valid?": all(not v for v in errors.values()),
            "read-count": len(reads),
            "error-count": sum(len(v) for v in errors.values()),
            "first-error": min_by(lambda e: e["op"]["index"], [v[0] for v in errors.values()]),
            "errors": out}


def rows_of(result):
    """A result map of op maps with every error replaced by its row."""
    def row(e):
        return None if e is None else e["op"]["index"]
    return {"valid?": result["valid?"], "read-count": result["read-count"], "error-count": result["error-count"],
            "first-error": row(result["first-error"]),
            "errors": {t: {k: (v if k == "count" else row(v)) for k, v in m.items()} for t, m in result["errors"].items()}}


def points_ref(test, ops):
    """bank/by-node + bank/points over the :ok :reads."""
    nodes = list(test["nodes"])
    out = {}
    for op in ops:
        if op["type"] == "ok" and op["f"] == "read" and isinstance(op["process"], int):
            tot = reduce_plus(b for b in (op.get("value") or {}).values() if b is not None)
            t = op.get("time")
            out.setdefault(nodes[op["process"] % len(nodes)], []).append([None if t is None else t / 1e9, tot])
    return out or None


def _seg(x, off):
    c = np.zeros(len(x) + 1, np.int64)
    np.cumsum(x, out=c[1:])
    return c[off[1:]] - c[off[:-1]]


def ref_cols(cols, n_accounts, total_amount, negative_balances=False, exact=False):
    """exact: the C entry point's own semantics -- :worst of the wrong-totals by
    exact |diff| (no float, so nothing to divide or to overflow)."""
    typ, f = np.asarray(cols.type), np.asarray(cols.f)
    rows = np.nonzero((typ == A.TYPE_OK) & (f == A.F_READ))[0]
    R = len(rows)
    aux = np.asarray(cols.aux, np.int64)
    if len(aux) % 2:
        raise ValueError("odd n_aux")
    half = len(aux) // 2
    v, c = np.asarray(cols.value)[rows], np.asarray(cols.value2)[rows]
    nil = v == A.NIL
    start, cnt = np.where(nil, 0, v), np.where(nil, 0, c)
    if R and ((start < 0) | (cnt < 0) | (start > half) | (cnt > half - start)).any():
        raise ValueError("pair range out of bounds")
    off = np.zeros(R + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    E = int(off[R])
    rid = np.repeat(np.arange(R, dtype=np.int64), cnt)
    pos = start[rid] + (np.arange(E, dtype=np.int64) - off[rid])
    code, bal = aux[2 * pos], aux[2 * pos + 1]
    bnil = bal == A.NIL
    n_un = _seg(((code < 0) | (code >= n_accounts)).astype(np.int64), off)
    n_nil = _seg(bnil.astype(np.int64), off)
    b = np.where(bnil, 0, bal)
    # 32-bit limbs of the positive and the negative part: exact segment sums
    pos, neg = np.where(b > 0, b, 0), np.where(b < 0, b, 0)
    phi, plo, nhi, nlo = _seg(pos >> 32, off), _seg(pos & 0xFFFFFFFF, off), _seg(neg >> 32, off), _seg(neg & 0xFFFFFFFF, off)
    safe = (phi < (1 << 29)) & (plo < (1 << 61)) & (nhi > -(1 << 29)) & (nlo < (1 << 61))    # both sums far inside int64
    psum = np.where(safe, (phi << 32) + plo, 0)
    nsum = np.where(safe, (nhi << 32) + nlo, 0)
    total = psum + nsum                               # every prefix lies in [nsum, psum]
    ovf = np.zeros(R, bool)
    for r in np.nonzero(~safe)[0]:
        acc, nacc = 0, 0
        for x in b[off[r]:off[r + 1]][~bnil[off[r]:off[r + 1]]].tolist():       # pair order decides
            acc += x
            nacc += min(x, 0)
            if not I64_MIN <= acc <= I64_MAX:
                ovf[r] = True
                break
        total[r] = A.NIL if ovf[r] else acc
        nsum[r] = max(nacc, I64_MIN)
    diff = np.abs(total.astype(object) - total_amount) if R else np.zeros(0, object)
    cls = np.where(n_un > 0, 1, np.where(n_nil > 0, 2, np.where(ovf, 0, np.where(
        total != total_amount, 3, np.where((nsum < 0) & (not negative_balances), 4, 0))))).astype(np.int64)
    bad = np.zeros(R, object)
    for t, src in ((1, n_un), (2, n_nil), (3, diff), (4, -nsum.astype(object) if R else nsum)):
        sel = cls == t
        bad[sel] = src[sel]
    triples = np.stack([rows, total, cls + 8 * ovf], axis=1).astype(np.int64) if R else np.zeros((0, 3), np.int64)
    if (ovf & (cls == 0)).any():
        return {"raises": ArithmeticError, "triples": triples}
    errors, firsts = {}, []
    for t, name in enumerate(TYPES, start=1):
        idx = np.nonzero(cls == t)[0]
        if len(idx) == 0:
            continue
        bs = bad[idx].tolist()
        if t == 3 and len(idx) >= 2 and not exact:
            if total_amount == 0 or any(not I64_MIN <= int(total[i]) - total_amount <= I64_MAX for i in idx):
                return {"raises": ArithmeticError, "triples": triples}
            if max(bs) >= (1 << 22):
                bs = [wrong_total_badness(int(total[i]), total_amount) for i in idx]
        m = {"count": len(idx), "first": int(rows[idx[0]]), "worst": int(rows[idx[bs.index(max(bs))]]),
             "last": int(rows[idx[-1]])}
        if t == 3:
            tt = total[idx]
            m["lowest"], m["highest"] = int(rows[idx[np.argmin(tt)]]), int(rows[idx[np.argmax(tt)]])
        errors[name] = m
        firsts.append(m["first"])
    return {"valid?": not errors, "read-count": R, "error-count": int((cls > 0).sum()),
            "first-error": min(firsts) if firsts else None, "errors": errors, "triples": triples}
