"""checker/linearizable over the multi-register model
(yugabyte/src/yugabyte/multi_key_acid.clj:20-42,112-127): the encoder of
jh_check_multi_register's txn layout (include/jh.h), the device call, and a
host path -- a plain Python WGL in the device's order -- for what the device
refuses.

The value of an op (parity unpinned): an :ok op's txn is its
completion's :value when that is not nil, else its invocation's -- the workload
invokes reads as [:r k nil] and fills the values in on the completion
(multi_key_acid.clj:59-69). A crashed op keeps its invocation's txn.

Searched are the client ops that can matter: not the failed ones, not the
crashed ones without a write, not the :ok ones whose txn is the identity
(every micro-op a read of nil). Registers are interned to 0..R-1 (those of the
initial map first), values to dense ids 1..V by Python equality, nil is 0; the
state is R fields of ceil(log2(V + 1)) bits in one 32-bit word.
"""
import types

import numpy as np

from . import _abi as A
from . import history as H
from .model import _MOP_READ, _MOP_WRITE, MultiRegister, is_inconsistent

def _client(p):
    return isinstance(p, (int, np.integer)) and not isinstance(p, bool) and p >= 0


def _txn_of(op, keyed):
    """(key or None, txn or None) of a client op map; TypeError for a :value
    that is no txn."""
    v = op.get("value")
    key = None
    if keyed and H.is_tuple(v):
        key, v = v.key, v.val
    if v is None:
        return key, None
    if not isinstance(v, (list, tuple)):
        raise TypeError(f"the :value of {op!r} is not a txn")
    for mop in v:
        if not isinstance(mop, (list, tuple)) or len(mop) != 3:
            raise TypeError(f"{mop!r} is not a micro-op [f k v]")
    return key, v


def encode(history, model, keyed=False):
    """(Columns, meta) of op maps in the multi-register txn layout: every client
    row carries its txn as [f, reg, val] triples in aux, value = the index of the
    first triple, value2 = their number. meta: n_regs, bits, init (value ids per
    register), regs and values (id -> original). Raises TypeError for a register
    or value that cannot be interned (unhashable) or a :value that is no txn,
    ValueError for a micro-op f without a clause on an op that did not fail (a
    failed op's rows carry a nil txn)."""
    history = list(history)
    n = len(history)
    reg_ids, regs, val_ids, values = {}, [], {}, []

    def reg(k):
        if k not in reg_ids:
            reg_ids[k] = len(regs)
            regs.append(k)
        return reg_ids[k]

    def val(v):
        if v is None:
            return A.NIL
        if v not in val_ids:
            values.append(v)
            val_ids[v] = len(values)
        return val_ids[v]

    init_pairs = [(reg(k), val(v)) for k, v in model.values.items()]
    # the rows of failed ops carry no txn: the op is dropped whatever it says (its micro-ops need no clause)
    open_inv, failed = {}, set()
    for i, op in enumerate(history):
        p, t, v = op.get("process"), op.get("type"), op.get("value")
        if not _client(p) or t == "info":
            continue
        who = (v.key if keyed and H.is_tuple(v) else None, p)
        if t == "invoke":
            open_inv[who] = i
        elif who in open_inv:
            j = open_inv.pop(who)
            if t == "fail":
                failed.update((i, j))
    proc = np.empty(n, np.int64)
    typ = np.empty(n, np.int64)
    fcol = np.empty(n, np.int64)
    key = np.full(n, -1, np.int64)
    value = np.full(n, A.NIL, np.int64)
    value2 = np.zeros(n, np.int64)
    aux = []
    key_ids, keys, f_ids, f_names, others = {}, [], {}, [], {"nemesis": -1}
    for i, op in enumerate(history):
        p = op.get("process")
        if _client(p):
            proc[i] = int(p)
        else:
            proc[i] = others.setdefault(p, -1 - len(others))
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
        v = op.get("value")
        if keyed and H.is_tuple(v):
            if v.key not in key_ids:
                key_ids[v.key] = len(keys)
                keys.append(v.key)
            key[i] = key_ids[v.key]
        if not _client(p) or i in failed:
            continue
        _, txn = _txn_of(op, keyed)
        if txn is None:
            continue
        value[i] = len(aux) // 3
        value2[i] = len(txn)
        for mf, mk, mv in txn:
            if mf in _MOP_READ:
                code = A.F_READ
            elif mf in _MOP_WRITE:
                code = A.F_WRITE
            else:
                raise ValueError(f"No matching clause: {mf}")
            aux.extend((code, reg(mk), val(mv)))
    bits = max(1, len(values).bit_length())
    init = [0] * len(regs)
    for r, v in init_pairs:
        init[r] = 0 if v == A.NIL else v
    cols = H.Columns(n=n, process=proc, type=typ, f=fcol, key=key, value=value, value2=value2, n_keys=len(keys),
                     aux=np.asarray(aux, np.int64) if aux else np.zeros(0, np.int64), keys=keys, f_names=f_names)
    return cols, {"n_regs": len(regs), "bits": bits, "init": init, "regs": regs, "values": values}


# ---------------------------------------------------------------------------
# the host path

def _identity(txn):
    return all(f in _MOP_READ and v is None for f, _, v in (txn or ()))


def key_ops(rows):
    """One key's client rows [(row, process, type name, txn or None)] in history
    order -> (cause, ops): knossos.history/complete's pairing (an :info row
    never completes an invocation) and the ops the search keeps, in call order,
    each {call, ret (None: crashed), txn}. cause 3 / 4: a double invocation / an
    orphan completion, at the smallest such row."""
    open_inv, pair, viol = {}, {}, 0
    for i, (row, p, ty, txn) in enumerate(rows):
        if ty == "info":
            continue
        if ty == "invoke":
            if p in open_inv and not viol:
                viol = 3
            open_inv[p] = i
        elif p in open_inv:
            pair[open_inv.pop(p)] = i
        elif not viol:
            viol = 4
    if viol:
        return viol, None
    ops = []
    for i, (row, p, ty, txn) in enumerate(rows):
        if ty != "invoke":
            continue
        ret = None
        if i in pair:
            crow, _, cty, ctxn = rows[pair[i]]
            if cty == "fail":
                continue
            ret = crow
            if ctxn is not None:
                txn = ctxn
        for f, _, _ in txn or ():
            if f not in _MOP_READ and f not in _MOP_WRITE:
                raise ValueError(f"No matching clause: {f}")
        if ret is None:
            if not any(f in _MOP_WRITE for f, _, _ in txn or ()):
                continue
        elif _identity(txn):
            continue
        ops.append({"call": row, "ret": ret, "txn": list(txn or ())})
    return 0, ops


def _state_key(values):
    """The registers that are not nil, compared as the encoder interns values
    (Python equality); by repr only where a register or a value is unhashable,
    which the encoder refuses."""
    try:
        return frozenset((k, v) for k, v in values.items() if v is not None)
    except TypeError:
        return tuple(sorted((repr(k), repr(v)) for k, v in values.items() if v is not None))


def wgl(ops, model, budget=None):
    """(valid, cause, fail_entry, explored) of one key's kept ops: the WGL
    depth-first search of DESIGN section 3 in the device's order -- candidates
    in call order, restart after a lift, resume after a pop, the child cached
    before descending; explored = the cache's size. A state is the registers
    that are not nil (a register written nil is one never written)."""
    budget = int(budget) if budget and budget > 0 else A.DEFAULT_BUDGET
    rets = sorted((o["ret"], j) for j, o in enumerate(ops) if o["ret"] is not None)
    n_ok = len(rets)
    if n_ok == 0:
        return A.VALID, 0, -1, 0
    ret_op = [j for _, j in rets]
    rr = [None] * len(ops)
    for t, j in enumerate(ret_op):
        rr[j] = t
    windows = [[j for j, o in enumerate(ops) if o["call"] < row and (rr[j] is None or rr[j] >= t)]
               for t, (row, _) in enumerate(rets)]
    t, lin, m, start, tmax = 0, frozenset(), model, 0, 0
    stack, memo = [], set()
    while True:
        w = windows[t]
        took = False
        for i in range(start, len(w)):
            j = w[i]
            if j in lin:
                continue
            m2 = m.step({"value": ops[j]["txn"]})
            if is_inconsistent(m2):
                continue
            t2, lin2 = t, lin | {j}
            if j == ret_op[t]:
                t2 = t + 1
                while t2 < n_ok and ret_op[t2] in lin2:
                    t2 += 1
                lin2 = frozenset(x for x in lin2 if rr[x] is None or rr[x] >= t2) if t2 < n_ok else frozenset()
            c = (t2, lin2, _state_key(m2.values))
            if c in memo:
                continue
            if len(memo) >= budget:
                return A.UNKNOWN, 1, -1, len(memo)
            memo.add(c)
            stack.append((t, i, m, lin))
            t, lin, m, start = t2, lin2, m2, 0
            tmax = max(tmax, t)
            if t == n_ok:
                return A.VALID, 0, -1, len(memo)
            took = True
            break
        if took:
            continue
        if not stack:
            return A.INVALID, 0, ops[ret_op[tmax]]["ret"], len(memo)
        t, i, m, lin = stack.pop()
        start = i + 1


def host_verdicts(history, model, budget=None, keyed=False):
    """{key (None un-keyed): (valid, cause, fail_entry, explored)} by the host
    path, for every key with a client row."""
    per = {}
    for row, op in enumerate(history):
        if not _client(op.get("process")):
            continue
        key, txn = _txn_of(op, keyed)
        per.setdefault(key, []).append((row, op["process"], op.get("type"), txn))
    out = {}
    for key, rows in per.items():
        cause, ops = key_ops(rows)
        out[key] = (A.UNKNOWN, cause, -1, 0) if cause else wgl(ops, model, budget)
    return out


# ---------------------------------------------------------------------------
def verdicts(history, model, budget=None, keyed=False, ctx=None, **hooks):
    """({key: (valid, cause, fail_entry, explored)}, path) of every key with a
    client row (un-keyed: the one key None; no client row at all: {}). path is
    "device", or "host" when the encoder cannot intern a value (TypeError) or
    the library answers JH_EUNSUPPORTED. hooks: waves, flags (jh.h)."""
    from . import _native
    history = list(history)
    try:
        cols, meta = encode(history, model, keyed)
    except TypeError:
        return host_verdicts(history, model, budget, keyed), "host"
    ctx = ctx or _native.default_context()
    try:
        v, _ = ctx.check_multi_register(cols, meta["n_regs"], meta["bits"], meta["init"], budget, **hooks)
    except _native.JhError as e:
        if e.code != A.JH_EUNSUPPORTED:
            raise
        return host_verdicts(history, model, budget, keyed), "host"
    keys = cols.keys if keyed and cols.n_keys else [None]
    out = {}
    for kid, key in enumerate(keys):
        if int(v[kid]["explored"]) == -1:             # in no client row: no :results entry
            continue
        out[key] = (int(v[kid]["valid"]), int(v[kid]["cause"]), int(v[kid]["fail_entry"]), int(v[kid]["explored"]))
    return out, "device"


def result_map(verdict, history):
    """The result map of checker/linearizable for one key's verdict (checker.py
    lin_result). :configs and :final-paths stay empty: jh_lin_configs for this
    model is not built."""
    from .checker import lin_result
    valid, cause, fail_entry, explored = verdict
    return lin_result(valid, cause, fail_entry, explored, types.SimpleNamespace(n=len(history)), ops=history)


def check(history, model, budget=None):
    """(checker/linearizable {:model (multi-register init)}) on one un-keyed
    history of op maps: the result map."""
    assert isinstance(model, MultiRegister)
    history = list(history)
    v, _ = verdicts(history, model, budget, keyed=False)
    return result_map(v.get(None, (A.VALID, 0, -1, 0)), history)
