"""A plain reference for the cas-register linearizability path of one key,
from the definitions and nothing else (not a test module): pure Python over
one key's rows, no C and no numpy in the algorithm. test_lin_cases.py holds
it against the oracle on every case of lin_cases.py, test_gpu_lin_edges.py
holds the device against both.

Three parts, each stated from its source:

  complete()  knossos.history/complete as jh_oracle.c cites it: an
      invocation's completion is the next entry of the same process that is
      not :info; an :invoke there is a double invocation (cause 3, at that
      row), an :ok / :fail with no open invocation an orphan (cause 4); the
      smallest violating row decides, as the device's atomicMin on viol does.
      Failed ops, crashed reads and :ok reads of nil are dropped; an :ok
      completion supplies a nil invoke value; an :f outside read / write /
      cas on a kept op is cause 5.
  widest_window()  jh_lin.hip's definition: the ops called before the t-th ok
      return and not yet returned there, over kept ops, crashed ops open to
      the end; the widest over t.
  search()  just-in-time linearization: the set of configurations (register
      value, frozenset of linearized open ops), layer by layer over the ok
      returns. An invalid key's fail_entry is the row of the ok completion of
      the first op no configuration gets past (jh_key_verdict). A layer whose
      set passes CONFIG_CAP raises: the cap is a condition on the inputs, never
      a tolerance, so no case is silently skipped.

check() adds the rule outcomes of include/jh.h, stated, not searched: widest
window > 256 -> UNKNOWN / window; more than 65 532 distinct values in the key
(the initial value counts) -> UNKNOWN / states; n_ok >= 2^20 - 1 -> UNKNOWN /
window; under algorithm "linear" the analyzer is LINEAR exactly when the
widest window <= 32, n_states < 4096 and n_ok < 2^20 - 2.

What it does not compute: `explored` (WGL's cache size depends on the order of
its depth-first search), `previous_ok` and `last_op`. Those three come from
the oracle alone.
"""
from jepsen_amd import _abi as A

CONFIG_CAP = 50_000
MAX_VALUES = 65_532
N_OK_LIMIT = (1 << 20) - 1
NIL = A.NIL


class CapExceeded(Exception):
    pass


def key_rows(cols, key=None):
    """One key's rows of Columns as (row, process, type, f, value, value2)
    tuples, in history order: key None takes every row (an unkeyed history),
    else the rows of `key` and the rows in no tuple (independent.clj:234-245)."""
    import numpy as np
    sel = np.arange(int(cols.n)) if key is None else np.nonzero((cols.key == key) | (cols.key < 0))[0]
    return list(zip(sel.tolist(), cols.process[sel].tolist(), cols.type[sel].tolist(), cols.f[sel].tolist(),
                    cols.value[sel].tolist(), cols.value2[sel].tolist()))


def complete(rows):
    """(cause, viol_row, ops): cause 0 and the kept ops in call order, each
    {call, ret (None: crashed), f, v1, v2}, or a cause and no ops (viol_row:
    the smallest violating row for causes 3 and 4, else -1)."""
    open_inv, pair, viol = {}, {}, None
    for i, (row, p, ty, f, v1, v2) in enumerate(rows):
        if p < 0 or ty == A.TYPE_INFO:
            continue
        if ty == A.TYPE_INVOKE:
            if p in open_inv and viol is None:
                viol = (row, 3)
            open_inv[p] = i
        elif p in open_inv:
            pair[open_inv.pop(p)] = i
        elif viol is None:
            viol = (row, 4)
    if viol:
        return viol[1], viol[0], None
    ops = []
    for i, (row, p, ty, f, v1, v2) in enumerate(rows):
        if p < 0 or ty != A.TYPE_INVOKE:
            continue
        ret = None
        if i in pair:
            crow, _, cty, _, c1, c2 = rows[pair[i]]
            if cty == A.TYPE_FAIL:
                continue
            ret = crow
            if f == A.F_CAS:
                if v1 == NIL and v2 == NIL:
                    v1, v2 = c1, c2
            elif v1 == NIL:
                v1 = c1
        if f not in (A.F_READ, A.F_WRITE, A.F_CAS):
            return 5, -1, None
        if f == A.F_READ and (ret is None or v1 == NIL):
            continue
        ops.append({"call": row, "ret": ret, "f": f, "v1": v1, "v2": v2})
    return 0, -1, ops


def widest_window(ops):
    """(widest window, n_ok, sum of the windows): at each ok return, the kept
    ops called before it and not yet returned."""
    ev = []
    for o in ops:
        ev.append((o["call"], 1))
        if o["ret"] is not None:
            ev.append((o["ret"], 0))
    open_n = widest = n_ok = total = 0
    for _, call in sorted(ev):
        if call:
            open_n += 1
        else:
            widest = max(widest, open_n)
            total += open_n
            open_n -= 1
            n_ok += 1
    return widest, n_ok, total


def distinct_values(ops, init=NIL):
    vals = {init} if init != NIL else set()
    for o in ops:
        vals.add(o["v1"])
        if o["f"] == A.F_CAS:
            vals.add(o["v2"])
    vals.discard(NIL)
    return len(vals)


def step(o, s):
    """knossos.model/cas-register: the next value, or None (inconsistent)."""
    if o["f"] == A.F_WRITE:
        return (o["v1"],)
    if o["f"] == A.F_CAS:
        return (o["v2"],) if s == o["v1"] else None
    return (s,) if o["v1"] == NIL or o["v1"] == s else None


def search(ops, init=NIL, cap=CONFIG_CAP):
    """(valid, fail_entry, largest layer) by just-in-time linearization."""
    ev = []
    for j, o in enumerate(ops):
        ev.append((o["call"], 1, j))
        if o["ret"] is not None:
            ev.append((o["ret"], 0, j))
    configs = {(init, frozenset())}
    writes, needs = set(), {}                # the open ops, by the value they need
    largest = 1
    for row, call, j in sorted(ev):
        o = ops[j]
        if call:
            if o["f"] == A.F_WRITE or (o["f"] == A.F_READ and o["v1"] == NIL):
                writes.add(j)
            else:
                needs.setdefault(o["v1"], set()).add(j)
            continue
        # every configuration reachable by linearizing open ops ...
        seen, todo = set(configs), list(configs)
        while todo:
            s, lin = todo.pop()
            for c in (writes | needs.get(s, set())) - lin:
                s2 = step(ops[c], s)
                if s2 is None:
                    continue
                nc = (s2[0], lin | {c})
                if nc not in seen:
                    seen.add(nc)
                    todo.append(nc)
                    if len(seen) > cap:
                        raise CapExceeded(f"{len(seen)} configurations at row {row}")
        largest = max(largest, len(seen))
        # ... of which those that linearized the returning op go on
        configs = {(s, lin - {j}) for s, lin in seen if j in lin}
        if not configs:
            return A.INVALID, row, largest
        writes.discard(j)
        if o["v1"] in needs:
            needs[o["v1"]].discard(j)
    return A.VALID, -1, largest


def replay_sequential(ops, init=NIL):
    """(valid, fail_entry) of a key whose ops never overlap (every window is
    one op): the register replayed in call order. Only for keys too long to
    search in Python; asserts the shape."""
    s, last_ret = init, -1
    for o in ops:
        assert o["ret"] is not None and o["call"] > last_ret
        s2 = step(o, s)
        if s2 is None:
            return A.INVALID, o["ret"]
        s, last_ret = s2[0], o["ret"]
    return A.VALID, -1


def linear_analyzer(width, n_states, n_ok):
    """The analyzer under algorithm "linear" (n_states: the call's interned
    state count, lin_cases.n_states)."""
    return A.ANALYZER_LINEAR if width <= 32 and n_states < 4096 and n_ok < (1 << 20) - 2 else A.ANALYZER_WGL


def check(rows, init=NIL, sequential=False, per_key=False):
    """{valid, cause, fail_entry, width, n_ok, sum_w, n_values, layer} of one key.
    per_key: the call interns values per key (lin_cases.per_key_values), where
    the states rule applies. sequential: replay instead of search."""
    out = {"valid": A.VALID, "cause": 0, "fail_entry": -1, "width": 0, "n_ok": 0, "n_values": 0, "layer": 0, "sum_w": 0}
    if not any(p >= 0 for _, p, *_ in rows):
        return out
    cause, _, ops = complete(rows)
    if cause:
        out.update(valid=A.UNKNOWN, cause=cause)
        return out
    out["n_values"] = distinct_values(ops, init)
    # the device numbers the values of every client read / write / cas row of
    # the key, the rows of dropped ops included (k_ival): count those too
    vals = {init} if init != NIL else set()
    for _, p, _, f, v1, v2 in rows:
        if p >= 0 and f in (A.F_READ, A.F_WRITE, A.F_CAS):
            vals.add(v1)
            if f == A.F_CAS:
                vals.add(v2)
    vals.discard(NIL)
    out["row_values"] = len(vals)
    if per_key and len(vals) > MAX_VALUES:
        out.update(valid=A.UNKNOWN, cause=8)
        return out
    out["width"], out["n_ok"], out["sum_w"] = widest_window(ops)
    if out["n_ok"] == 0:
        return out
    if out["width"] > A.MAX_WINDOW or out["n_ok"] >= N_OK_LIMIT:
        out.update(valid=A.UNKNOWN, cause=2)
        return out
    if sequential:
        out["valid"], out["fail_entry"] = replay_sequential(ops, init)
    else:
        out["valid"], out["fail_entry"], out["layer"] = search(ops, init)
    return out
