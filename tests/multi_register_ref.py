"""A plain reference for linearizability over the multi-register model
(yugabyte/src/yugabyte/multi_key_acid.clj:20-42), from the definitions and
nothing else (not a test module): pure Python over op maps.

  step()      the literal reduce of multi_key_acid.clj:22-34 over a state map
  normal_form() / nf_step()   the five words (never, rmask, rval, wmask, wval)
              the device compiles a txn to, over a bit-packed state
  prepare()   one key's client op maps -> (cause, ops): the pairing of
              knossos.history/complete (an :info row completes nothing; a
              double invocation is cause 3, an orphan completion cause 4, the
              first in history order decides), the value of an :ok op (its
              completion's :value when not nil, else its invocation's), and
              the ops that are searched (not the failed ones, not the crashed
              ones without a write, not the :ok ones that only read nil)
  wgl()       the literal WGL (Lowe 2017 fig. 3, knossos.wgl): a doubly linked
              list of call and return entries, lift / unlift, a cache of
              (linearized set, state); explored = the cache's size; an invalid
              key's fail_entry = the :ok completion row of the deepest return
              the search reached
  brute()     every permitted order, every subset of the crashed ops included
  check()     prepare + the device's stated window rule + wgl

A state is the registers that are not nil: a register written nil is one
never written (the device's packed state says the same).
"""
import itertools

from jepsen_amd import _abi as A

READ, WRITE = ("r", "read", ":r"), ("w", "write", ":w")
MAX_WINDOW = 64


def step(state, txn):
    """The state after txn, or None (inconsistent). state: dict register -> value."""
    for f, k, v in txn:
        if f in READ:
            if not (v is None or v == state.get(k)):
                return None
        elif f in WRITE:
            state = dict(state)
            state[k] = v
        else:
            raise ValueError(f"No matching clause: {f}")
    return state


def skey(state):
    return frozenset((k, v) for k, v in state.items() if v is not None)


def normal_form(txn, bits, reg_id, val_id):
    """(never, rmask, rval, wmask, wval): reg_id / val_id intern registers and
    non-nil values (ids from 1); nil is 0."""
    never, rmask, rval, wmask, wval, written = False, 0, 0, 0, 0, set()
    for f, k, v in txn:
        r = reg_id[k]
        fm = ((1 << bits) - 1) << (r * bits)
        vv = (0 if v is None else val_id[v]) << (r * bits)
        if f in READ:
            if v is None:
                continue
            if r in written:
                never |= (wval & fm) != vv
            elif rmask & fm:
                never |= (rval & fm) != vv
            else:
                rmask |= fm
                rval |= vv
        else:
            written.add(r)
            wmask |= fm
            wval = (wval & ~fm) | vv
    return never, rmask, rval, wmask, wval


def nf_step(nf, s):
    never, rmask, rval, wmask, wval = nf
    return None if never or (s & rmask) != rval else (s & ~wmask) | wval


def prepare(rows):
    """rows: one key's client op maps as (row, op) in history order, values
    unwrapped. -> (cause, ops), ops in call order: {call, ret, txn}."""
    open_inv, pair, cause = {}, {}, 0
    for i, (row, op) in enumerate(rows):
        p, ty = op["process"], op["type"]
        if ty == "info":
            continue
        if ty == "invoke":
            if p in open_inv and not cause:
                cause = 3
            open_inv[p] = i
        elif p in open_inv:
            pair[open_inv.pop(p)] = i
        elif not cause:
            cause = 4
    if cause:
        return cause, None
    ops = []
    for i, (row, op) in enumerate(rows):
        if op["type"] != "invoke":
            continue
        txn, ret = op.get("value"), None
        if i in pair:
            crow, cop = rows[pair[i]]
            if cop["type"] == "fail":
                continue
            ret = crow
            if cop.get("value") is not None:
                txn = cop["value"]
        txn = list(txn or ())
        writes = any(f in WRITE for f, _, _ in txn)
        if ret is None and not writes:
            continue
        if ret is not None and not writes and all(v is None for _, _, v in txn):
            continue
        ops.append({"call": row, "ret": ret, "txn": txn})
    return 0, ops


def widest_window(ops):
    """The most ops open at an :ok return, the returning one not counted."""
    ev = sorted([(o["call"], 1) for o in ops] + [(o["ret"], 0) for o in ops if o["ret"] is not None])
    open_n = widest = 0
    for _, call in ev:
        if call:
            open_n += 1
        else:
            widest = max(widest, open_n - 1)
            open_n -= 1
    return widest


class _Entry:
    __slots__ = ("op", "is_call", "prev", "next", "match")


def wgl(ops, init, budget=None):
    """(valid, cause, fail_entry, explored)."""
    budget = budget if budget and budget > 0 else A.DEFAULT_BUDGET
    rets = sorted(o["ret"] for o in ops if o["ret"] is not None)
    if not rets:
        return A.VALID, 0, -1, 0
    rank = {r: t for t, r in enumerate(rets)}
    ev = sorted([(o["call"], j, True) for j, o in enumerate(ops)] +
                [(o["ret"], j, False) for j, o in enumerate(ops) if o["ret"] is not None])
    head = _Entry()
    head.op, head.is_call, head.prev, head.next, head.match = None, False, None, None, None
    last, calls = head, {}
    for _, j, is_call in ev:
        e = _Entry()
        e.op, e.is_call, e.prev, e.next, e.match = j, is_call, last, None, None
        last.next = e
        last = e
        if is_call:
            calls[j] = e
        else:
            calls[j].match = e

    def lift(e):
        e.prev.next = e.next
        if e.next:
            e.next.prev = e.prev
        m = e.match
        if m:
            m.prev.next = m.next
            if m.next:
                m.next.prev = m.prev

    def unlift(e):
        m = e.match
        if m:
            m.prev.next = m
            if m.next:
                m.next.prev = m
        e.prev.next = e
        if e.next:
            e.next.prev = e

    def first_return():
        e = head.next
        while e and e.is_call:
            e = e.next
        return e

    state, lin, cache, stack, tmax = dict(init), frozenset(), set(), [], 0
    entry = head.next
    while True:
        if entry is not None and entry.is_call:
            s2 = step(state, ops[entry.op]["txn"])
            c = (lin | {entry.op}, skey(s2)) if s2 is not None else None
            if c is not None and c not in cache:
                if len(cache) >= budget:
                    return A.UNKNOWN, 1, -1, len(cache)
                cache.add(c)
                stack.append((entry, state, lin))
                state, lin = s2, c[0]
                lift(entry)
                fr = first_return()
                if fr is None:
                    return A.VALID, 0, -1, len(cache)
                tmax = max(tmax, rank[ops[fr.op]["ret"]])
                entry = head.next
            else:
                entry = entry.next
        else:
            if not stack:
                return A.INVALID, 0, rets[tmax], len(cache)
            entry, state, lin = stack.pop()
            unlift(entry)
            entry = entry.next


def brute(ops, init):
    """Is there a sequential order of every :ok op and any subset of the crashed
    ops that respects real time (a before b when a returned before b was
    called) and steps consistently?"""
    ok = [j for j, o in enumerate(ops) if o["ret"] is not None]
    crashed = [j for j, o in enumerate(ops) if o["ret"] is None]

    def go(state, todo):
        if not any(ops[j]["ret"] is not None for j in todo):
            return True
        for j in todo:
            if any(ops[y]["ret"] is not None and ops[y]["ret"] < ops[j]["call"] for y in todo if y != j):
                continue
            s2 = step(state, ops[j]["txn"])
            if s2 is not None and go(s2, todo - {j}):
                return True
        return False

    for n in range(len(crashed) + 1):
        for sub in itertools.combinations(crashed, n):
            if go(dict(init), frozenset(ok) | frozenset(sub)):
                return True
    return False


def check(rows, init, budget=None):
    """(valid, cause, fail_entry, explored) of one key as the device states it."""
    cause, ops = prepare(rows)
    if cause:
        return A.UNKNOWN, cause, -1, 0
    if any(o["ret"] is not None for o in ops) and widest_window(ops) > MAX_WINDOW:
        return A.UNKNOWN, 2, -1, 0
    return wgl(ops, init, budget)


def check_history(history, init, budget=None, keyed=True):
    """{key: verdict} over op maps, for every key with a client row."""
    per = {}
    for row, op in enumerate(history):
        p = op.get("process")
        if not (isinstance(p, int) and not isinstance(p, bool) and p >= 0):
            continue
        v = op.get("value")
        key = None
        if keyed:
            key, v = v.key, v.val
        per.setdefault(key, []).append((row, dict(op, value=v)))
    return {k: check(rows, init, budget) for k, rows in per.items()}
