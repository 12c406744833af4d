"""Seeded builders of cas-register histories that sit on the boundaries where
jh_lin.hip switches paths (not a test module). test_lin_cases.py (CPU) and
test_gpu_lin_edges.py (GPU) build the same cases from here; lin_ref.py is the
reference that says what each must give.

What synth.cas_register never produces, and these do:

  A  a widest window of exactly W members, W on both sides of 32 (the
     reachable-set engine), 40 (LEAN / WIDE), 64 (WIDE / k_lin_xw), 128
     (JH_XW_SL2) and 256 (JH_MAX_WINDOW), reached two ways -- crashed ops held
     open, and W genuinely concurrent :ok ops -- valid and invalid, the widest
     layer before or after the failing read or at the key's last ok return;
     and 40 / 64 / 256 kept members with dropped ops open beside them.
  B  one far-off value in one key (or the initial value) that sets vmax - vmin
     for the whole call, on both sides of states8 (n_states <= 256), states_ok
     (n_states < 4096) and the per-key interning switch (span 65 531).
  C  255 / 256 / 257 and 65 531 / 65 532 / 65 533 distinct values in one key.
  D  n_ok = 15 999 / 16 000 (the compact tables' limit) and 2^20 - 2 / 2^20 - 1
     (the t field's). The other arm of long_key, n_ops > 65535, cannot be
     reached below n_ok = 16 000: ops that are not ok are crashed, crashed ops
     stay in the window, and the window holds 256. No case fakes it.
  E  controlled sorted layouts for k_pair / k_orphan / key_pass1: segment
     sizes around 64 and 128, invocations on lane 63, completions 64, 65 and
     200 positions on, the same process in adjacent segments, violations.
  F  calls whose engine lists have 0, 1 and many members.

The search cost stays tiny by construction. Crashed width comes from crashed
:cas ops whose `cur` value the register never holds (they can never be
linearized, so they widen every window and add no configuration) next to at
most four crashed writes that can. Concurrent width comes from a chain of W
:ok :cas ops c -> c+1 -> ... all open at once: only one order is legal, so a
layer holds at most W + 1 configurations. Valid keys come from a simulated
register (class Key): every op takes effect at a point inside its interval.

A case is a Case: the Columns, the initial value, and one label per key saying
what it sits on (width, verdict, failing row, engine).
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from jepsen_amd import _abi as A
from jepsen_amd.history import Columns

INV, OK, FAIL, INFO = A.TYPE_INVOKE, A.TYPE_OK, A.TYPE_FAIL, A.TYPE_INFO
RD, WR, CAS = A.F_READ, A.F_WRITE, A.F_CAS
NEMESIS = -1

WIDTHS = (1, 2, 31, 32, 33, 39, 40, 41, 42, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257)
DROPPED_WIDTHS = (40, 64, 256)
SPANS = (253, 254, 255, 4092, 4093, 4094, 65_529, 65_530, 65_531, 65_532)
VALUE_COUNTS = (255, 256, 257)
STATES_COUNTS = (65_531, 65_532, 65_533)
LONG_N_OK = (15_999, 16_000)
T_N_OK = ((1 << 20) - 2, (1 << 20) - 1)
SEGMENTS = (1, 63, 64, 65, 127, 128, 129)
GAPS = (64, 65, 200)
BAD = 6                 # the value no op of families A, E, F ever writes
NEVER = (7, 8, 9)       # `cur` of the crashed :cas ops: never in the register


class Key:
    """One key's rows (process, type, f, value, value2) and the register they
    are simulated on: inv() opens an op, lin() is its linearization point,
    ok() / fail() / info() complete it with what the register gave it."""

    def __init__(self, init=None):
        self.rows, self.reg, self.pend = [], init, {}
        self.label = {}

    def raw(self, p, ty, f, a=None, b=None):
        self.rows.append((p, ty, f, a, b))
        return len(self.rows) - 1

    def inv(self, p, f, a=None, b=None):
        assert p not in self.pend
        self.pend[p] = [f, a, b, None]
        return self.raw(p, INV, f, a, b)

    def lin(self, p):
        o = self.pend[p]
        assert o[3] is None
        if o[0] == WR:
            self.reg, o[3] = o[1], "done"
        elif o[0] == CAS:
            o[3] = "done" if self.reg == o[1] else "failed"
            if o[3] == "done":
                self.reg = o[2]
        else:
            o[3] = ("read", self.reg)

    def ok(self, p):
        f, a, b, res = self.pend.pop(p)
        assert res is not None and res != "failed", (p, f, a, b, res)
        return self.raw(p, OK, f, res[1] if f == RD else a, b)

    def fail(self, p):
        f, a, b, res = self.pend.pop(p)
        assert res is None or res == "failed"
        return self.raw(p, FAIL, f, a, b)

    def info(self, p):
        f, a, b, _ = self.pend[p]         # stays open: the process is never used again
        return self.raw(p, INFO, f, a, b)

    def seq(self, p, f, a=None, b=None):
        self.inv(p, f, a, b)
        self.lin(p)
        return self.ok(p)

    def bad_read(self, p, v=BAD):
        """A read of a value the register never held: the key is invalid at
        the returned row unless it is already."""
        self.raw(p, INV, RD)
        return self.raw(p, OK, RD, v)


def _engine(width, states8=True):
    if width > 256:
        return "window"
    if width > 128:
        return "xw4"
    if width > 64:
        return "xw2"
    return "lean" if (width <= 40 and states8) else "wide"


def crashed_key(W, valid=True, place="last", seed=0, init=None, infos=True):
    """Widest window W from W - 1 crashed ops held open beside sequential ops
    of process 0 / 1. place: "last" (valid: the last ok return is W wide),
    "before" (the window is W wide before the failing read, and at it),
    "after" (the failing read sits in a window of 1; the crashed ops come
    after it)."""
    rng = np.random.default_rng(seed)
    k = Key(init)
    P = W - 1
    k.seq(0, WR, 1)
    k.seq(1, RD)
    fail_at = None
    if not valid and place == "after":
        fail_at = k.bad_read(1)
    procs = [100 + i for i in range(P)]
    for i, p in enumerate(procs):
        if i < 4:
            k.inv(p, WR, 2 + i % 2)
        else:
            k.inv(p, CAS, NEVER[i % 3], 5)
        if i % 5 == 0:
            k.seq(i % 2, RD)                  # sequential ops while the window grows
    for i, p in enumerate(procs[:4]):
        if i % 2 == 0:
            k.lin(p)                          # two of the crashed writes took effect
    k.seq(0, RD)
    k.seq(1, CAS, k.reg, 4)
    k.seq(0, WR, 1)
    if not valid and place == "before":
        fail_at = k.bad_read(1)
        k.seq(0, RD)
    if infos:
        for p in procs:
            if rng.random() < 0.5:
                k.info(p)
    if valid:
        k.seq(1, RD)                          # the last ok return: W - 1 crashed ops and itself
    k.label = dict(width=max(W, 1), valid=A.VALID if valid else A.INVALID, fail_at=fail_at, how="crashed",
                   place=place)
    return k


def concurrent_key(W, valid=True, place="before", seed=0, init=None, base=10):
    """Widest window W from W :ok :cas ops base -> base+1 -> ... -> base+W, all
    invoked (in shuffled order) before the first returns (in shuffled order).
    place (invalid): the burst "before" the failing read, or "after" it."""
    rng = np.random.default_rng(seed)
    k = Key(init)
    k.seq(0, WR, base)
    k.seq(1, RD)
    fail_at = None
    if not valid and place == "after":
        fail_at = k.bad_read(1)
    procs = [10 + i for i in range(W)]
    for i in rng.permutation(W).tolist():
        k.inv(procs[i], CAS, base + i, base + i + 1)
    for p in procs:
        k.lin(p)
    for i in rng.permutation(W).tolist():
        k.ok(procs[i])
    k.seq(0, RD)
    if not valid and place == "before":
        fail_at = k.bad_read(1)
    k.seq(1, WR, 1)
    k.seq(0, RD)
    k.label = dict(width=W, valid=A.VALID if valid else A.INVALID, fail_at=fail_at, how="concurrent", place=place)
    return k


def dropped_key(W, n_drop, valid=True):
    """W kept members (W - 1 crashed ops and one sequential op) with n_drop
    dropped ops open at the same return: a failed write, a crashed read, an
    :ok read of nil. The width stays W."""
    k = Key()
    k.seq(0, WR, 1)
    procs = [100 + i for i in range(W - 1)]
    for i, p in enumerate(procs):
        k.inv(p, CAS, NEVER[i % 3], 5) if i >= 2 else k.inv(p, WR, 2 + i)
    k.raw(50, INV, WR, 3)                     # fails
    if n_drop >= 2:
        k.raw(51, INV, RD)                    # crashes
    if n_drop >= 3:
        k.raw(52, INV, RD)                    # reads nil
    k.seq(0, RD)                              # W kept ops open here, and n_drop dropped ones
    fail_at = None if valid else k.bad_read(1)
    k.raw(50, FAIL, WR, 3)
    if n_drop >= 2:
        k.raw(51, INFO, RD)
    if n_drop >= 3:
        k.raw(52, OK, RD, None)
    k.seq(0, RD)
    k.label = dict(width=W, valid=A.VALID if valid else A.INVALID, fail_at=fail_at, how="dropped", n_drop=n_drop)
    return k


def pass1_window_key(P=300):
    """P crashed ops invoked before the first ok return, then six sequential
    ops: every window has P + 1 members, so even the average window passes
    JH_MAX_WINDOW and key_pass1 settles the key (UNKNOWN / window) without
    building a table. (A key whose widest window alone passes 256, like
    crashed_key(257), goes to k_lin_xw's list and is found there.)"""
    k = Key()
    for i in range(P):
        k.inv(100 + i, CAS, NEVER[i % 3], 5)
    for i in range(6):
        k.seq(i % 2, WR, 1 + i % 4)
    k.label = dict(width=P + 1, valid=A.UNKNOWN, cause=2, fail_at=None, how="pass1-window")
    return k


def small_key(seed, valid=True, init=None):
    """A neighbour: three processes, a dozen overlapping ops."""
    rng = np.random.default_rng(seed)
    k = Key(init)
    k.seq(0, WR, 1 + int(rng.integers(5)))
    for _ in range(12):
        p = int(rng.integers(3))
        if p in k.pend:
            k.lin(p) if k.pend[p][3] is None else None
            k.fail(p) if k.pend[p][3] == "failed" else k.ok(p)
            continue
        u = rng.random()
        if u < 0.4:
            k.inv(p, RD)
        elif u < 0.8:
            k.inv(p, WR, 1 + int(rng.integers(5)))
        else:
            k.inv(p, CAS, 1 + int(rng.integers(5)), 1 + int(rng.integers(5)))
    for p in list(k.pend):
        if k.pend[p][3] is None:
            k.lin(p)
        k.fail(p) if k.pend[p][3] == "failed" else k.ok(p)
    fail_at = None if valid else k.bad_read(4)
    k.label = dict(valid=A.VALID if valid else A.INVALID, fail_at=fail_at, how="small")
    return k


# -- packing -------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    cols: Columns
    init: object                       # None = nil
    keys: list                         # one label dict per key id
    keyed: bool = True
    budget: int = A.DEFAULT_BUDGET
    notes: dict = field(default_factory=dict)

    @property
    def init64(self):
        return A.NIL if self.init is None else int(self.init)


def columns(rows, n_keys):
    """Columns of (key, process, type, f, value, value2) rows, straight into
    the arrays (key ids as given: H.encode would renumber them by first
    appearance)."""
    n = len(rows)
    a = np.full((6, max(n, 1)), A.NIL, np.int64)
    for i, (key, p, ty, f, v1, v2) in enumerate(rows):
        a[0, i], a[1, i], a[2, i], a[3, i] = key, p, ty, f
        if v1 is not None:
            a[4, i] = v1
        if v2 is not None:
            a[5, i] = v2
    a = a[:, :n]
    return Columns(n=n, process=a[1].copy(), type=a[2].copy(), f=a[3].copy(), key=a[0].copy(), value=a[4].copy(),
                   value2=a[5].copy(), n_keys=n_keys, aux=np.zeros(1, np.int64))


def pack(name, keys, init=None, seed=0, mix=True, nemesis=True, keyed=True, absent=(), **kw):
    """The keys' rows merged into one history. Key i of `keys` gets the i-th
    key id that is not in `absent`; mix: the keys' rows interleave at random
    (each key's own order kept), else key after key. Un-keyed nemesis rows go
    in between. Each label gains fail_entry (the history row) and rows."""
    rng = np.random.default_rng(seed + 17)
    ids = [i for i in range(len(keys) + len(absent)) if i not in absent]
    order = np.repeat(np.arange(len(keys)), [len(k.rows) for k in keys])
    if mix:
        order = order[rng.permutation(len(order))]
    nxt = [0] * len(keys)
    rows, where = [], [[] for _ in keys]
    for j, i in enumerate(order.tolist()):
        if nemesis and keyed and j % 97 == 50:
            rows.append((-1, NEMESIS, INFO, 16, None, None))
        where[i].append(len(rows))
        rows.append((ids[i] if keyed else -1,) + keys[i].rows[nxt[i]])
        nxt[i] += 1
    n_keys = len(keys) + len(absent) if keyed else 0
    labels = [dict(absent=True, valid=A.VALID, fail_entry=-1) for _ in range(max(n_keys, 1))]
    for i, k in enumerate(keys):
        lab = dict(k.label, rows=len(k.rows), absent=False)
        if lab.get("width", 0) > A.MAX_WINDOW:             # past JH_MAX_WINDOW: no search
            lab.update(valid=A.UNKNOWN, cause=2, fail_at=None)
        fa = lab.get("fail_at")
        lab["fail_entry"] = where[i][fa] if fa is not None else -1
        labels[ids[i] if keyed else 0] = lab
    return Case(name, columns(rows, n_keys), init, labels, keyed=keyed, **kw)


def single(name, key, init=None, **kw):
    """One key as an un-keyed history (jh_check_cas)."""
    return pack(name, [key], init=init, mix=False, nemesis=False, keyed=False, **kw)


# -- what the call does with the values (jh_lin.hip, lin_check_independent) --------------
def value_range(cols, init=None):
    cl = (cols.process >= 0) & (cols.f <= CAS)
    v = cols.value[cl]
    v2 = cols.value2[cl & (cols.f == CAS)]
    vals = [int(x) for x in np.concatenate([v[v != A.NIL], v2[v2 != A.NIL]]).tolist()]
    if init is not None:
        vals.append(int(init))
    return (min(vals), max(vals)) if vals else (0, 0)


def span(cols, init=None):
    lo, hi = value_range(cols, init)
    return hi - lo


def per_key_values(cols, init=None):
    """Interning turns per-key at a span of RQ_EMPTY - 3 = 65 531; a span that
    wraps int64 counts as huge."""
    return span(cols, init) >= 65_531


def n_states(case):
    """The call's n_states: vmax - vmin + 2 over the whole history (and the
    initial value), or under per-key interning the largest key's distinct
    values (the initial value among them) + 1."""
    if not per_key_values(case.cols, case.init):
        return span(case.cols, case.init) + 2
    c = case.cols
    worst = 1 if case.init is not None else 0
    cl = (c.process >= 0) & (c.f <= CAS)
    for k in (range(c.n_keys) if case.keyed else [None]):
        sel = cl & (c.key == k) if k is not None else cl
        a, b = c.value[sel], c.value2[sel & (c.f == CAS)]
        vals = set(a[a != A.NIL].tolist()) | set(b[b != A.NIL].tolist())
        if case.init is not None:
            vals.add(int(case.init))
        worst = max(worst, len(vals))
    return worst + 1


def engine(case, label):
    """Where k_key_tables sends the key: "lean", "wide", "xw2", "xw4",
    "window" (over 256: no search), or None when the label has no width."""
    if "width" not in label:
        return None
    return _engine(label["width"], n_states(case) <= 256)


# -- family A ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def width_case(W):
    """One call per width: the width reached from crashed ops (valid with the
    last return widest; invalid with the widest layer before and after the
    failing read) and from concurrent :ok ops (valid; invalid before / after),
    and a small neighbour. Values stay within [1, W + 11]."""
    keys = [crashed_key(W, True, "last", seed=W),
            crashed_key(W, False, "before", seed=W + 1),
            crashed_key(W, False, "after", seed=W + 2, infos=False),
            concurrent_key(W, True, seed=W + 3),
            concurrent_key(W, False, "before", seed=W + 4),
            concurrent_key(W, False, "after", seed=W + 5),
            small_key(W)]
    return pack(f"width{W}", keys, seed=W)


@functools.lru_cache(maxsize=None)
def width_single(W, how, valid):
    """One key of width_case(W) as an un-keyed history."""
    k = crashed_key(W, valid, "last" if valid else "before", seed=W) if how == "crashed" else \
        concurrent_key(W, valid, "before", seed=W + 3)
    return single(f"width{W}-{how}-{'valid' if valid else 'invalid'}", k)


@functools.lru_cache(maxsize=None)
def dropped_case(W):
    keys = [dropped_key(W, n, valid=n != 2) for n in (1, 2, 3)]
    return pack(f"dropped{W}", keys, seed=W)


# -- family B ------------------------------------------------------------------------
def _span_base():
    """Keys with values in [1, 50]: widths 40 (LEAN while states8), 41, 33, 32,
    a concurrent invalid one and two neighbours."""
    return [crashed_key(40, True, "last", seed=1), crashed_key(41, False, "before", seed=2),
            crashed_key(32, True, "last", seed=3), crashed_key(33, False, "after", seed=4),
            concurrent_key(40, False, "before", seed=5), small_key(6), small_key(7, valid=False)]


N_SPAN_BASE = 7


def _outlier(v):
    k = Key()
    k.seq(0, WR, v)
    k.seq(1, RD)
    k.label = dict(width=1, valid=A.VALID, fail_at=None, how="outlier")
    return k


@functools.lru_cache(maxsize=None)
def span_case(s, how="high"):
    """The base keys (ids 0..6, the same rows in every span case) and a span of
    exactly s set by: "high" one far-off value above in key 7; "low" one
    below (negative); "init_high" / "init_low" the initial value alone."""
    base = _span_base()
    lo, hi = 1, 50
    if how == "high":
        c = pack(f"span{s}-{how}", base + [_outlier(lo + s)], seed=5)
    elif how == "low":
        c = pack(f"span{s}-{how}", base + [_outlier(hi - s)], seed=5)
    elif how == "init_high":
        c = pack(f"span{s}-{how}", base, init=lo + s, seed=5)
    else:
        c = pack(f"span{s}-{how}", base, init=hi - s, seed=5)
    lo2, hi2 = value_range(c.cols, c.init)
    assert (lo2, hi2) == ((lo, lo + s) if how.endswith("high") else (hi - s, hi)), (lo2, hi2)
    c.notes["span"] = s
    return c


@functools.lru_cache(maxsize=None)
def wrap_case():
    """Values near -2^62 and +2^62 in keys 7 and 8: vmax - vmin wraps int64 (to
    a negative number), and per-key interning must still order them."""
    far = 1 << 62
    k = Key()
    k.seq(0, WR, far + 3)
    k.seq(1, CAS, far + 3, -far - 3)
    k.seq(0, RD)
    k.seq(1, WR, far - 1)
    k.bad_read(0, far)
    k.label = dict(width=1, valid=A.INVALID, fail_at=len(k.rows) - 1, how="wrap")
    k2 = Key()
    k2.seq(0, WR, -far)
    k2.seq(1, CAS, -far, far)
    k2.seq(0, RD)
    k2.label = dict(width=1, valid=A.VALID, fail_at=None, how="wrap")
    c = pack("span-wrap", _span_base() + [k, k2], seed=5)
    c.notes["span"] = 2 * far + 6
    return c


# -- family C ------------------------------------------------------------------------
def _values_key(n, step, init=None, bad=False):
    """n distinct values step, 2 step, ... written in turn by process 0 and
    read back by process 1 now and then."""
    k = Key(init)
    for i in range(1, n + 1):
        k.seq(0, WR, i * step)
        if i % 50 == 0:
            k.seq(1, RD)
    fail_at = k.bad_read(1, 2 * step) if bad else None
    k.label = dict(width=1, valid=A.INVALID if bad else A.VALID, fail_at=fail_at, how="values", n_values=n)
    return k


@functools.lru_cache(maxsize=None)
def values_case(n, with_init):
    """A key of n distinct values 300 apart (a span past 65 531: per-key
    interning) and neighbours. with_init: the initial value is one of the n;
    else it is nil."""
    init = 300 * 7 if with_init else None
    keys = [small_key(1, init=init), _values_key(n, 300, init, bad=n % 2 == 1), crashed_key(40, True, "last", seed=2, init=init),
            small_key(3, valid=False, init=init)]
    c = pack(f"values{n}-{'init' if with_init else 'nil'}", keys, init=init, seed=n)
    c.notes["n_values"] = n
    return c


@functools.lru_cache(maxsize=None)
def states_case(n):
    """Key 1: n distinct values 3, 6, ... written in turn by one process (about
    2 n rows, straight into the arrays) and a last read; keys 0 and 2: small
    neighbours. n = 65 533 is one past what a key may hold."""
    a, b = small_key(11), small_key(12, valid=False)
    rows = [(0,) + r for r in a.rows]
    vals = np.arange(1, n + 1, dtype=np.int64) * 3
    m = 2 * n + 2
    big = np.full((6, m), A.NIL, np.int64)
    big[0], big[1], big[3] = 1, 0, WR
    big[2, 0::2], big[2, 1::2] = INV, OK
    big[4, 0:2 * n:2], big[4, 1:2 * n:2] = vals, vals
    big[3, 2 * n:], big[4, 2 * n + 1] = RD, vals[-1]
    rows_b = [(2,) + r for r in b.rows]
    head, tail = columns(rows, 3), columns(rows_b, 3)
    cat = lambda f: np.concatenate([getattr(head, f), big[{"key": 0, "process": 1, "type": 2, "f": 3, "value": 4, "value2": 5}[f]],
                                    getattr(tail, f)])       # noqa: E731
    cols = Columns(n=head.n + m + tail.n, process=cat("process"), type=cat("type"), f=cat("f"), key=cat("key"),
                   value=cat("value"), value2=cat("value2"), n_keys=3, aux=np.zeros(1, np.int64))
    labels = [dict(a.label, fail_entry=-1, absent=False, rows=len(a.rows)),
              dict(width=1, valid=A.VALID if n <= 65_532 else A.UNKNOWN, cause=8 if n > 65_532 else 0, fail_entry=-1,
                   absent=False, how="states", n_values=n, rows=m),
              dict(b.label, fail_entry=head.n + m + b.label["fail_at"], absent=False, rows=len(b.rows))]
    return Case(f"states{n}", cols, None, labels, notes={"n_values": n})


# -- family D ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_case(n_ok, valid):
    """One sequential key of exactly n_ok ok ops (writes of i mod 5 and reads,
    two processes in turn); invalid: the bad read is the last op but two."""
    k = Key()
    fail_at = None
    for i in range(n_ok):
        if not valid and i == n_ok - 3:
            fail_at = k.bad_read(i % 2)
        elif i % 3 == 2:
            k.seq(i % 2, RD)
        else:
            k.seq(i % 2, WR, i % 5)
    k.label = dict(width=1, valid=A.VALID if valid else A.INVALID, fail_at=fail_at, how="long", n_ok=n_ok)
    assert fail_at is None or len(k.rows) - fail_at <= 10
    return single(f"long{n_ok}-{'valid' if valid else 'invalid'}", k)


@functools.lru_cache(maxsize=2)
def t_limit_case(n_ok):
    """One process, n_ok writes of i mod 5 and nothing else, straight into the
    arrays (keyed, key 0; key 1 a small neighbour at the end). At n_ok = 2^20
    - 1 the key is past every table's t field: UNKNOWN / window."""
    b = small_key(21)
    m = 2 * n_ok
    proc = np.zeros(m, np.int64)
    ty = np.tile(np.array([INV, OK], np.int64), n_ok)
    val = np.repeat(np.arange(n_ok, dtype=np.int64) % 5, 2)
    tail = columns([(1,) + r for r in b.rows], 2)
    cols = Columns(n=m + tail.n, process=np.concatenate([proc, tail.process]), type=np.concatenate([ty, tail.type]),
                   f=np.concatenate([np.full(m, WR, np.int64), tail.f]), key=np.concatenate([np.zeros(m, np.int64), tail.key]),
                   value=np.concatenate([val, tail.value]), value2=np.concatenate([np.full(m, A.NIL, np.int64), tail.value2]),
                   n_keys=2, aux=np.zeros(1, np.int64))
    over = n_ok >= (1 << 20) - 1
    labels = [dict(width=1, valid=A.UNKNOWN if over else A.VALID, cause=2 if over else 0, fail_entry=-1, absent=False,
                   how="t-limit", n_ok=n_ok, rows=m),
              dict(b.label, fail_entry=-1, absent=False, rows=len(b.rows))]
    return Case(f"tlimit{n_ok}", cols, None, labels, budget=1 << 21)


# -- family E ------------------------------------------------------------------------
def segment_key(n, first="invoke", seed=0):
    """A key of exactly n rows by processes 0 and 1 (the same two in every
    segment). first: "invoke" (a sequential op of process 0 first) or "ok" (an
    :ok of process 0 with no invocation first: an orphan at the segment's first
    row). An odd remainder ends the segment with a lone invocation of process 0
    (a crashed write: the last row of the segment has no completion)."""
    k = Key()
    orphan = first == "ok"
    if orphan:
        k.raw(0, OK, WR, 1)
    i = 0
    while len(k.rows) + 2 <= n:
        if i % 3 == 2:
            k.seq(i % 2, RD)
        else:
            k.seq(i % 2, WR, 1 + i % 4)
        i += 1
    if len(k.rows) < n:
        k.raw(0, INV, WR, 2)
    assert len(k.rows) == n
    k.label = dict(valid=A.UNKNOWN if orphan else A.VALID, cause=4 if orphan else 0, fail_at=None, how="segment")
    if not orphan and n > 1:
        k.label["width"] = 1
    return k


@functools.lru_cache(maxsize=None)
def segments_case(mix=False):
    """Segments of 1, 63, 64, 65, 127, 128, 129 rows, then 65 rows starting
    with an orphan, then 2: K = 9 keys, every one on processes 0 and 1. The odd
    segments end with a lone invocation of process 0 and the next segment
    starts with process 0: an :invoke (no double invocation across the edge)
    or, after the 129, an :ok (an orphan of its own key, no completion of the
    key before). Sorted, the 63-row segment puts its last invocation on
    position 63 of the first group."""
    keys = [segment_key(n, seed=n) for n in SEGMENTS] + [segment_key(65, first="ok"), segment_key(2)]
    return pack("segments-mixed" if mix else "segments", keys, seed=3, mix=mix, nemesis=mix)


def gap_key(gaps=GAPS, lead=1):
    """After `lead` :info rows of process 9 (they move every later position),
    for each gap g: process 7 invokes a write, g - 1 rows follow (sequential
    ops of process 1 and, for an even g, one :info of process 7; two more
    :info rows of process 7 replace a pair for g >= 65), then its :ok exactly g
    positions after the invocation."""
    k = Key()
    for _ in range(lead):
        k.raw(9, INFO, WR, 1)
    at = []
    for n, g in enumerate(gaps):
        i0 = k.inv(7, WR, 1 + n)
        k.lin(7)
        fill = g - 1
        infos = fill % 2 + (2 if g >= 65 else 0)
        for j in range((fill - infos) // 2):
            k.seq(1, RD) if j % 2 else k.seq(1, CAS, k.reg, 1 + (k.reg + 1) % 4)
            if infos and j % 9 == 4:
                k.info(7)
                infos -= 1
        for _ in range(infos):
            k.info(7)
        i1 = k.ok(7)
        assert i1 - i0 == g, (g, i1 - i0)
        at.append(i0)
    k.label = dict(width=2, valid=A.VALID, fail_at=None, how="gaps", inv_at=at)
    return k


@functools.lru_cache(maxsize=None)
def gaps_case():
    """Key 0: 62 rows, so key 1 starts at sorted position 62 and, after its one
    leading :info, invokes on position 63 with the completion on the next row
    (gap 1), then completions 64, 65 and 200 positions after their
    invocations; key 2 the same gaps from another offset, invalid at the end."""
    k0 = segment_key(62)
    k1 = gap_key((1,) + GAPS, lead=1)
    k2 = gap_key(GAPS[::-1], lead=30)
    k2.label.update(valid=A.INVALID, fail_at=k2.bad_read(3))
    c = pack("gaps", [k0, k1, k2], mix=False, nemesis=False)
    assert (62 + k1.label["inv_at"][0]) % 64 == 63
    return c


def violation_key(which):
    k = Key()
    k.seq(0, WR, 1)
    if which == "double-first":                # rows 2, 3: double invocation at 3; orphan at 5
        k.raw(2, INV, WR, 2), k.raw(2, INV, WR, 3), k.raw(2, OK, WR, 3), k.raw(3, OK, RD, 1)
        cause = 3
    elif which == "orphan-first":              # orphan at 2; double invocation at 4
        k.raw(3, FAIL, RD), k.raw(2, INV, WR, 2), k.raw(2, INV, WR, 3), k.raw(2, OK, WR, 3)
        cause = 4
    elif which == "info-double":               # :info does not close the process
        k.raw(2, INV, WR, 2), k.raw(2, INFO, WR, 2), k.raw(2, INFO, WR, 2), k.raw(2, INV, WR, 3)
        cause = 3
    elif which == "bad-f":
        k.raw(2, INV, 16, 2), k.raw(2, OK, 16, 2)
        cause = 5
    elif which == "bad-f-failed":              # a failed op's :f is never looked at
        k.raw(2, INV, 16, 2), k.raw(2, FAIL, 16, 2)
        cause = 0
    k.seq(1, RD)
    k.label = dict(valid=A.UNKNOWN if cause else A.VALID, cause=cause, fail_at=None, how=which)
    if not cause:
        k.label["width"] = 1
    return k


def empty_key(which):
    """No ok return of a kept op (n_ok == 0): valid, nothing explored."""
    k = Key()
    if which == "nemesis":                     # keyed rows of no client process
        k.raw(NEMESIS, INFO, 16), k.raw(-2, INFO, 17), k.raw(NEMESIS, INFO, 16)
    elif which == "dropped":                   # a failed write, a crashed read, a read of nil
        k.raw(0, INV, WR, 3), k.raw(1, INV, RD), k.raw(2, INV, RD)
        k.raw(0, FAIL, WR, 3), k.raw(1, INFO, RD), k.raw(2, OK, RD, None)
    else:                                      # crashed writes only
        k.raw(0, INV, WR, 3), k.raw(1, INV, WR, 4), k.raw(0, INFO, WR, 3)
    k.label = dict(valid=A.VALID, fail_at=None, how="empty-" + which, n_ok=0)
    return k


@functools.lru_cache(maxsize=None)
def violations_case():
    """K = 11 keys with ids 3 and 8 absent: violations (the smaller row wins),
    keys without a kept ok op, neighbours."""
    keys = [violation_key("double-first"), small_key(1), violation_key("orphan-first"), empty_key("nemesis"),
            violation_key("info-double"), empty_key("dropped"), violation_key("bad-f"), empty_key("crashed"),
            violation_key("bad-f-failed")]
    return pack("violations", keys, seed=9, absent=(3, 8))


@functools.lru_cache(maxsize=None)
def one_key_case():
    """K = 1, keyed."""
    return pack("one-key", [gap_key((65,), lead=2)], nemesis=False)


# -- family F ------------------------------------------------------------------------
ENGINE_LISTS = ("lean", "wide", "xw2", "xw4", "each", "none")


@functools.lru_cache(maxsize=None)
def engines_case(which):
    """Calls whose keys all go to one engine, to one engine each, or to none
    (every key settled in key_pass1)."""
    mk = lambda ws: [f(w, v, "before" if not v else ("last" if f is crashed_key else "before"), seed=w + i)      # noqa: E731
                     for i, (w, f, v) in enumerate(ws)]
    c, o = crashed_key, concurrent_key
    if which == "lean":
        keys = mk([(40, c, True), (7, o, False), (39, o, True), (3, c, False), (40, o, False)])
    elif which == "wide":
        keys = mk([(41, c, False), (64, o, True), (50, c, True), (41, o, False), (64, c, False)])
    elif which == "xw2":
        keys = mk([(65, c, False), (128, o, True), (100, c, True), (128, c, False), (65, o, False)])
    elif which == "xw4":
        keys = mk([(129, c, False), (256, o, True), (200, c, True), (256, c, False), (129, o, False)])
    elif which == "each":
        keys = mk([(40, c, False), (64, c, False), (128, c, False), (256, c, False), (257, c, False)])
    else:
        keys = [violation_key("double-first"), empty_key("dropped"), pass1_window_key(),
                empty_key("nemesis"), violation_key("bad-f"), empty_key("crashed")]
    return pack(f"engines-{which}", keys, seed=4)


# -- budget cases: one key per engine whose search the budget cuts ----------------------------
BUDGET_ENGINES = {"lean": 40, "wide": 64, "xw2": 128, "xw4": 256}


@functools.lru_cache(maxsize=None)
def budget_case(eng):
    return single(f"budget-{eng}", concurrent_key(BUDGET_ENGINES[eng], False, "before", seed=77))


def all_cases():
    """Every case the reference searches (the 2^20 pair is apart: t_limit_case)."""
    for W in WIDTHS:
        yield width_case(W)
    for W in DROPPED_WIDTHS:
        yield dropped_case(W)
    for s in SPANS:
        yield span_case(s, "high")
    for s, how in ((254, "low"), (255, "low"), (4093, "init_high"), (4094, "init_low"), (65_530, "init_low"),
                   (65_531, "init_high"), (65_531, "low")):
        yield span_case(s, how)
    yield wrap_case()
    for n in VALUE_COUNTS:
        yield values_case(n, False)
        yield values_case(n, True)
    for n in LONG_N_OK:
        yield long_case(n, True)
        yield long_case(n, False)
    yield segments_case(False)
    yield segments_case(True)
    yield gaps_case()
    yield violations_case()
    yield one_key_case()
    for w in ENGINE_LISTS:
        yield engines_case(w)
    for e in BUDGET_ENGINES:
        yield budget_case(e)


def big_cases():
    for n in STATES_COUNTS:
        yield states_case(n)


# -- what each case must give (computed once, shared by both test modules) ---------------------
_ref, _orc = {}, {}


def reference(case):
    """lin_ref.check of every key of the case: a list of dicts by key id. The
    keys of the 2^20 pair (how = "t-limit") are replayed, every other searched."""
    import lin_ref as R
    if case.name not in _ref:
        pk = per_key_values(case.cols, case.init)
        ks = range(case.cols.n_keys) if case.keyed else [None]
        _ref[case.name] = [R.check(R.key_rows(case.cols, k), case.init64, per_key=pk,
                                   sequential=case.keys[k or 0].get("how") == "t-limit") for k in ks]
    return _ref[case.name]


def oracle_verdicts(case, algorithm=None, budget=None):
    """The oracle's verdicts (a VERDICT_DTYPE array by key id; one entry for an
    un-keyed case), computed once per (case, algorithm, budget)."""
    from oracle import oracle
    key = (case.name, algorithm, budget)
    if key not in _orc:
        b = budget or case.budget
        if case.keyed:
            _orc[key] = oracle.check_cas_independent(case.cols, init=case.init64, budget=b, threads=8,
                                                     algorithm=algorithm)[0]
        else:
            assert algorithm is None
            d = oracle.check_cas_full(case.cols, init=case.init64, budget=b)
            v = np.zeros(1, A.VERDICT_DTYPE)
            for f in A.VERDICT_FIELDS:
                v[f] = d[f]
            _orc[key] = v
    return _orc[key]


def expected(case, algorithm=None, budget=None):
    """The oracle's verdicts with the two rule outcomes the oracle has no rule
    for put in from the reference: a key of more than 65 532 distinct values
    (UNKNOWN / states) and one of n_ok >= 2^20 - 1 (UNKNOWN / window), both
    settled before any search: nothing explored, no rows."""
    want = oracle_verdicts(case, algorithm, budget).copy()
    for k, r in enumerate(reference(case)):
        if r["cause"] == 8 or (r["cause"] == 2 and r["n_ok"] >= (1 << 20) - 1):
            want[k]["valid"], want[k]["cause"], want[k]["explored"] = A.UNKNOWN, r["cause"], 0
            want[k]["fail_entry"] = want[k]["previous_ok"] = want[k]["last_op"] = -1
    return want
