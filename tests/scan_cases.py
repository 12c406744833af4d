"""Seeded builders of counter, set and queue histories (op maps) that reach
the structural edges of the scan kernels (not a test module). The CPU tests
(test_scan_refs.py) and the GPU tests (test_gpu_scan_edges.py) build the same
cases from here.

Two rules keep the counter cases decidable by the reference: every operation
is completed before the history ends, and a nil invocation value is given
only to an :add that completes :ok or :fail. (A crashed add with a nil value
is (+ upper nil): the whole history is :unknown and a comparison of it checks
nothing.)
"""
import numpy as np

from jepsen_amd import history as H

inv = H.invoke_op
ok = H.ok_op
fail = H.fail_op
info = H.info_op


def encode(ops, proc_offset=0):
    """(ops', cols): the columns of `ops` with every process id shifted by
    proc_offset, and the op maps with the same shifted ids (encode itself
    renumbers negative ids, so the shift is applied to its output)."""
    cols = H.encode(ops, keyed=False)
    if proc_offset:
        cols.process = cols.process + np.int64(proc_offset)
        ops = [dict(o, process=o["process"] + proc_offset) for o in ops]
    return ops, cols


# -- counter ------------------------------------------------------------------
COUNTER_VALUE_SETS = {
    "small": [1, -1, 3],
    "field-edges": [(1 << 26) - 1, 1 << 26, -(1 << 26), -(1 << 26) - 1, 5],
    "wide": [1 << 40, -(1 << 40), 7],
    "zero-one": [0, 1],
}
COUNTER_ROWS = [1, 2, 7, 2047, 2048, 2049, 4096, 4097, 6150]
COUNTER_PROCS = [1, 3, 33, 70]


def counter_random(n_rows, n_procs, values, seed, p_nil=0.2, p_fail=0.06, p_info=0.04, p_read=0.15,
                   p_bad=0.05, read_inv_value=False):
    """Exactly n_rows rows over processes 0..n_procs-1: adds with values drawn
    from `values` (p_nil of their invocations carry nil, the completion the
    value), reads of the acknowledged sum (p_bad of them off by +-1000), :fail
    completions and stray :info rows before a completion. Every invocation is
    completed."""
    rng = np.random.default_rng(seed)
    ops, open_, acked = [], {}, 0
    idle = list(range(n_procs))

    def complete(p):
        nonlocal acked
        f, v, nil = open_.pop(p)
        idle.append(p)
        if f == "read":
            ops.append(ok(p, "read", v) if rng.random() >= p_fail else fail(p, "read", None))
        elif rng.random() < p_fail:
            ops.append(fail(p, "add", v))
        else:
            ops.append(ok(p, "add", v))
            acked += v

    while len(ops) + len(open_) < n_rows:
        room = n_rows - len(ops) - len(open_)
        if idle and room >= 2 and (not open_ or rng.random() < 0.55):
            p = idle.pop(int(rng.integers(len(idle))))
            if rng.random() < p_read:
                v = acked + (0 if rng.random() >= p_bad else int(rng.choice([-1000, 1000])))
                open_[p] = ("read", v, True)
                ops.append(inv(p, "read", v if read_inv_value else None))
            else:
                v = int(values[int(rng.integers(len(values)))])
                nil = rng.random() < p_nil
                open_[p] = ("add", v, nil)
                ops.append(inv(p, "add", None if nil else v))
        elif open_:
            p = list(open_)[int(rng.integers(len(open_)))]
            if room >= 1 and rng.random() < p_info:
                ops.append(info(p, open_[p][0], None))      # not a completion: the op stays open
            else:
                complete(p)
        else:
            ops.append(info(idle[0], "add", None))          # one odd row left: nothing is open
    for p in list(open_):
        complete(p)
    assert len(ops) == n_rows
    return ops


def counter_many_processes(n_procs=1100, seed=5):
    """n_procs invocations by as many processes, then their completions: the
    first 2048 rows hold more distinct processes than the 1024-slot process
    table of a chunk. Every 9th op is a read, every 5th add is invoked nil,
    every 7th add value lies outside the 27-bit field."""
    rng = np.random.default_rng(seed)
    head, tail, acked = [], [], 0
    order = rng.permutation(n_procs)
    kind = {}
    for p in range(n_procs):
        if p % 9 == 4:
            kind[p] = ("read", None)
            head.append(inv(p, "read", None))
        else:
            v = (1 << 30) + p if p % 7 == 0 else 1 + p % 3
            kind[p] = ("add", v)
            head.append(inv(p, "add", None if p % 5 == 0 else v))
    for p in order.tolist():
        f, v = kind[p]
        if f == "add":
            tail.append(ok(p, "add", v))
            acked += v
        else:
            tail.append(ok(p, "read", acked if p % 2 else acked + (1 << 50)))
    return head + tail


def counter_reads_at(n_rows, reads, bad=-7):
    """A filler of unit adds by three processes with reads placed at exact
    rows: reads = [(invoke row, ok row, is_bad)]. A bad read returns `bad`
    (below every lower bound here); a good one the acknowledged sum at its
    completion. Each read has a process of its own."""
    slots = [None] * n_rows
    for k, (r_inv, r_ok, is_bad) in enumerate(reads):
        assert r_inv < r_ok and slots[r_inv] is None and slots[r_ok] is None
        slots[r_inv] = inv(100 + k, "read", None)
        slots[r_ok] = ("read", 100 + k, is_bad)
    free = [i for i, s in enumerate(slots) if s is None]
    for j in range(0, len(free) - 1, 2):
        p = (j // 2) % 3
        slots[free[j]] = inv(p, "add", 1)
        slots[free[j + 1]] = ok(p, "add", 1)
    if len(free) % 2:
        slots[free[-1]] = info(0, "add", None)
    acked = 0
    for i, s in enumerate(slots):
        if isinstance(s, tuple):
            slots[i] = ok(s[1], "read", bad if s[2] else acked)
        elif s["type"] == "ok" and s["f"] == "add":
            acked += 1
    return slots


def counter_big_adds(value, k):
    """k acknowledged adds of `value` and one read of their sum (of `value`
    when the sum is past a long: the reference throws before it gets there)."""
    ops = []
    for i in range(k):
        ops += [inv(i % 2, "add", value), ok(i % 2, "add", value)]
    return ops + [inv(5, "read", None), ok(5, "read", k * value if k * value < 1 << 63 else value)]


# -- set ----------------------------------------------------------------------
def set_history(elements, seed, read=None, order="asc", twice=False, p_fail=0.06, p_info=0.08, n_lost=3,
                n_unexpected=2, earlier_reads=(), later_reads=True):
    """One :add per entry of `elements` (an element listed twice is attempted
    twice), acknowledged, failed or crashed; then the final :ok :read of
    `read` (default: every acknowledged element but n_lost of them, every
    other crashed one, and n_unexpected elements nobody attempted), listed
    ascending / descending / shuffled, each element twice with `twice`.
    earlier_reads: element lists of :ok :reads before the final one;
    later_reads: an :info and a :fail read after it."""
    rng = np.random.default_rng(seed)
    ops, acked, crashed = [], [], []
    for i, e in enumerate(elements):
        p = i % 10
        ops.append(inv(p, "add", e))
        u = rng.random()
        if u < p_fail:
            ops.append(fail(p, "add", e))
        elif u < p_fail + p_info:
            ops.append(info(p, "add", e))
            crashed.append(e)
        else:
            ops.append(ok(p, "add", e))
            acked.append(e)
        if earlier_reads and i == len(elements) // 2:
            for er in earlier_reads:
                ops += [inv(11, "read", None), ok(11, "read", list(er))]
    if read is None:
        lost = set(rng.choice(acked, size=min(n_lost, len(acked)), replace=False).tolist()) if acked else set()
        read = [e for e in dict.fromkeys(acked) if e not in lost] + crashed[::2]
        hi = max(elements) if len(elements) else 0
        read += [hi + 3 + 2 * k for k in range(n_unexpected)]
        read = list(dict.fromkeys(read))
    read = [int(x) for x in read]
    if order == "asc":
        read = sorted(read)
    elif order == "desc":
        read = sorted(read, reverse=True)
    else:
        read = [read[i] for i in rng.permutation(len(read))]
    if twice:
        read = [x for e in read for x in (e, e)] if order != "shuffled" else read + read[::-1]
    ops += [inv(12, "read", None), ok(12, "read", read)]
    if later_reads:
        ops += [inv(12, "read", None), info(12, "read", None), inv(13, "read", None), fail(13, "read", None)]
    return ops


def gapped(m, vmin=0, run=100, gap=3):
    """m elements from vmin in runs of `run` consecutive ones, `gap` apart:
    runs cross the 32-element word edges and every bucket edge."""
    return [vmin + i + (i // run) * gap for i in range(m)]


def set_read_size(k, seed=1, vmin=0):
    """A final read of exactly k elements in a span of more than 8192
    elements (so a bucket holds more than 32 of them), small enough for the
    history to stay on the dense path."""
    m = 3000 + k + k // 4               # about 11% of the adds are not acknowledged
    els = [vmin + 3 * i for i in range(m)] if k < 4000 else gapped(m, vmin)
    ops = set_history(els, seed, read=[], p_info=0.05, later_reads=False)
    acked = [o["value"] for o in ops if o["type"] == "ok" and o["f"] == "add"]
    read = acked[5:5 + k - min(k, 2)] + [els[-1] + 1, els[-1] + 4][:min(k, 2)]
    assert len(read) == k
    ops[-1] = ok(12, "read", read)
    return ops


def set_runs(vmin):
    """Named runs at offsets from vmin (itself an element): 30..34 (over a word edge), 60..70 (over
    the bucket edge at 64 of 64-element buckets), 200..299 (100 consecutive
    elements, four words), a filler of every 7th element and 9990..9999 to fix
    the span at 10000 (dense: the filler makes the history long enough). One
    filler element is lost, offset 40 is a crashed add that is read
    (recovered), offset 5 is read and never attempted (unexpected)."""
    offs = [0] + list(range(30, 35)) + list(range(60, 71)) + list(range(200, 300)) + list(range(1000, 9000, 7)) + \
        list(range(9990, 10000))
    read = [vmin + o for o in offs if o != 1021] + [vmin + 40, vmin + 5]
    return [inv(9, "add", vmin + 40), info(9, "add", vmin + 40)] + \
        set_history([vmin + o for o in offs], seed=3, read=read, p_fail=0.0, p_info=0.0)


def set_switch(side):
    """One history on either side of the dense / sparse switch (span <= 8 (n +
    cnt) + 4096). side None: the base history; "dense": one far element,
    attempted, acknowledged and read, that makes the span exactly the bound;
    "sparse": one element further."""
    base = set_history(gapped(2000, vmin=-40), seed=8, order="shuffled", later_reads=False)
    if side is None:
        return base
    read = base[-1]["value"]
    n, cnt = len(base) + 2, len(read) + 1
    vmin = min(min(read), -40)
    bound = 8 * (n + cnt) + 4096
    far = vmin + bound - 1 + (1 if side == "sparse" else 0)      # span = far - vmin + 1
    return base[:-2] + [inv(3, "add", far), ok(3, "add", far), base[-2], ok(12, "read", read + [far])]


# -- queue --------------------------------------------------------------------
def queue_history(values, seed, n_ops=600, p_nil=0.0, drains=(), p_fail=0.08, p_info=0.05, p_unexpected=0.03,
                  p_dup=0.04):
    """Enqueues and dequeues of elements of `values` (p_nil of them nil):
    enqueues acknowledged, failed or crashed; dequeues of enqueued values,
    some twice, some never enqueued. `drains`: value lists (or None) of
    :ok :drain ops placed evenly; the history ends in a :fail :drain."""
    rng = np.random.default_rng(seed)
    values = list(values)
    ops, pending, seen = [], [], []

    def pick():
        return None if rng.random() < p_nil else values[int(rng.integers(len(values)))]

    drain_at = {int((k + 1) * n_ops / (len(drains) + 1)): d for k, d in enumerate(drains)}
    for i in range(n_ops):
        p = i % 7
        if i in drain_at:
            ops += [inv(8, "drain", None), ok(8, "drain", drain_at[i])]
        if not pending or rng.random() < 0.55:
            v = pick()
            ops.append(inv(p, "enqueue", v))
            u = rng.random()
            ops.append(fail(p, "enqueue", v) if u < p_fail else info(p, "enqueue", v) if u < p_fail + p_info
                       else ok(p, "enqueue", v))
            pending.append(v)
            seen.append(v)
        else:
            u = rng.random()
            if u < p_unexpected:
                v = pick()
            elif u < p_unexpected + p_dup:
                v = seen[int(rng.integers(len(seen)))]
            else:
                v = pending.pop(int(rng.integers(len(pending))))
            ops.append(inv(p, "dequeue", None))
            ops.append(ok(p, "dequeue", v) if rng.random() >= p_fail else fail(p, "dequeue", None))
    ops += [inv(8, "drain", None), fail(8, "drain", None)]
    return ops


def queue_span(S, seed, clean=False):
    """Values over a span of exactly S - 1 (both ends used), with nil enqueued
    and dequeued: the device's value table has S slots, nil the last one.
    clean: every dequeue takes a pending value, so the queue model accepts
    the history and returns its final queue."""
    span = S - 1
    rng = np.random.default_rng(seed)
    vals = sorted({0, span - 1} | set(rng.integers(0, span, size=min(span, 150)).tolist()))
    ops = queue_history(vals, seed, n_ops=400, p_nil=0.1, **(dict(p_unexpected=0.0, p_dup=0.0) if clean else {}))
    for v in [0, span - 1, span - 1, None, None]:      # both ends and nil surely present
        ops += [inv(0, "enqueue", v), ok(0, "enqueue", v)]
    ops += [inv(1, "dequeue", None), ok(1, "dequeue", span - 1), inv(1, "dequeue", None), ok(1, "dequeue", None)]
    return ops


def long_drain(k, seed):
    """Enqueues of 0..k/2, then one :ok :drain of k elements: duplicates,
    values never enqueued, and a nil element."""
    rng = np.random.default_rng(seed)
    ops = []
    for v in range(k // 2):
        ops += [inv(v % 5, "enqueue", v), ok(v % 5, "enqueue", v) if v % 11 else info(v % 5, "enqueue", v)]
    els = rng.integers(0, k // 2 + 40, size=k).tolist()
    els[k // 3] = None
    return ops + [inv(6, "drain", None), ok(6, "drain", els)]


def many_drains(n_drains=70_000, seed=4):
    """n_drains :ok :drain rows of zero or one element over 0..120, after
    enqueues of 0..99."""
    rng = np.random.default_rng(seed)
    ops = []
    for v in range(100):
        ops += [inv(v % 5, "enqueue", v), ok(v % 5, "enqueue", v)]
    els = rng.integers(0, 121, size=n_drains).tolist()
    empty = rng.random(n_drains) < 0.3
    for i in range(n_drains):
        ops += [inv(6, "drain", None), ok(6, "drain", [] if empty[i] else [els[i]])]
    return ops


# -- the cases both test modules run -------------------------------------------
def counter_sweep(vs_name, n_procs):
    """(id, ops) for every row count of COUNTER_ROWS, one value set and one
    process count; the two longest also with reads invoked with their value."""
    values = COUNTER_VALUE_SETS[vs_name]
    for n_rows in COUNTER_ROWS:
        seed = n_rows * 131 + n_procs * 7 + len(vs_name)
        yield f"{vs_name}-p{n_procs}-n{n_rows}", counter_random(n_rows, n_procs, values, seed,
                                                                 read_inv_value=n_rows in (4097, 6150))


COUNTER_EDGE_CASES = {
    "completed-history-reads": lambda: counter_random(3000, 5, [1, -1, 3], 77, read_inv_value=True),
    "many-processes": counter_many_processes,
    # invocation at row 2000 (chunk 0), completion at row 2100 (chunk 1)
    "error-read-across-chunks": lambda: counter_reads_at(4200, [(2000, 2100, True), (10, 20, False),
                                                                (3000, 4150, False)]),
    # errors on both sides of the edges at 2048 and 4096; the smallest row is 2046
    "errors-around-chunk-edges": lambda: counter_reads_at(
        4300, [(2040, 2046, True), (2041, 2047, True), (2042, 2048, True), (2043, 2050, True),
               (4000, 4095, True), (4001, 4096, True), (100, 4200, False)]),
    "late-first-error": lambda: counter_reads_at(6150, [(5, 9, False), (4090, 4097, True), (4091, 6000, True)]),
}


def _twice(els, seed):
    rng = np.random.default_rng(seed)
    both = list(els) + list(els)
    return [both[i] for i in rng.permutation(len(both))]


SET_CASES = {
    "asc": lambda: set_history(gapped(3001), 1, order="asc"),
    "desc": lambda: set_history(gapped(3001), 2, order="desc"),
    "shuffled": lambda: set_history(gapped(3001), 3, order="shuffled"),
    "read-twice-asc": lambda: set_history(gapped(3000), 4, order="asc", twice=True),
    "read-twice-shuffled": lambda: set_history(gapped(3000), 5, order="shuffled", twice=True),
    "attempted-twice": lambda: set_history(_twice(gapped(1500), 6), 6),
    "earlier-reads": lambda: set_history(gapped(2500), 7, earlier_reads=([-500, 7, 8], [100_000, 3])),
    "vmin-neg-1000": lambda: set_runs(-1000),
    "vmin-17": lambda: set_runs(17),
    "odd-n": lambda: set_history(gapped(777), 9)[:-1],
    "switch-base": lambda: set_switch(None),
    "switch-dense": lambda: set_switch("dense"),
    "switch-sparse": lambda: set_switch("sparse"),
}
SET_READ_SIZES = [0, 1, 8191, 8192, 8193, 16385]
for _k in SET_READ_SIZES:
    SET_CASES[f"read-{_k}"] = (lambda k: lambda: set_read_size(k, seed=k % 97))(_k)

QUEUE_SPANS = [2, 3, 1 << 8, (1 << 8) + 1, 1 << 16, (1 << 16) + 1]
DRAIN_SIZES = [4095, 4096, 4097, 9000]
QUEUE_CASES = {
    "neg-50-50": lambda: queue_history(range(-50, 51), 1, n_ops=1500, p_nil=0.05),
    "sparse-2^24": lambda: queue_history([k * ((1 << 24) // 37) for k in range(37)] + [(1 << 24) - 1], 2, n_ops=900),
    "nil-values": lambda: queue_history(range(5), 3, n_ops=300, p_nil=0.4),
    "drains": lambda: queue_history(range(-9, 30), 4, n_ops=500, drains=([], None, [3, 3, None, 500, -9], [])),
}
for _s in QUEUE_SPANS:
    QUEUE_CASES[f"S-{_s}"] = (lambda s: lambda: queue_span(s, seed=s % 89))(_s)
    QUEUE_CASES[f"S-{_s}-clean"] = (lambda s: lambda: queue_span(s, seed=s % 83, clean=True))(_s)
for _d in DRAIN_SIZES:
    QUEUE_CASES[f"drain-{_d}"] = (lambda d: lambda: long_drain(d, seed=d))(_d)
