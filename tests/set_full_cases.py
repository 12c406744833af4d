"""Seeded builders of (checker/set-full) histories (op maps with explicit
:index and :time) that reach the structural edges of jh_setfull.hip (not a
test module). The CPU tests (test_set_full_cases.py) and the GPU tests
(test_gpu_set_full_edges.py) build the same cases from here.

What synth.set_full_history never produces, and these do: element values
with holes over a window of about 4 M at a negative / zero / 2^40 base; three
readers with a read in flight each, completing out of invocation order;
:fail / :info reads and adds, nemesis reads and a nemesis add far outside
the client range; reads that are shuffled, repeat elements, hold values
below, above and between the elements, nil, and elements whose add is not
invoked yet; nil and empty reads; re-invoked adds; :time steps on both
sides of a millisecond from a base near 2^62.

Outcomes are planned per element ("fate") against the ordinal q of a read
among the :ok reads of integer processes in invocation order, which is also
their order by :index:
  normal  present in every read invoked after its acknowledgement
  stale   acknowledged in the prelude, missing from the reads q < hide
  lost    acknowledged in the prelude, present in the reads q < cut only
  never   its add crashes (:info) and no read holds it
  fail    its add fails and no read holds it
  late    added between the reads; some earlier reads already hold it, and
          every other one is read while its add is in flight
  flap    present in every other read or so
"""
import functools

import numpy as np

from jepsen_amd import history as H

STEPS = (1, 999_998, 999_999, 1_000_000, 1_000_001, 2_500_000)
MS = 1_000_000

SF_ELEMS = [1, 63, 64, 65, 255, 256, 257, 300]
SF_READS = [1, 2, 63, 64, 65, 130]
SF_BATCHES = [0, 1, 7, 64, 65]
CHUNK_READ_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193]
CHUNK_ELEMS = 8300
QUANTILE_STABLE = [1, 2, 19, 20, 21, 99, 100, 101, 200]
QUANTILE_LOST = [1, 20, 101]
WORST_STALE = [0, 1, 7, 8, 9, 30]

N_ADDERS, N_READERS = 4, 3
N_PROCS = N_ADDERS + N_READERS
FATES = ("normal", "stale", "lost", "never", "late", "flap", "normal", "fail", "normal", "lost", "normal", "late")
REINVOKED_IDS = (1, 7, 20, 41, 62, 67)          # five in element word 0, one in word 1


def op(process, type_, f, value):
    return {"process": process, "type": type_, "f": f, "value": value}


def stamp(rows, times):
    """The rows as op maps with :index = row and :time."""
    assert len(rows) == len(times)
    return [dict(o, index=i, time=int(t)) for i, (o, t) in enumerate(zip(rows, times))]


def encode(ops):
    """(Columns, time) of op maps. Values are never interned, so a nil inside
    a read's list is JH_NIL in aux and the read's elements stay as written."""
    cols = H.encode(ops, keyed=False, intern_values=False)
    return cols, np.asarray([o["time"] for o in ops], np.int64)


def element_values(m, base, seed):
    """m distinct values of a window of about 4 m at `base`, ascending."""
    rng = np.random.default_rng(seed)
    width = 4 * m if m > 1 else 1
    return [int(base + x) for x in np.sort(rng.choice(width, size=m, replace=False))]


def history(m, n_reads, seed, base=0, time_base=0, values=None, contents="dirty", nil_inside=False,
            faults=True, reinvoke=True):
    """A history of `m` elements and exactly `n_reads` :ok :reads by integer
    processes (module docstring). contents: "sorted" (each read its present
    elements, ascending), "shuffled" (the same, shuffled), "dirty" (shuffled,
    the first three repeated, with a value below the smallest element, one
    above the largest and one in a hole between them; nil too with
    nil_inside). Everything but the reads' contents is the same for the three
    modes of one seed."""
    rng = np.random.default_rng(seed)
    crng = np.random.default_rng(seed + 7919)            # the reads' decoration only
    vals = list(values) if values is not None else element_values(m, base, seed)
    assert len(vals) == m and vals == sorted(set(vals))
    holes = sorted(set(range(vals[0], min(vals[-1], vals[0] + 50_000))) - set(vals))
    R = n_reads
    perm = rng.permutation(m).tolist()
    fate = {e: FATES[k % len(FATES)] for k, e in enumerate(perm)}
    if m < 3:
        fate = {e: "normal" for e in perm}
    early = [e for e in perm if fate[e] == "normal"][:3] if R >= 5 else []
    q0 = 2 if early else 0                                # the nil and the empty read come first
    hide = {e: q0 + 1 + int(rng.integers(max(1, min(3, R - q0 - 1)))) for e in perm}
    cut = {e: q0 + int(rng.integers(max(1, R - q0))) for e in perm}
    reinv = [e for e in REINVOKED_IDS if e < m] if (reinvoke and m >= 63 and R - q0 >= 3) else []
    for e in reinv:
        if fate[e] in ("late", "fail", "never"):
            fate[e] = "normal"
    after = m // 2 if (reinvoke and m >= 3) else None      # re-invoked after the last read
    if after is not None and fate[after] in ("late", "fail", "never"):
        fate[after] = "normal"
    tail = perm[-1] if m >= 4 and perm[-1] not in reinv and perm[-1] != after else None   # first added after it

    rows, forced = [], {}
    applied = np.zeros(m, bool)
    invoked = np.zeros(m, bool)
    adders = list(range(N_ADDERS))
    readers = list(range(N_ADDERS, N_PROCS))
    in_flight = {}                                         # adder slot -> element id
    pending = {}                                           # reader slot -> (kind, snapshot)
    state = {"q": 0, "nem": 0}

    def add_invoke(slot, e):
        rows.append(op(adders[slot], "invoke", "add", vals[e]))
        invoked[e] = True
        applied[e] = fate[e] == "late" and e % 2 == 0      # seen while in flight: known from a read, the :ok :add later
        in_flight[slot] = e

    def add_complete(slot):
        e = in_flight.pop(slot)
        p = adders[slot]
        if fate[e] == "fail":
            rows.append(op(p, "fail", "add", vals[e]))
        elif fate[e] == "never":
            rows.append(op(p, "info", "add", vals[e]))
            adders[slot] = p + N_PROCS                     # a crashed process is replaced
        else:
            rows.append(op(p, "ok", "add", vals[e]))
            applied[e] = True

    def add_all(queue):
        """The adds of `queue`, up to N_ADDERS of them in flight."""
        queue = list(queue)
        while queue or in_flight:
            idle = [s for s in range(N_ADDERS) if s not in in_flight]
            if queue and idle and (not in_flight or rng.random() < 0.6):
                add_invoke(idle[int(rng.integers(len(idle)))], queue.pop(0))
            else:
                busy = list(in_flight)
                add_complete(busy[int(rng.integers(len(busy)))])

    def present(e, q):
        if not invoked[e]:
            return fate[e] == "late" and q % 2 == 0        # held by a read before its add is invoked
        if not applied[e]:
            return False
        f = fate[e]
        if f == "stale":
            return q >= hide[e]
        if f == "lost":
            return q < cut[e]
        if f == "flap":
            return (q + e) % 2 == 0
        return f in ("normal", "late")

    def content(snap):
        els = [vals[e] for e in snap]
        if contents == "sorted":
            return els
        els = [els[i] for i in crng.permutation(len(els))]
        if contents == "dirty":
            els += els[:3] + [vals[0] - 1 - int(crng.integers(5)), vals[-1] + 2]
            if holes:
                els.append(holes[int(crng.integers(len(holes)))])
            if nil_inside:
                els.append(None)
            els = [els[i] for i in crng.permutation(len(els))]
        return els

    def read_invoke(slot, kind="ok"):
        rows.append(op(readers[slot], "invoke", "read", None))
        snap = None
        if kind == "ok":
            q = state["q"]
            state["q"] += 1
            snap = [e for e in range(m) if present(e, q)]
        pending[slot] = (kind, snap)

    def read_complete(slot, value="content"):
        kind, snap = pending.pop(slot)
        p = readers[slot]
        if kind == "ok":
            rows.append(op(p, "ok", "read", content(snap) if value == "content" else value))
        elif kind == "fail":
            rows.append(op(p, "fail", "read", None))
        else:
            rows.append(op(p, "info", "read", None))
            readers[slot] = p + N_PROCS

    def nemesis():
        """Rows the reference skips: not (number? :process)."""
        k = state["nem"]
        state["nem"] += 1
        if k % 3 == 0:
            rows.append(op("nemesis", "info", "start", None))
            rows.append(op("nemesis", "invoke", "read", None))
            rows.append(op("nemesis", "ok", "read", list(vals)))
        elif k % 3 == 1:
            far = vals[-1] + 10 ** 12
            rows.append(op("nemesis", "invoke", "add", far))
            rows.append(op("nemesis", "ok", "add", far))
        else:
            rows.append(op("nemesis", "invoke", "read", None))
            rows.append(op("nemesis", "ok", "read", []))
            rows.append(op("nemesis", "info", "stop", None))

    # the first three elements, then a nil and an empty read, in flight together
    if early:
        add_all(early)
        read_invoke(0)
        read_invoke(1)
        read_complete(1, None)
        read_complete(0, [])
    if faults:
        nemesis()
    prelude = [e for e in perm if fate[e] != "late" and e not in early and e != tail]
    add_all(prelude)
    if faults:
        nemesis()
    late = [e for e in perm if fate[e] == "late" and e != tail]
    n_final = min(N_READERS, R - q0)
    main = R - q0 - n_final                                # :ok reads invoked in the loop below
    redo = {}                                              # ordinal -> elements re-invoked there
    for k, e in enumerate(reinv):
        redo.setdefault(q0 + 1 + (k * (R - q0 - 1)) // len(reinv), []).append(e)
    redo_open = []
    redo_kind = 0
    forced[len(rows)] = 2_500_000                          # acknowledged in the prelude: >= 2 ms before any read

    def add_step():
        idle = [s for s in range(N_ADDERS) if s not in in_flight]
        if late and idle and (not in_flight or rng.random() < 0.5):
            add_invoke(idle[int(rng.integers(len(idle)))], late.pop(0))
        elif in_flight:
            busy = list(in_flight)
            add_complete(busy[int(rng.integers(len(busy)))])

    def redo_step():
        """Re-invoke the elements due at this ordinal, each by a process of its
        own: completed :ok one reader step later, crashed, or never completed."""
        nonlocal redo_kind
        for p, e in redo_open:
            rows.append(op(p, "ok", "add", vals[e]))
        redo_open.clear()
        for e in redo.pop(state["q"], ()):
            p = 1000 + e
            rows.append(op(p, "invoke", "add", vals[e]))
            kind = ("ok", "info", "none")[redo_kind % 3]
            redo_kind += 1
            if kind == "ok":
                redo_open.append((p, e))
            elif kind == "info":
                rows.append(op(p, "info", "add", vals[e]))
            applied[e] = True                              # visible to the reads invoked from here on

    steps = 0
    while state["q"] < R - n_final:
        steps += 1
        slot = int(rng.integers(N_READERS))
        if slot in pending:
            read_complete(slot)
        else:
            u = rng.random() if faults else 1.0
            read_invoke(slot, "fail" if u < 0.06 else "info" if u < 0.12 else "ok")
            redo_step()
        if rng.random() < 0.7:
            add_step()
        if faults and steps % 37 == 0:
            nemesis()
    for slot in [s for s in rng.permutation(N_READERS).tolist() if s in pending]:
        read_complete(slot)
    # the last reads: invoked in ascending, completed in descending process order
    last = sorted(range(N_READERS), key=lambda s: readers[s])[:n_final]
    for slot in last:
        read_invoke(slot)
        redo_step()
        add_step()
    redo_step()
    while late or in_flight:
        add_step()
    for slot in reversed(last):
        read_complete(slot)
    assert state["q"] == R and not pending and not redo, (state, redo)
    if faults:
        nemesis()
    if after is not None:
        rows += [op(adders[0], "invoke", "add", vals[after]), op(adders[0], "ok", "add", vals[after])]
    if tail is not None:
        rows += [op(adders[1], "invoke", "add", vals[tail]), op(adders[1], "ok", "add", vals[tail])]
    step = rng.choice(STEPS, size=len(rows))
    for r, s in forced.items():
        if r < len(rows):
            step[r] = s
    return stamp(rows, time_base + np.cumsum(step.astype(object)))


# -- sweep ----------------------------------------------------------------------
BASES = (0, "negative", 1 << 40)
TIME_BASES = (0, (1 << 62) - 12_345)


@functools.lru_cache(maxsize=None)
def sweep_case(m, r, contents="dirty"):
    """The sweep's history of m elements and r reads: base and time base
    rotate with the shape; every other one carries a nil inside its reads."""
    k = SF_ELEMS.index(m) + SF_READS.index(r) if (m in SF_ELEMS and r in SF_READS) else m + r
    base = BASES[k % 3]
    if base == "negative":
        base = -(2 * m) - 7                                # the window straddles zero
    return history(m, r, seed=1000 * m + r, base=base, time_base=TIME_BASES[k % 2], contents=contents,
                   nil_inside=k % 2 == 1)


def sweep():
    for m in SF_ELEMS:
        for r in SF_READS:
            yield m, r


@functools.lru_cache(maxsize=None)
def overlapping():
    """130 elements, 9 reads by three readers, nothing else in the way."""
    return history(130, 9, seed=42, base=-90, faults=False, reinvoke=False, contents="shuffled")


@functools.lru_cache(maxsize=None)
def reinvoked():
    return history(140, 23, seed=77, base=1 << 40, faults=False, contents="shuffled")


@functools.lru_cache(maxsize=None)
def ignored_rows():
    return history(70, 40, seed=5, base=-30, nil_inside=True)


@functools.lru_cache(maxsize=None)
def sparse(which):
    """Elements far apart: three across a span of 2^20, and 40 over 2^20 at a
    negative base."""
    if which == "three":
        return history(3, 5, seed=3, values=[-5, 1000, (1 << 20) - 6])
    rng = np.random.default_rng(9)
    vals = sorted({int(x) for x in rng.integers(-(1 << 19), 1 << 19, size=40)} | {-(1 << 19), (1 << 19) - 1})
    return history(len(vals), 6, seed=4, values=vals)


# -- read sizes around the bitmap kernel's chunk edges ------------------------------
@functools.lru_cache(maxsize=None)
def chunk_edges():
    """CHUNK_ELEMS acknowledged elements, then one read of each size of
    CHUNK_READ_SIZES: exactly that many aux entries, every one an element,
    none repeated, shuffled; the reads are shuffled too, three in flight.
    Then a read of 4096 and one of 8192 elements padded with values that are
    no elements (entries 4096 + 7 and 8192 + 7), and a last read of all."""
    rng = np.random.default_rng(8300)
    vals = element_values(CHUNK_ELEMS, -1000, 8300)
    m = len(vals)
    rows = []
    for i, v in enumerate(vals):
        rows += [op(i % 4, "invoke", "add", v), op(i % 4, "ok", "add", v)]
    sizes = [CHUNK_READ_SIZES[i] for i in rng.permutation(len(CHUNK_READ_SIZES))]
    reads = [[vals[i] for i in rng.permutation(m)[:k]] for k in sizes]
    for k in (4096, 8192):
        pad = [vals[0] - 3, vals[-1] + 9, vals[-1] + 9] + sorted(set(range(vals[0], vals[0] + 400)) - set(vals))[:4]
        els = [vals[i] for i in rng.permutation(m)[:k]] + pad
        reads.append([els[i] for i in rng.permutation(len(els))])
    reads.append([vals[i] for i in rng.permutation(m)])
    for j in range(0, len(reads), 3):
        group = list(enumerate(reads[j:j + 3]))
        for s, _ in group:
            rows.append(op(4 + s, "invoke", "read", None))
        for s, els in reversed(group):
            rows.append(op(4 + s, "ok", "read", els))
    step = rng.choice(STEPS, size=len(rows))
    return stamp(rows, np.cumsum(step))


# -- planned latencies ----------------------------------------------------------------
def latency_history(stable_lats, lost_lats, seed, extra_never=0):
    """Elements with exactly these stable / lost latencies (ms), by two reads.
    Read X (invoked at time TX) holds the lost elements only, read Y after it
    the stable ones only: a stable element has last-absent = X and
    last-present = Y, a lost one last-present = X and last-absent = Y, so
    either latency is (TX + 1 - time[known]) / 10^6, floored. An element of
    latency i is acknowledged at TX + 1 - i ms - d, d = 0 for odd i (the
    exact millisecond), 999 999 for even i >= 2 (one ns short of the next
    one), 1 for i = 0. Element values are assigned in shuffled order, so
    neither list is sorted by latency. extra_never: elements whose add
    crashes."""
    rng = np.random.default_rng(seed)
    lats = [("s", int(x)) for x in stable_lats] + [("l", int(x)) for x in lost_lats] + [("n", 0)] * extra_never
    m = len(lats)
    vals = element_values(m, -3 * m, seed)
    vals = [vals[i] for i in rng.permutation(m)]
    TX = (max(x for _, x in lats) + 3) * MS + 17
    ack = []
    for (kind, i), v in zip(lats, vals):
        d = 1 if i == 0 else 0 if i % 2 else 999_999
        ack.append((TX + 1 - i * MS - d, kind, v))
    ack.sort(key=lambda a: (a[0], a[2]))
    rows, times = [], []
    for k, (_, kind, v) in enumerate(ack):
        rows.append(op(k, "invoke", "add", v))
        times.append(k)
    for k, (t, kind, v) in enumerate(ack):
        rows.append(op(k, "info" if kind == "n" else "ok", "add", v))
        times.append(t)
    assert times == sorted(times) and times[-1] <= TX
    lost = [v for (kind, _), v in zip(lats, vals) if kind == "l"]
    stable = [v for (kind, _), v in zip(lats, vals) if kind == "s"]
    rows += [op(1000, "invoke", "read", None), op(1000, "ok", "read", lost),
             op(1001, "invoke", "read", None), op(1001, "ok", "read", stable)]
    times += [TX, TX + 5, TX + 9, TX + 11]
    return stamp(rows, times)


def worst_stale_lats(s):
    """s stale latencies and two of 0 ms. 9 and 30: at least three share the
    largest; 30 also has three equal ones across the cut after the 8th."""
    if s >= 30:
        top = [20, 20, 20, 19, 18, 17, 16, 15, 15, 15]
        return [0, 0] + top + [1 + k % 9 for k in range(s - len(top))]
    if s >= 9:
        return [0, 0] + [7, 7, 7] + list(range(1, s - 2))
    return [0, 0] + list(range(1, s + 1))


@functools.lru_cache(maxsize=None)
def quantile_case(c_stable, c_lost):
    return latency_history(range(c_stable), range(c_lost), seed=100 * c_stable + c_lost)


@functools.lru_cache(maxsize=None)
def worst_stale_case(s):
    return latency_history(worst_stale_lats(s), [], seed=500 + s)


@functools.lru_cache(maxsize=None)
def list_cap_case():
    """5 stale of 9 stable, 4 lost and 3 never-read elements."""
    return latency_history([0, 0, 0, 0, 1, 2, 3, 3, 5], [0, 1, 2, 4], seed=12, extra_never=3)


# -- two hand-placed cases, with the answers written out in test_set_full_cases.py -----
T0 = (1 << 62) + 5


def boundary_case():
    """Elements 10, 11, 12: time[last-absent] - time[known] = 999 998, 999 999
    and 1 000 000 ns (0, 1 and 1 ms with the inc of checker.clj:332). Element
    13 is acknowledged 2.5 ms after the read that misses it was invoked: its
    latency clamps to 0 (without the max it is -2 ms)."""
    L = T0 + 3 * MS                                        # read X's invocation
    rows = [(op(0, "invoke", "add", 10), T0), (op(1, "invoke", "add", 11), T0 + 1),
            (op(2, "invoke", "add", 12), T0 + 2),
            (op(2, "ok", "add", 12), L - 1_000_000), (op(1, "ok", "add", 11), L - 999_999),
            (op(0, "ok", "add", 10), L - 999_998),
            (op(5, "invoke", "read", None), L),                            # row 6: X
            (op(3, "invoke", "add", 13), L + 10), (op(3, "ok", "add", 13), L + 2_500_000),   # rows 7, 8
            (op(5, "ok", "read", []), L + 2_500_010),
            (op(5, "invoke", "read", None), L + 2_500_020), (op(5, "ok", "read", [13, 12, 11, 10]), L + 2_500_030)]
    return stamp([o for o, _ in rows], [t for _, t in rows])


def reversed_completion_case():
    """Reads A, B, C invoked at rows 6, 7, 8 by processes 5, 6, 7 and completed
    C, B, A. Element 1 is in A only, 2 in B and C, 3 in A and C, 4 in B only."""
    rows = [op(e - 1, "invoke", "add", e) for e in (1, 2, 3, 4)]
    rows += [op(0, "ok", "add", 1), op(1, "ok", "add", 2)]              # 3 and 4: known from a read
    rows += [op(5, "invoke", "read", None), op(6, "invoke", "read", None), op(7, "invoke", "read", None)]
    rows += [op(7, "ok", "read", [3, 2]), op(6, "ok", "read", [4, 2]), op(5, "ok", "read", [1, 3])]
    return stamp(rows, [i * 2 * MS for i in range(len(rows))])
