"""The set-full kernels (jh_setfull.hip) at their structural edges against the
op-map fold (oracle/set_full.py, pinned by the reference's known answers),
every field of the result map, exactly. The cases come from
set_full_cases.py; test_set_full_cases.py checks the same cases between the
two CPU restatements without a device, and that they do not degenerate.

Which input takes which branch is argued from the kernels' code in each
docstring: one bitmap word and one wave of k_sf_elem hold 64 elements, one
workgroup 256; k_sf_elem steps through 64 reads per readlane round;
k_sf_bits takes BITS_CHUNK = 4096 aux entries per workgroup, 256 x
BITS_UNROLL = 1024 per pass of its loop and 64 per run_or.
"""
import types

import numpy as np
import pytest

import set_full_cases as C
from hipcols import DevCols
from jepsen_amd import _abi as A
from jepsen_amd import checker
from jepsen_amd._native import JhError
from oracle import set_full as SF

pytestmark = pytest.mark.gpu

_want = {}


def _flat_worst(m):
    m = dict(m)
    m["worst-stale"] = [(r["element"], r["stable-latency"], r["known"]["index"],
                         r["last-absent"]["index"] if r["last-absent"] else -1) for r in m["worst-stale"]]
    return m


def want_of(key, ops, lin=False):
    """The fold's answer, computed once per case."""
    if (key, lin) not in _want:
        _want[key, lin] = _flat_worst(SF.set_full(ops, linearizable=lin))
    return _want[key, lin]


def _reads(ops):
    return [o for o in ops if o["type"] == "ok" and o["f"] == "read" and isinstance(o["process"], int)]


def device_same(ctx, key, ops, lin=False, batches=(0,)):
    """Both routes against the fold: the columns through ctx.check_set_full
    (every read_batch of `batches`) and the op maps through the Checker. A
    history with a nil inside a read's list has no Checker route (it takes
    integer elements only) and is checked through the columns alone."""
    want = want_of(key, ops, lin)
    cols, time = C.encode(ops)
    reads = _reads(ops)
    raw = None
    for b in batches:
        r = ctx.check_set_full(cols, time, linearizable=lin, read_batch=b)
        got = _flat_worst(checker.set_full_result(r, cols, time))
        assert got == want, (key, b, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]})
        assert r["n_reads"] == len(reads), (key, b)
        assert r["read_elements"] == sum(len(o["value"] or ()) for o in reads), (key, b)
        assert r["stable_count"] + r["lost_count"] + r["never_read_count"] == r["attempt_count"], (key, b)
        for _, _, known, la in r["worst_stale"]:
            assert ops[known]["type"] == "ok" and ops[known]["f"] in ("add", "read"), (key, b)
            assert la < 0 or (ops[la]["type"], ops[la]["f"]) == ("invoke", "read"), (key, b)
        raw = raw or r
    sf = checker.set_full({"linearizable?": lin})
    if any(None in (o["value"] or ()) for o in reads):
        with pytest.raises(TypeError):
            sf.check({}, ops, {})
    else:
        assert _flat_worst(sf.check({}, ops, {})) == want, key
    return want, raw, cols, time


# R and R + 1 join SF_BATCHES: 65 reads in batches of 64 (the second batch one
# read, k_sf_elem's lo = 0 of nb = 1), of 7 (65 = 9 * 7 + 2), of 66 (> R)
CROSS = {1: 1, 63: 2, 64: 64, 65: 65, 255: 65, 256: 64, 257: 130, 300: 63}


@pytest.mark.parametrize("m", C.SF_ELEMS)
def test_sf_sweep(ctx, m):
    """M elements x R reads, M and R around 64 and 256.

    M = 63 / 64 / 65: the last lane of k_sf_elem's only wave dead (live =
    false, LLONG_MAX in the amin reduction), the wave full, a second wave with
    one live lane and a second bitmap word (W = 2). 255 / 256 / 257: the same
    at the workgroup edge (gridDim.x = 1, 1, 2). R = 63 / 64 / 65 / 130: kmax
    = 63, one full readlane round, a second round of one read, a third of two.
    R = 1, 2: the binary search on one and two reads.
    Element values have holes (elem_id: lut = -1), every read holds a value
    below vmin, one above vmax and, in every other case, JH_NIL (the range
    test before the LUT load), repeats and shuffled order (run_or: many short
    runs, b ORed twice). Bases -2 M, 0 and 2^40: value - vmin with vmin
    negative and large. With R >= 5 the first two reads are a nil and an empty
    one (cnt = 0: k_sf_bits returns, the word stays 0) that complete before
    most adds are invoked (row > a false for those elements). Some elements
    are read while their add is in flight (known_read < known_add in
    k_sf_final), some before it is invoked (a set bit with row < a). With M >=
    255 and R <= 2 a read's invocation lies more than 64 rows back (k_sf_inv's
    second ballot). Times start near 2^62 in every other case.

    The reduced cross with read_batch: one (M, R) per M through SF_BATCHES, R
    and R + 1. The bitmap is [W][batch] and rewritten per batch: a batch of 7
    does not divide 65, 64 leaves one read for the second batch (nb = 1 with
    NB = 64), R + 1 is capped to R by the host."""
    for r in C.SF_READS:
        ops = C.sweep_case(m, r)
        want, raw, _, _ = device_same(ctx, ("sweep", m, r), ops)
        assert raw["attempt_count"] == m
        if m >= 63 and r >= 2:
            assert want["valid?"] != "unknown"
    r = CROSS[m]
    device_same(ctx, ("sweep", m, r), C.sweep_case(m, r), batches=C.SF_BATCHES[1:] + [r, r + 1])
    device_same(ctx, ("sweep", m, r), C.sweep_case(m, r), lin=True, batches=(0, 7))


@pytest.mark.parametrize("batch", [0, 3])
def test_sf_chunk_edges(ctx, batch):
    """8 300 elements; reads of exactly 0 .. 8193 aux entries, every one an
    element, shuffled. k_sf_bits: gx = 3 workgroups per read (max_cnt 8300);
    a read of 4096 fills workgroup 0 and workgroup 1 returns at base >= cnt,
    4097 gives workgroup 1 a single entry (one live lane: v = JH_NIL in the
    others, w = -1, a run of 63 that stores nothing), 8193 the same for
    workgroup 2. 1023 / 1024 / 1025: one pass of the g loop short of a lane,
    full, and a second pass for wave 0 only. 63 / 64 / 65 and 255 / 256 /
    257: the last of the BITS_UNROLL groups of a wave, and the waves of a
    workgroup. Shuffled elements over W = 130 words: up to 64 runs per
    run_or, each of one lane. Two reads are padded with values that are no
    elements (below vmin, above vmax, in holes, one repeated). read_batch 3:
    20 reads in 7 batches, the last of 2."""
    ops = C.chunk_edges()
    want, raw, _, _ = device_same(ctx, "chunk-edges", ops, batches=(batch,))
    assert raw["attempt_count"] == C.CHUNK_ELEMS and raw["n_reads"] == len(C.CHUNK_READ_SIZES) + 3
    assert want["stable-count"] == C.CHUNK_ELEMS


def test_sf_read_order_is_irrelevant(ctx):
    """One history three ways: every read sorted (run_or sees one or two long
    runs per wave), shuffled (runs of one lane, the same word met again in
    later runs and later waves: atomicOr), and shuffled with repeats and
    values that are no elements (w = -1 runs between the others). The three
    device results are the same map, and the fold's."""
    res = {}
    for contents in ("sorted", "shuffled", "dirty"):
        ops = C.history(130, 20, seed=21, base=-77, contents=contents)
        want, raw, _, _ = device_same(ctx, ("order", contents), ops, batches=(0, 7))
        res[contents] = ({k: v for k, v in raw.items() if k not in ("device_ms", "read_elements", "lost",
                                                                    "never_read", "stale")},
                         [raw[k].tolist() for k in ("lost", "never_read", "stale")], want)
    assert res["sorted"] == res["shuffled"] == res["dirty"]
    assert res["sorted"][2]["stale-count"] > 0 and res["sorted"][2]["lost-count"] > 0


def test_sf_overlapping_reads(ctx):
    """Three readers with a read in flight each; the last three complete in
    descending order of invocation. k_sf_elem walks the reads in row order
    of their :ok, so inv is not monotone along the walk: lp = max(lp, inv)
    and la = max(la, inv) keep the invocation of greater :index
    (checker.clj:266-280), which "the latest row wins" does not
    (test_set_full_cases.py shows that the two differ here). k_sf_inv: each
    :ok read's invocation is its process' previous row, several rows back and
    past other readers' rows. The hand-written reversed-completion case has
    its expected map in test_set_full_cases.py."""
    device_same(ctx, "overlapping", C.overlapping(), batches=(0, 1, 4))
    ops = C.reversed_completion_case()
    want, _, _, _ = device_same(ctx, "reversed-completion", ops, batches=(0, 1, 2))
    assert (want["lost"], want["never-read"], want["stale"]) == ([1], [4], [2])


@pytest.mark.parametrize("batch", [0, 1, 7])
def test_sf_reinvoked_adds(ctx, batch):
    """Five elements of word 0 and one of word 1 are invoked again at
    different rows between the reads, one after the last read. k_sf_addinv
    keeps the last invocation (atomicMax); k_sf_okadd must skip the :ok :add
    that precedes it (r > last_inv[id]), else known is the first add's.
    k_sf_elem starts at the first read after amin, the wave's smallest last
    invocation, which is below the own a of the re-invoked lanes: only row > a
    keeps their earlier reads out. With read_batch 1 and 7 the binary search
    runs per batch, and batches before amin return at lo >= nb. The element
    invoked again after the last read has no read left: never-read, known
    from the new :ok (state from the 0xff fill and k_sf_okadd alone)."""
    device_same(ctx, "reinvoked", C.reinvoked(), batches=(batch,))


def test_sf_ignored_rows(ctx):
    """Rows the reference skips: :fail and :info reads (read_flag = 0; the
    reader's next read is by a new process after :info), :fail and :info adds
    (their :invoke still makes the element), nemesis reads of every element
    and of none (proc < 0: not counted in n_reads, not flagged), and a nemesis
    add 10^12 above the client range, which must not move vmax (a span past
    2^31 would be refused) nor count as an attempt. Every read holds a nil."""
    ops = C.ignored_rows()
    want, raw, _, _ = device_same(ctx, "ignored-rows", ops, batches=(0, 5))
    assert raw["attempt_count"] == 70
    far = max(o["value"] for o in ops if o["process"] == "nemesis" and o["f"] == "add")
    assert far not in want["never-read"] + want["lost"] + want["stale"]


@pytest.mark.parametrize("which", ["three", "forty"])
def test_sf_sparse_and_negative_elements(ctx, which):
    """Three elements over a span of 2^20 (flag / LUT of 2^20 entries, the
    exclusive scan over them, ids 0, 1, 2 far apart), and 42 over the same
    span from -2^19 (v - vmin with both signs)."""
    ops = C.sparse(which)
    want, raw, _, _ = device_same(ctx, ("sparse", which), ops, batches=(0, 2))
    els = sorted({o["value"] for o in ops if o["f"] == "add" and isinstance(o["process"], int)})
    assert raw["attempt_count"] == len(els) and els[-1] - els[0] + 1 == 1 << 20


def test_sf_latency_boundaries(ctx):
    """time[last-absent] - time[known] = 999 998 / 999 999 / 1 000 000 ns: 0 /
    1 / 1 ms only with the inc of k_sf_final (time[la] + 1); an element known
    after the invocation of the read that misses it: max(.., 0). Times lie
    just above 2^62. The expected map is written out in
    test_set_full_cases.py."""
    want, raw, _, _ = device_same(ctx, "boundary", C.boundary_case(), batches=(0, 1))
    assert want["stale"] == [11, 12] and want["worst-stale"] == [(12, 1, 3, 6), (11, 1, 4, 6)]
    assert raw["stable_latencies"] == [0, 1, 1, 1, 1]


@pytest.mark.parametrize("c", C.QUANTILE_STABLE)
def test_sf_quantiles(ctx, c):
    """c stable elements of latencies 0 .. c-1 ms, not in element order: the
    pick at floor(c p) (min c - 1) of the radix-sorted latencies, around c =
    20 and 100 where floor(0.95 c) and floor(0.99 c) step. Latency i is
    reached at exactly i ms for odd i and at i ms + 999 999 ns for even i.
    The same for the lost latencies at c = 1, 20, 101."""
    want, raw, _, _ = device_same(ctx, ("quantile", c, 0), C.quantile_case(c, 0))
    assert raw["stable_latencies"] == [0, c // 2, min(c - 1, int(np.floor(c * 0.95))),
                                       min(c - 1, int(np.floor(c * 0.99))), c - 1]
    if c in C.QUANTILE_LOST:
        want, raw, _, _ = device_same(ctx, ("quantile", 3, c), C.quantile_case(3, c))
        assert raw["has_lost_latencies"] and raw["lost_latencies"][4] == c - 1 and raw["lost_count"] == c


@pytest.mark.parametrize("s", C.WORST_STALE)
def test_sf_worst_stale(ctx, s):
    """s stale elements: none (no sort, n_worst = 0), fewer than, exactly and
    more than JH_SF_WORST. k_sf_worst takes the last entries of the (latency,
    id) pairs sorted by latency with a stable radix sort, reversed (src = ns -
    1 - i): among equal latencies the larger element first, as (reverse
    (sort-by :stable-latency ..)). 9 and 30 have three elements at the
    largest latency, 30 three across the cut after the 8th."""
    want, raw, _, _ = device_same(ctx, ("worst", s), C.worst_stale_case(s))
    assert raw["stale_count"] == s and raw["n_worst"] == min(s, 8)
    if s >= 9:
        w = raw["worst_stale"]
        assert w[0][1] == w[1][1] == w[2][1] and w[0][0] > w[1][0] > w[2][0]


def test_sf_linearizable_option(ctx):
    """Stale elements and none lost: valid, and invalid with :linearizable?."""
    ops = C.worst_stale_case(7)
    want, _, _, _ = device_same(ctx, ("worst", 7), ops)
    assert want["valid?"] is True and want["lost-count"] == 0 and want["stale-count"] == 7
    want, _, _, _ = device_same(ctx, ("worst", 7), ops, lin=True)
    assert want["valid?"] is False
    ops = C.worst_stale_case(0)
    assert device_same(ctx, ("worst", 0), ops, lin=True)[0]["valid?"] is True


def test_sf_list_cap(ctx):
    """4 lost, 3 never-read, 5 stale elements: with list_cap 0, 1, count - 1,
    count and count + 1 of each, the counts, quantiles and worst-stale are
    those of the full result and each list is its sorted prefix."""
    ops = C.list_cap_case()
    want, full, cols, time = device_same(ctx, "list-cap", ops)
    names = ("lost", "never_read", "stale")
    counts = [full[k + "_count"] for k in names]
    assert counts == [4, 3, 5]
    for k in names:
        assert full[k].tolist() == want[k.replace("_", "-")] == sorted(full[k].tolist())
    for cap in sorted({0, 1} | {c + d for c in counts for d in (-1, 0, 1)}):
        r = ctx.check_set_full(cols, time, list_cap=cap)
        for k in r:
            if k not in names + ("device_ms",):
                assert r[k] == full[k], (cap, k)
        for k in names:
            assert r[k].tolist() == full[k][:cap].tolist(), (cap, k)


def test_sf_device_resident(ctx):
    """The columns and the :time column already in device memory
    (on_device = 1: no staging, the pointers as given, 8-byte aligned only):
    the result of the host-buffer call."""
    ops = C.sweep_case(257, 65)
    want, host, cols, time = device_same(ctx, ("sweep", 257, 65), ops)
    dev = DevCols(cols, shift=1)
    z = np.zeros(1, np.int64)
    # a second staging whose first column is the :time column
    dtime = DevCols(types.SimpleNamespace(n=cols.n, n_keys=0, process=time, type=z, f=z, key=z, value=z, value2=z,
                                          aux=z), shift=1)
    for batch in (0, 64):
        r = ctx.check_set_full(dev, dtime.process, on_device=True, read_batch=batch)
        for k in r:
            if k in ("lost", "never_read", "stale"):
                assert r[k].tolist() == host[k].tolist(), k
            elif k != "device_ms":
                assert r[k] == host[k], k
        assert _flat_worst(checker.set_full_result(r, cols, time)) == want


def _raises(ctx, code, ops=None, cols=None, time=None):
    if cols is None:
        cols, time = C.encode(ops)
    with pytest.raises(JhError) as e:
        ctx.check_set_full(cols, time)
    assert e.value.code == code


def test_sf_refusals(ctx):
    """An :add of nil and a span of 2^31 values (refused after the first scan,
    before the LUT is allocated): JH_EUNSUPPORTED. An :ok :read whose process
    has no read invocation before it (k_sf_inv finds an add, or no row), and
    reads with elements but no aux array: JH_EINVAL. After each refusal the
    context answers an ordinary case."""
    op = C.op
    adds = [op(0, "invoke", "add", 1), op(0, "ok", "add", 1)]
    read = [op(1, "invoke", "read", None), op(1, "ok", "read", [1])]

    def stamped(rows):
        return C.stamp(rows, [i * C.MS for i in range(len(rows))])

    def ordinary():
        device_same(ctx, "boundary", C.boundary_case())

    _raises(ctx, A.JH_EUNSUPPORTED, stamped(adds + [op(2, "invoke", "add", None), op(2, "ok", "add", None)] + read))
    ordinary()
    _raises(ctx, A.JH_EUNSUPPORTED, stamped([op(0, "invoke", "add", 0), op(0, "ok", "add", 0),
                                            op(0, "invoke", "add", (1 << 31) - 1)] + read))
    ordinary()
    _raises(ctx, A.JH_EINVAL, stamped(adds + [op(1, "ok", "read", [1])]))
    ordinary()
    _raises(ctx, A.JH_EINVAL, stamped([op(1, "invoke", "add", 1), op(1, "ok", "read", [1])]))
    ordinary()
    cols, time = C.encode(stamped(adds + read))
    cols.aux = None
    _raises(ctx, A.JH_EINVAL, cols=cols, time=time)
    ordinary()
