"""jepsen.tests.long-fork/checker on the device (jh_check_long_fork,
jh_longfork.hip) against the CPU restatements of tests/long_fork_ref.py: the
raw result and the fork pairs of the C entry point against the numpy
restatement, and whole result maps through long_fork.checker against the brute
force. Every case runs on both forced paths; everything is integer, so every
comparison is exact."""
import json
import os

import numpy as np
import pytest

from conftest import GOLD
from jepsen_amd import _abi as A
from jepsen_amd import _native, checker, synth
from jepsen_amd import long_fork as L
from jepsen_amd.history import Columns
from long_fork_cases import CASES, HOST_ONLY, RAISING
from long_fork_ref import RAW_FIELDS, Illegal, ref_cols, ref_ops, strip

pytestmark = pytest.mark.gpu

NIL = A.NIL
I64_MAX = (1 << 63) - 1
PATHS = (A.LF_PATH_DENSE, A.LF_PATH_SPARSE)
POISON = (12345, 7)              # the pair between the reads' ranges: a key of another group, a value


def build(n, items, order=None, gap=0):
    """Columns from row items: ("r", g, mask[, value]) an :ok read of group g
    (keys g*n .. g*n+n-1, named in an order that changes from read to read)
    that saw the keys of `mask`; ("R", keys, values) an :ok read as given;
    ("w", key) an :invoke write; ("i",) an :invoke read; ("x",) a nemesis row.
    order: the reads' ranges lie in aux in this order of reads, `gap` poisoned
    pairs before each."""
    reads = []
    for it in items:
        if it[0] == "r":
            g, mask = it[1], it[2]
            v = it[3] if len(it) > 3 else 1
            bits = list(range(n))
            k = len(reads) % n
            bits = bits[k:] + bits[:k] if len(reads) % 2 else bits[::-1]
            reads.append(([g * n + b for b in bits], [v if (mask >> b) & 1 else NIL for b in bits]))
        elif it[0] == "R":
            reads.append((list(it[1]), list(it[2])))
    K = len(reads)
    order = list(range(K)) if order is None else list(order)
    pos, aux = [0] * K, []
    for r in order:
        aux += list(POISON) * gap
        pos[r] = len(aux) // 2
        for k, v in zip(*reads[r]):
            aux += [k, v]
    N = len(items)
    proc, typ, f = np.zeros(N, np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)
    val, val2 = np.full(N, NIL, np.int64), np.full(N, NIL, np.int64)
    j = 0
    for i, it in enumerate(items):
        proc[i] = i % 5
        if it[0] in ("r", "R"):
            typ[i], f[i], val[i], val2[i] = A.TYPE_OK, A.F_READ, pos[j], len(reads[j][0])
            j += 1
        elif it[0] == "w":
            typ[i], f[i], val[i], val2[i] = A.TYPE_INVOKE, A.F_WRITE, it[1], 1
        elif it[0] == "i":
            typ[i], f[i], val2[i] = A.TYPE_INVOKE, A.F_READ, 0
        else:
            proc[i], typ[i], f[i] = -1, A.TYPE_INFO, 16
    return Columns(n=N, process=proc, type=typ, f=f, key=np.full(N, -1, np.int64), value=val, value2=val2,
                   n_keys=0, aux=np.asarray(aux, np.int64).reshape(-1), f_names=["start"])


def agree(ctx, cols, n, paths=PATHS, want=None, maps=True):
    """The raw call on every path against ref_cols: every field and every fork
    pair; then the checker's map against the brute force. Returns ref_cols'
    map."""
    want = ref_cols(cols, n) if want is None else want
    assert want["rc"] == A.JH_OK
    for path in paths:
        r = ctx.check_long_fork(cols, n, path, fork_cap=max(want["fork_count"], 1))
        assert {k: r[k] for k in RAW_FIELDS} == {k: want[k] for k in RAW_FIELDS}, path
        assert r["forks"].tolist() == want["forks"].tolist(), path
        ended_early = want["cause"] == A.CAUSE_MULTIPLE_WRITES or want["illegal_kind"] == 1 or want["reads_count"] == 0
        assert r["path"] == (0 if ended_early else path)
    if maps:
        ops = L.decode(cols)
        try:
            by_ops = ref_ops(n, ops)
        except Illegal as e:
            for path in paths:
                with pytest.raises(L.IllegalHistory) as ei:
                    L.checker(n, path).check({}, cols, {})
                assert ei.value.row == want["illegal_row"] and e.kind == want["illegal_kind"]
        else:
            for path in paths:
                assert strip(L.checker(n, path).check({}, cols, {})) == by_ops, path
    return want


@pytest.mark.parametrize("name", list(CASES))
def test_hand_written_cases(ctx, name):
    n, h, want = CASES[name]
    for path in (A.LF_PATH_AUTO,) + PATHS:
        assert strip(L.checker(n, path).check({}, h, {})) == want          # HOST_ONLY: through the fallback
    if name not in HOST_ONLY:
        agree(ctx, L.encode(h), n)
    else:
        with pytest.raises(_native.JhError) as e:
            ctx.check_long_fork(L.encode(h), n)
        assert e.value.code == A.JH_EUNSUPPORTED


@pytest.mark.parametrize("name", list(RAISING))
def test_raising_cases(ctx, name):
    n, h, kind, row = RAISING[name]
    for path in PATHS:
        with pytest.raises(L.IllegalHistory) as e:
            L.checker(n, path).check({}, h, {})
        assert (e.value.type, e.value.row) == ("illegal-history", row)
        assert ("exactly 2 keys" in e.value.msg) == (kind == 1) and ("distinct values" in e.value.msg) == (kind == 2)
    want = agree(ctx, L.encode(h), n, maps=False)
    assert (want["illegal_kind"], want["illegal_row"]) == (kind, row)
    r = checker.check_safe(L.checker(n), {}, h, {})
    assert r["valid?"] == "unknown" and "IllegalHistory" in r["error"]


def test_golden_map(ctx):
    g = json.load(open(os.path.join(GOLD, "long_fork.json")))
    for path in (A.LF_PATH_AUTO,) + PATHS:
        got = L.checker(g["n"], path).check({}, g["history"], {})
        for pair in got["forks"]:
            for op in pair:
                op.pop("index")
        assert got == g["expected"]


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64])
def test_group_sizes(ctx, n):
    """Mask bit n - 1 (bit 63), the full mask, and a synthetic workload."""
    full, top = (1 << n) - 1, 1 << (n - 1)
    items = [("w", 5 * n), ("r", 5, 0), ("i",), ("r", 5, top), ("r", -2, full), ("r", 5, full), ("x",), ("r", 5, top),
             ("r", -2, top | 1), ("r", 5, 1), ("r", -2, full >> 1), ("r", 7, 0)]
    want = agree(ctx, build(n, items), n)
    # n = 1: one key, nothing to fork; n = 2: top | 1 is the full mask
    assert want["fork_count"] == (0 if n == 1 else 2 if n == 2 else 3)
    # n = 1: every mask is 0 or full (full >> 1 is 0)
    assert want["late_count"] == (6 if n == 1 else 3 if n == 2 else 2) and want["early_count"] == (3 if n == 1 else 2)
    cols = synth.long_fork_history(300, n=n, forks=0 if n == 1 else 2, seed=n, sparse=n == 3)
    assert agree(ctx, cols, n)["fork_count"] == (0 if n == 1 else 2)


def test_empty_histories(ctx):
    none = build(2, [])
    for path in (0,) + PATHS:
        r = ctx.check_long_fork(none, 2, path)
        assert (r["valid"], r["reads_count"], r["fork_count"], r["multiple_row"], r["illegal_row"], r["path"]) == \
            (A.VALID, 0, 0, -1, -1, 0) and r["multiple_key"] == NIL
    agree(ctx, build(2, [("x",), ("i",), ("x",)]), 2)                            # no read, no write
    assert agree(ctx, build(2, [("w", 3), ("x",), ("w", 4), ("w", -3)]), 2)["valid"] == A.VALID    # only writes
    assert agree(ctx, build(2, [("w", 3), ("w", 4), ("w", 3)]), 2)["multiple_row"] == 2
    assert agree(ctx, build(2, [("w", 3)]), 2)["valid"] == A.VALID


@pytest.mark.parametrize("k", [1, 63, 64, 65])
def test_read_counts(ctx, k):
    """k reads and nothing else; then k reads of one valid group and a fork at its end."""
    masks = [0b000, 0b010, 0b011, 0b111]
    want = agree(ctx, build(3, [("r", i % 4, masks[(i // 4) % 4]) for i in range(k)]), 3)
    assert (want["reads_count"], want["fork_count"]) == (k, 0)
    want = agree(ctx, build(3, [("r", 9, masks[(4 * i) // k]) for i in range(k)] + [("r", 9, 0b100)]), 3)
    assert want["fork_count"] == sum(1 for i in range(k) if masks[(4 * i) // k] in (0b010, 0b011))


def tile_edge_items(N):
    """N rows with a group whose reads straddle the first tile edge and a write
    on each side of it."""
    items = [("x",) if i % 3 else ("i",) for i in range(N)]
    for i, m in zip(range(A.LF_TILE - 3, A.LF_TILE + 3), (0b01, 0b10, 0b11, 0b01, 0b10, 0b00)):
        if i < N:
            items[i] = ("r", 4, m)
    items[0], items[1] = ("r", 4, 0b11), ("w", 8)
    if N > A.LF_TILE + 5:
        items[A.LF_TILE + 4] = ("w", 9)
        items[N - 1] = ("r", 4, 0b01)
    return items


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_tile_edges(ctx, d):
    """LF_TILE - 1, LF_TILE and LF_TILE + 1 rows (then two tiles more), with a
    group whose reads straddle the tile edge and a write on each side."""
    for extra in (0, 2 * A.LF_TILE):
        items = tile_edge_items(A.LF_TILE + d + extra)
        want = agree(ctx, build(2, items), 2, maps=extra == 0)
        ms = [it[2] for it in items if it[0] == "r"]
        assert want["fork_groups"] == 1 and want["fork_count"] == ms.count(0b01) * ms.count(0b10) >= 1


@pytest.mark.parametrize("shift", [0, 1])
def test_device_columns(ctx, shift):
    """The history of test_tile_edges' d = 1 in device memory, its columns
    16-byte aligned (shift 0) and 8-byte aligned only (shift 1: the flag and
    compact kernels load the rows of a pair one by one): every field and every
    fork pair equal the host-column call's."""
    from hipcols import DevCols
    cols = build(2, tile_edge_items(A.LF_TILE + 1))
    want = agree(ctx, cols, 2, maps=False)
    assert want["fork_count"] >= 1
    d = DevCols(cols, shift)
    for path in (A.LF_PATH_AUTO,) + PATHS:
        host = ctx.check_long_fork(cols, 2, path, fork_cap=want["fork_count"])
        dev = ctx.check_long_fork(d, 2, path, fork_cap=want["fork_count"], on_device=True)
        assert set(dev) == set(host)
        for k, v in host.items():
            if k == "forks":
                assert dev[k].tolist() == v.tolist() == want["forks"].tolist(), path
            elif k != "device_ms":
                assert dev[k] == v, (k, path)


def test_scattered_ranges(ctx):
    """The reads' ranges reversed and shuffled in aux, with poisoned pairs
    between them: nothing outside a range is read."""
    rng = np.random.default_rng(5)
    masks = [0b0000, 0b0001, 0b0011, 0b0111, 0b1111, 0b1000]
    items = []
    for i in range(150):
        items += [("i",), ("r", int(rng.integers(-3, 4)), masks[int(rng.integers(0, 6))])]
    plain = agree(ctx, build(4, items), 4)
    assert plain["fork_count"] > 0
    for order, gap in ((range(149, -1, -1), 0), (rng.permutation(150), 3), (range(150), 1)):
        want = agree(ctx, build(4, items, order=order, gap=gap), 4, maps=False)
        assert all(np.array_equal(want[k], plain[k]) for k in RAW_FIELDS + ("forks",))


@pytest.mark.parametrize("s", [2, 64, 65, 130])
def test_one_flagged_group(ctx, s):
    """One group of s suspects among valid groups: a wave's partner loop ends
    inside its first step (s <= 64) or runs more than once."""
    masks = [0b01, 0b10, 0b11, 0b00, 0b10]
    items = [("r", 1, 0b01), ("r", 3, 0b11)]
    for i in range(s):
        items += [("r", 2, masks[i % 5 if s > 2 else i]), ("r", 1 + 2 * (i % 2), 0b11)]
    want = agree(ctx, build(2, items), 2, maps=s <= 65)
    a, b = sum(1 for i in range(s) if masks[i % 5 if s > 2 else i] == 0b01), \
        sum(1 for i in range(s) if masks[i % 5 if s > 2 else i] == 0b10)
    assert (want["fork_groups"], want["fork_count"]) == (1, a * b)
    # the truncated prefixes: fork_count stays exact
    fc = want["fork_count"]
    for path in PATHS:
        for cap in sorted({0, 1, fc - 1, fc}):
            r = ctx.check_long_fork(build(2, items), 2, path, fork_cap=cap)
            assert (r["fork_count"], r["fork_groups"], r["valid"]) == (fc, 1, A.INVALID)
            assert r["forks"].tolist() == want["forks"][:cap].tolist()


def test_two_flagged_groups(ctx):
    """Two broken groups separated by valid ones; the forks' reads are the
    first and the last read of the history. The higher group comes first in
    the history and second in the answer."""
    items = [("r", 6, 0b001), ("w", 1), ("r", 0, 0b111), ("r", 3, 0b011), ("r", 6, 0b011), ("r", -4, 0b100),
             ("r", 3, 0b001), ("r", -4, 0b110), ("x",), ("r", 6, 0b111), ("r", -4, 0b010), ("r", 0, 0b000),
             ("r", -4, 0b100), ("r", 6, 0b110)]
    want = agree(ctx, build(3, items), 3)
    assert want["forks"].tolist() == [[5, 10], [10, 12], [0, 13], [4, 13]] and want["fork_groups"] == 2
    for path in PATHS:
        for cap in (0, 1, 2, 3, 4, 50):
            r = ctx.check_long_fork(build(3, items), 3, path, fork_cap=cap)
            assert r["fork_count"] == 4 and r["forks"].tolist() == want["forks"][:cap].tolist()


def test_many_forks_through_the_checker(ctx, monkeypatch):
    """fork_count above the first call's cap: the mirror calls again."""
    monkeypatch.setattr(L, "FORK_CAP", 4)
    items = [("r", 2, 0b01 if i % 2 else 0b10) for i in range(12)]
    cols = build(2, items)
    got = strip(L.checker(2).check({}, cols, {}))
    assert len(got["forks"]) == 36 and got == ref_ops(2, L.decode(cols))
    monkeypatch.setattr(L, "FORK_LIMIT", 10)
    got = strip(L.checker(2).check({}, cols, {}))
    assert got["fork-count"] == 36 and got["forks"] == ref_ops(2, L.decode(cols))["forks"][:10]


@pytest.mark.parametrize("where", ["first", "last"])
def test_repeated_write_by_tile(ctx, where):
    N = 3 * A.LF_TILE + 7
    items = [("w", 1000 + i) if i % 4 == 0 else ("x",) for i in range(N)]
    items[5] = ("r", 0, 0b1)                       # a read of the wrong size for n = 2 below: hidden by the error
    at = (9, 13) if where == "first" else (N - 6, N - 2)
    items[at[0]], items[at[1]] = ("w", -77), ("w", -77)
    want = agree(ctx, build(1, items), 2, maps=False)
    assert (want["multiple_key"], want["multiple_row"], want["cause"]) == (-77, at[1], A.CAUSE_MULTIPLE_WRITES)
    if where == "last":                            # an earlier pair of another key wins
        items[2 * A.LF_TILE + 1], items[2 * A.LF_TILE + 3] = ("w", 1004), ("w", 1 << 40)
        want = agree(ctx, build(1, items), 2, paths=(A.LF_PATH_SPARSE,), maps=False)
        assert (want["multiple_key"], want["multiple_row"]) == (1004, 2 * A.LF_TILE + 1)


def test_extreme_keys(ctx):
    """Groups and written keys next to INT64_MIN and INT64_MAX in one history:
    the differences to the minimum are unsigned. The dense tables cannot span
    them (JH_EINVAL); auto mode takes the sparse path."""
    for n in (2, 64):
        lo, hi = -(1 << 63) // n + 1, I64_MAX // n
        items = [("w", I64_MAX), ("r", hi, 1), ("r", lo, 1 << (n - 1)), ("w", -I64_MAX), ("r", 0, 3), ("r", hi, 2),
                 ("r", lo, 3), ("r", lo, 1 << (n - 1) | 1), ("r", hi, 3), ("w", 0)]
        cols = build(n, items)
        want = agree(ctx, cols, n, paths=(A.LF_PATH_SPARSE,))
        assert want["forks"].tolist() == ([[1, 5]] if n == 2 else [[2, 6], [6, 7], [1, 5]])
        assert ctx.check_long_fork(cols, n, A.LF_PATH_AUTO, 8)["path"] == A.LF_PATH_SPARSE
        with pytest.raises(_native.JhError) as e:
            ctx.check_long_fork(cols, n, A.LF_PATH_DENSE)
        assert e.value.code == A.JH_EINVAL
        items[9] = ("w", I64_MAX)
        want = agree(ctx, build(n, items), n, paths=(A.LF_PATH_SPARSE,))
        assert (want["multiple_key"], want["multiple_row"]) == (I64_MAX, 9)


def test_invalid_and_unsupported(ctx):
    def code(cols, n, path=0):
        with pytest.raises(_native.JhError) as e:
            ctx.check_long_fork(cols, n, path)
        return e.value.code

    good = [("r", 1, 0b01), ("r", 1, 0b11), ("w", 2)]
    for n, want in ((0, A.JH_EINVAL), (-3, A.JH_EINVAL), (65, A.JH_EUNSUPPORTED), (1 << 40, A.JH_EUNSUPPORTED)):
        assert code(build(2, good), n) == want
    assert code(build(2, good), 2, path=3) == A.JH_EINVAL
    for edit in (lambda c: c.value.__setitem__(0, 5),                    # 5 + 2 > 4 pairs
                 lambda c: c.value.__setitem__(1, -1), lambda c: c.value2.__setitem__(0, -2),
                 lambda c: c.value2.__setitem__(1, 3),                   # 2 + 3 > 4
                 lambda c: c.value2.__setitem__(1, NIL),
                 lambda c: setattr(c, "aux", c.aux[:-1].copy())):        # an odd n_aux
        cols = build(2, good)
        edit(cols)
        for path in PATHS:
            assert code(cols, 2, path) == A.JH_EINVAL
        assert ref_cols(cols, 2)["rc"] == A.JH_EINVAL
    # a bad range in a row that is not an :ok read is never looked at
    cols = build(2, good)
    cols.value[2], cols.type[0], cols.value[0] = 99, A.TYPE_FAIL, 99
    agree(ctx, cols, 2)
    for bad in ([("R", [2, 4], [1, NIL])], [("R", [3, 4], [1, 1])], [("R", [2, 2], [1, 1])],
                [("R", [0, 1, 3], [1, NIL, 1])], [("R", [-1, 0], [1, 1])]):
        n = len(bad[0][1])
        for path in PATHS:
            assert code(build(n, good[:2] + bad), n, path) == A.JH_EUNSUPPORTED
        assert ref_cols(build(n, good[:2] + bad), n)["rc"] == A.JH_EUNSUPPORTED
        # the duplicate-key and alignment tests apply only to reads of exactly n pairs
        assert agree(ctx, build(n, good[:2] + bad), n + 1, maps=False)["illegal_kind"] == 1


def test_auto_path(ctx):
    dense = synth.long_fork_history(400, n=2, forks=1, seed=3)
    sparse = synth.long_fork_history(400, n=2, forks=1, seed=3, sparse=True)
    for cols, path in ((dense, A.LF_PATH_DENSE), (sparse, A.LF_PATH_SPARSE)):
        want = agree(ctx, cols, 2)
        r = ctx.check_long_fork(cols, 2, A.LF_PATH_AUTO, 4)
        assert r["path"] == path and {k: r[k] for k in RAW_FIELDS} == {k: want[k] for k in RAW_FIELDS}
        assert r["forks"].tolist() == want["forks"].tolist()


@pytest.fixture(scope="module")
def big():
    cols = synth.long_fork_history(100_000, n=3, forks=3, seed=11, n_procs=16)
    return cols, ref_cols(cols, 3)


@pytest.mark.parametrize("path", PATHS)
def test_synth_200k_rows(ctx, big, path):
    cols, want = big
    assert cols.n >= 200_000 and want["fork_count"] == want["fork_groups"] == 3
    agree(ctx, cols, 3, paths=(path,), want=want, maps=False)
    got = L.checker(3, path).check({}, cols, {})
    assert [[a["index"], b["index"]] for a, b in got["forks"]] == want["forks"].tolist()
    assert (got["reads-count"], got["early-read-count"], got["late-read-count"]) == \
        (want["reads_count"], want["early_count"], want["late_count"])
