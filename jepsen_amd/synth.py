"""Seeded synthetic histories from libjhgen.so.

Workload generator for bench.py and the tests: the histories are shaped like
the reference workloads (see csrc/gen.cpp header) and are returned as
`history.Columns` (host numpy int64 columns in the include/jh.h layout).
"""
import ctypes as C
import os

import numpy as np

from .history import Columns

JH_NIL = -(1 << 63)

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


class _CasParams(C.Structure):
    _fields_ = [("n_keys", C.c_int64), ("ops_per_key", C.c_int64),
                ("threads_per_key", C.c_int32), ("readers", C.c_int32),
                ("n_values", C.c_int32), ("process_limit", C.c_int32),
                ("groups", C.c_int32), ("init_nil", C.c_int32),
                ("p_info", C.c_double), ("p_invalid", C.c_double),
                ("nemesis_every", C.c_int64), ("seed", C.c_uint64),
                ("keyed", C.c_int32), ("pad", C.c_int32)]


class _CounterParams(C.Structure):
    _fields_ = [("n_ops", C.c_int64), ("n_procs", C.c_int32), ("read_every", C.c_int32),
                ("p_fail", C.c_double), ("p_info", C.c_double),
                ("n_bad_reads", C.c_int64), ("seed", C.c_uint64)]


class _SetParams(C.Structure):
    _fields_ = [("n_adds", C.c_int64), ("n_procs", C.c_int32), ("pad", C.c_int32),
                ("p_fail", C.c_double), ("p_info", C.c_double),
                ("n_lost", C.c_int64), ("n_unexpected", C.c_int64), ("seed", C.c_uint64)]


_p64 = C.POINTER(C.c_int64)


class _Hist(C.Structure):
    _fields_ = [("n", C.c_int64), ("n_aux", C.c_int64), ("n_keys", C.c_int64),
                ("process", _p64), ("type", _p64), ("f", _p64), ("key", _p64),
                ("value", _p64), ("value2", _p64), ("aux", _p64), ("truth", _p64),
                ("impl", C.c_void_p)]


def _load():
    global _lib
    if _lib is None:
        path = os.path.join(_HERE, "libjhgen.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: run __graft_entry__.build()")
        _lib = C.CDLL(path)
        _lib.jhg_cas.argtypes = [C.POINTER(_CasParams), C.POINTER(_Hist)]
        _lib.jhg_cas_par.argtypes = [C.POINTER(_CasParams), C.c_int32, C.POINTER(_Hist)]
        _lib.jhg_counter.argtypes = [C.POINTER(_CounterParams), C.POINTER(_Hist)]
        _lib.jhg_set.argtypes = [C.POINTER(_SetParams), C.POINTER(_Hist)]
        _lib.jhg_free.argtypes = [C.POINTER(_Hist)]
    return _lib


def _take(h, n_truth):
    def arr(p, n):
        if n == 0:
            return np.zeros(0, np.int64)
        return np.ctypeslib.as_array(p, shape=(n,)).copy()
    n = h.n
    cols = Columns(n=n, process=arr(h.process, n), type=arr(h.type, n), f=arr(h.f, n),
                   key=arr(h.key, n), value=arr(h.value, n), value2=arr(h.value2, n),
                   n_keys=h.n_keys,
                   aux=arr(h.aux, h.n_aux) if h.n_aux else np.zeros(1, np.int64))
    cols.keys = list(range(h.n_keys))
    cols.f_names = ["start", "stop"]
    truth = arr(h.truth, n_truth) if n_truth else np.zeros(0, np.int64)
    return cols, truth


def cas_register(n_keys=10000, ops_per_key=500, threads_per_key=10, readers=5,
                 n_values=5, process_limit=20, groups=10, init_nil=True,
                 p_info=0.02, p_invalid=0.01, nemesis_every=10000, seed=3, keyed=True, parts=1):
    """Independent cas-register history (C3 defaults: 10k keys x ~1k entries).

    parts > 1 generates the keys as that many sub-histories on parallel host
    threads and concatenates them (gen.cpp jhg_cas_par; the C4 1M-key history).
    Returns (Columns, injected) where injected[k] = 1 for keys with a
    stale read injected (all other keys are linearizable by construction)."""
    lib = _load()
    p = _CasParams(n_keys, ops_per_key, threads_per_key, readers, n_values, process_limit,
                   groups, 1 if init_nil else 0, p_info, p_invalid, nemesis_every, seed,
                   1 if keyed else 0, 0)
    h = _Hist()
    if parts > 1:
        lib.jhg_cas_par(C.byref(p), parts, C.byref(h))
    else:
        lib.jhg_cas(C.byref(p), C.byref(h))
    try:
        return _take(h, n_keys)
    finally:
        lib.jhg_free(C.byref(h))


def counter(n_ops=1000, n_procs=10, read_every=101, p_fail=0.05, p_info=0.01,
            n_bad_reads=0, seed=2):
    lib = _load()
    p = _CounterParams(n_ops, n_procs, read_every, p_fail, p_info, n_bad_reads, seed)
    h = _Hist()
    lib.jhg_counter(C.byref(p), C.byref(h))
    try:
        return _take(h, 0)[0]
    finally:
        lib.jhg_free(C.byref(h))


def set_history(n_adds=1000, n_procs=10, p_fail=0.05, p_info=0.02, n_lost=0,
                n_unexpected=0, seed=2):
    lib = _load()
    p = _SetParams(n_adds, n_procs, 0, p_fail, p_info, n_lost, n_unexpected, seed)
    h = _Hist()
    lib.jhg_set(C.byref(p), C.byref(h))
    try:
        return _take(h, 0)[0]
    finally:
        lib.jhg_free(C.byref(h))


def set_full_history(n_adds=2000, n_procs=10, n_readers=2, read_every=10, p_fail=0.05,
                     p_info=0.02, n_lost=0, n_stale=0, row_ns=100_000, seed=6):
    """A (checker/set-full) workload (checker.clj:236-534; the shape of
    yugabyte/src/yugabyte/set.clj:92 and tidb/src/tidb/sets.clj:53): adds of
    distinct integers 0..n_adds-1 by `n_procs` processes, `n_readers`
    processes reading the WHOLE set every `read_every` rounds of adds.

    A round invokes one add per process and completes them in random order;
    a read invoked before a round completes after it. :ok adds are visible
    from their completion on, adds concurrent with a read are seen with
    probability 1/2, :info adds apply with probability 1/2 (and rename the
    process, core.clj:349), :fail adds never apply. Faults: `n_lost`
    acknowledged elements vanish from every read after the middle of the
    history (lost), `n_stale` elements are missed by the first read invoked
    after their :ok (stale, stable latency > 0). :time = row * row_ns.

    Returns (Columns, time) with the set reads' elements in `aux` (CSR)."""
    rng = np.random.default_rng(seed)
    P, RD = n_procs, n_readers
    rows_p, rows_t, rows_f, rows_v, rows_v2 = [], [], [], [], []
    aux_parts, aux_len = [], 0
    applied = np.zeros(n_adds, bool)          # visible from completion on
    acked_row = np.full(n_adds, -1, np.int64)
    proc_id = list(range(P))
    next_proc = P + RD
    n_rounds = (n_adds + P - 1) // P
    lost = rng.choice(n_adds, size=n_lost, replace=False) if n_lost else np.zeros(0, np.int64)
    stale = set(rng.choice(n_adds, size=n_stale, replace=False).tolist()) if n_stale else set()
    stale_pending = []
    reader = 0
    mid_round = n_rounds // 2

    def emit(p, t, f, v=JH_NIL, v2=JH_NIL):
        rows_p.append(p); rows_t.append(t); rows_f.append(f); rows_v.append(v); rows_v2.append(v2)

    for k in range(n_rounds):
        els = list(range(k * P, min(n_adds, (k + 1) * P)))
        rd = (k % read_every) == read_every - 1
        if rd:
            rp = P + (reader % RD)
            reader += 1
            emit(rp, 0, 0)                     # :invoke :read
            hide, stale_pending = stale_pending, []   # acked before this read's invocation
        for j, e in enumerate(els):
            emit(proc_id[j], 0, 3, e)          # :invoke :add e
        outcome = rng.random(len(els))
        seen_conc = rng.random(len(els)) < 0.5
        for j in rng.permutation(len(els)):
            e = els[j]
            if outcome[j] < p_fail:
                emit(proc_id[j], 2, 3, e)
            elif outcome[j] < p_fail + p_info:
                emit(proc_id[j], 3, 3, e)
                applied[e] = rng.random() < 0.5
                proc_id[j] = next_proc
                next_proc += 1
            else:
                applied[e] = True
                acked_row[e] = len(rows_p)
                emit(proc_id[j], 1, 3, e)
                if e in stale:
                    stale_pending.append(e)
        if rd:
            vis = applied.copy()
            conc = np.asarray(els, np.int64)
            vis[conc] = applied[conc] & seen_conc
            if k >= mid_round and n_lost:
                vis[lost] = False
            for e in hide:
                vis[e] = False
            elems = np.flatnonzero(vis).astype(np.int64)
            emit(rp, 1, 0, aux_len, len(elems))
            aux_parts.append(elems)
            aux_len += len(elems)
    n = len(rows_p)
    cols = Columns(n=n, process=np.asarray(rows_p, np.int64), type=np.asarray(rows_t, np.int64),
                   f=np.asarray(rows_f, np.int64), key=np.full(n, -1, np.int64),
                   value=np.asarray(rows_v, np.int64), value2=np.asarray(rows_v2, np.int64),
                   n_keys=0, aux=np.concatenate(aux_parts) if aux_parts else np.zeros(1, np.int64))
    time = np.arange(n, dtype=np.int64) * row_ns
    return cols, time


def columns_to_ops(cols, time):
    """Op maps (jepsen_amd.history form) of a set-full Columns history, for the
    pure-Python oracle and the checker mirror."""
    names = {0: "invoke", 1: "ok", 2: "fail", 3: "info"}
    fnames = {0: "read", 3: "add"}
    ops = []
    for i in range(cols.n):
        t, f = int(cols.type[i]), int(cols.f[i])
        if f == 0 and t == 1:
            o, c = int(cols.value[i]), int(cols.value2[i])
            v = cols.aux[o:o + c].tolist()
        elif f == 0:
            v = None
        else:
            v = int(cols.value[i])
        ops.append({"process": int(cols.process[i]), "type": names[t], "f": fnames[f],
                    "value": v, "index": i, "time": int(time[i])})
    return ops


def queue_history(n_enqueues=2000, n_procs=5, p_fail=0.05, p_info=0.05, n_lost=0, n_unexpected=0,
                  n_duplicated=0, n_repeat=0, drain_parts=2, seed=7):
    """A queue workload for (checker/total-queue) and (checker/queue
    (model/unordered-queue)) (checker.clj:160-180, 536-628; the shape of
    disque.clj:305-309 and rabbitmq_test.clj:56-59): `n_procs` enqueuers, one
    dequeuer taking a random pending element after every round, and a final
    drain in `drain_parts` :drain ops. Values are consecutive integers (as
    gen/queue, generator.clj:405-416) except `n_repeat` values enqueued twice. :fail enqueues never apply, :info ones
    apply with probability 1/2. Faults: `n_lost` acknowledged elements are
    never dequeued, `n_unexpected` never-enqueued values are dequeued,
    `n_duplicated` elements are dequeued twice. Returns Columns (drain
    elements in aux)."""
    rng = np.random.default_rng(seed)
    P = n_procs
    DQ = P                                  # dequeuer process
    # consecutive integers, as gen/queue enqueues them (generator.clj:405-416)
    vals = np.arange(n_enqueues, dtype=np.int64)
    if n_repeat:
        vals[-n_repeat:] = vals[:n_repeat]
    rows = []
    aux = []
    pending = []                            # applied, not yet dequeued
    lost_left = n_lost
    proc_id = list(range(P))
    next_proc = P + 1
    dup_left = n_duplicated
    dequeued = []
    for k in range(0, n_enqueues, P):
        els = vals[k:k + P]
        for j, v in enumerate(els):
            rows.append((proc_id[j], 0, 4, int(v), JH_NIL))
        for j in rng.permutation(len(els)):
            v = int(els[j])
            u = rng.random()
            if u < p_fail:
                rows.append((proc_id[j], 2, 4, v, JH_NIL))
            elif u < p_fail + p_info:
                rows.append((proc_id[j], 3, 4, v, JH_NIL))
                proc_id[j] = next_proc
                next_proc += 1
                if rng.random() < 0.5:
                    pending.append(v)
            else:
                rows.append((proc_id[j], 1, 4, v, JH_NIL))
                if lost_left and rng.random() < 0.3:
                    lost_left -= 1          # acknowledged, then lost
                else:
                    pending.append(v)
        if pending:
            i = int(rng.integers(len(pending)))
            v = pending.pop(i)
            rows.append((DQ, 0, 5, JH_NIL, JH_NIL))
            rows.append((DQ, 1, 5, v, JH_NIL))
            dequeued.append(v)
            if dup_left and rng.random() < 0.2:
                dup_left -= 1
                rows.append((DQ, 0, 5, JH_NIL, JH_NIL))
                rows.append((DQ, 1, 5, v, JH_NIL))
    rest = pending + [int(x) for x in dequeued[:dup_left]]
    rest += [int(n_enqueues + 100 + i) for i in range(n_unexpected)]
    rng.shuffle(rest)
    parts = np.array_split(np.asarray(rest, np.int64), max(drain_parts, 1))
    for part in parts:
        rows.append((DQ, 0, 6, JH_NIL, JH_NIL))
        rows.append((DQ, 1, 6, len(aux), len(part)))
        aux.extend(part.tolist())
    a = np.asarray(rows, np.int64).reshape(-1, 5)
    n = len(a)
    return Columns(n=n, process=a[:, 0].copy(), type=a[:, 1].copy(), f=a[:, 2].copy(),
                   key=np.full(n, -1, np.int64), value=a[:, 3].copy(), value2=a[:, 4].copy(),
                   n_keys=0, aux=np.asarray(aux, np.int64) if aux else np.zeros(1, np.int64))


def queue_columns_to_ops(cols):
    """Op maps of a queue_history (for the oracles and the checker mirror)."""
    names = {0: "invoke", 1: "ok", 2: "fail", 3: "info"}
    fnames = {4: "enqueue", 5: "dequeue", 6: "drain"}
    ops = []
    for i in range(cols.n):
        t, f = int(cols.type[i]), int(cols.f[i])
        v = int(cols.value[i])
        if f == 6 and t == 1:
            val = cols.aux[v:v + int(cols.value2[i])].tolist()
        else:
            val = None if v == JH_NIL else v
        ops.append({"process": int(cols.process[i]), "type": names[t], "f": fnames[f], "value": val})
    return ops


UID_F_NAMES = ["generate", "start", "stop"]     # interned f codes 16, 17, 18 of a unique_ids_history


def unique_ids_history(n_ops=1000, n_procs=8, p_fail=0.05, p_info=0.02, kind="counter", dups=(), nil_acks=0,
                       noise=True, seed=0):
    """An id-generator workload for (checker/unique-ids) (checker.clj:631-676;
    the shape of hazelcast.clj's id-gen workloads): rounds of `n_procs`
    :invoke :generate ops completed in a random order -- :ok with the id,
    :fail with probability p_fail, :info with p_info (the process is then
    replaced). kind: "counter" consecutive ids from a random negative start,
    "flake" distinct random 63-bit ids, "string" the counter ids as strings
    (the values are then interned, values_interned). dups: (how_many_ids,
    occurrences) pairs -- that many acknowledged ids are each acknowledged
    `occurrences` times in all. nil_acks: acks whose id is nil. noise: every
    round ends with an :ok :read whose value is an acknowledged id, or (every
    16th) a nemesis :info :start / :stop pair, and the :fail / :info
    completions carry the id of the op before them: none of it may count.
    Vectorised (100 M rows in seconds). Returns Columns."""
    rng = np.random.default_rng(seed)
    P = int(n_procs)
    R = (n_ops + P - 1) // P                    # rounds
    N = R * P
    j = np.arange(N, dtype=np.int64)
    if kind == "flake":
        ids = (rng.integers(0, 1 << 31, N, dtype=np.int64) << 32) | rng.permutation(N).astype(np.int64)
    elif kind in ("counter", "string"):
        ids = int(rng.integers(-(1 << 40), -(1 << 20))) + j
    else:
        raise ValueError(f"unknown kind {kind!r}")
    u = rng.random(N)
    ctype = np.where(u < p_fail, 2, np.where(u < p_fail + p_info, 3, 1)).astype(np.int64)
    live = j < n_ops
    ok_ops = np.nonzero((ctype == 1) & live)[0]
    need = sum(int(h) * int(o) for h, o in dups) + int(nil_acks)
    if need > len(ok_ops):
        raise ValueError("not enough acknowledged ops for the requested dups / nil acks")
    pick = rng.permutation(ok_ops)[:need]
    acked = ids.copy()
    at = 0
    for h, o in dups:
        grp = pick[at:at + int(h) * int(o)].reshape(int(h), int(o))
        acked[grp[:, 1:]] = acked[grp[:, :1]]
        at += int(h) * int(o)
    acked[pick[at:]] = JH_NIL
    cval = np.where(ctype == 1, acked, np.roll(ids, 1) if noise else JH_NIL)
    # rows of a round: P invokes, P completions in a random order, 2 noise rows
    W = 2 * P + (2 if noise else 0)
    proc = np.full((R, W), -1, np.int64)
    typ = np.zeros((R, W), np.int64)
    fc = np.full((R, W), 16, np.int64)
    val = np.full((R, W), JH_NIL, np.int64)
    keep = np.ones((R, W), bool)
    info = (ctype == 3).reshape(R, P)
    crashes = np.cumsum(info, axis=0) - info            # crashes of the slot before this round
    p_of = np.arange(P, dtype=np.int64)[None, :] + (P + 1) * crashes
    perm = np.argsort(rng.random((R, P)), axis=1)       # completion order of the round
    rr = np.arange(R)[:, None]
    proc[:, :P] = p_of
    keep[:, :P] = live.reshape(R, P)
    proc[:, P:2 * P] = p_of[rr, perm]
    typ[:, P:2 * P] = ctype.reshape(R, P)[rr, perm]
    val[:, P:2 * P] = cval.reshape(R, P)[rr, perm]
    keep[:, P:2 * P] = live.reshape(R, P)[rr, perm]
    if noise:
        nem = (np.arange(R) % 16) == 15
        some = ids.reshape(R, P)[np.arange(R), rng.integers(0, P, R)]
        proc[:, 2 * P:] = np.where(nem, -1, P)[:, None]
        typ[:, 2 * P] = np.where(nem, 3, 0)
        typ[:, 2 * P + 1] = np.where(nem, 3, 1)
        fc[:, 2 * P] = np.where(nem, 17, 0)
        fc[:, 2 * P + 1] = np.where(nem, 18, 0)
        val[:, 2 * P + 1] = np.where(nem, JH_NIL, some)
    k = keep.reshape(-1)
    n = int(k.sum())
    cols = Columns(n=n, process=proc.reshape(-1)[k], type=typ.reshape(-1)[k], f=fc.reshape(-1)[k],
                   key=np.full(n, -1, np.int64), value=val.reshape(-1)[k], value2=np.full(n, JH_NIL, np.int64),
                   n_keys=0, aux=np.zeros(1, np.int64), f_names=list(UID_F_NAMES))
    if kind == "string":
        from . import history as H
        ops = unique_ids_columns_to_ops(cols)
        for op in ops:
            if op["process"] == "nemesis":
                op["value"] = "partition-" + op["f"]
            elif op["value"] is not None:
                op["value"] = "id%+d" % op["value"]
        cols = H.encode(ops, keyed=False)
    return cols


def unique_ids_columns_to_ops(cols):
    """Op maps of a unique_ids_history (for the restatements and the checker
    mirror); interned values come back from the value table."""
    names = {0: "invoke", 1: "ok", 2: "fail", 3: "info"}
    ops = []
    for i in range(cols.n):
        f, v, p = int(cols.f[i]), int(cols.value[i]), int(cols.process[i])
        if v == JH_NIL:
            v = None
        elif cols.values_interned:
            v = cols.value_table[v]
        ops.append({"process": p if p >= 0 else "nemesis", "type": names[int(cols.type[i])],
                    "f": "read" if f == 0 else cols.f_names[f - 16], "value": v})
    return ops


BANK_F_NAMES = ["transfer", "start", "stop"]    # interned f codes 16, 17, 18 of a bank_history


def bank_history(n_ops=1000, n_accounts=8, n_procs=8, total=100, p_read=0.5, read_sizes=None, p_info=0.02,
                 unexpected=(), nils=(), wrong=(), negative=(), nil_values=(), noise=True, seed=0):
    """A bank workload for jepsen.tests.bank/checker (tests/bank.clj): `n_ops`
    ops of `n_procs` processes, each an invocation row and a completion row;
    an op is a :read with probability p_read, else a :transfer. Reads complete
    :ok (an :info with probability p_info: not a read the checker sees), and
    an :ok :read carries {account balance} over `size` accounts summing to
    `total`, all balances >= 0; size is n_accounts, or drawn from the list
    read_sizes (each <= n_accounts; a size of 0 is the empty map). The pairs
    lie in aux in read order (include/jh.h "Bank reads"). noise: every 64th op
    is a nemesis :info :start / :stop pair instead.

    Errors are planted at chosen reads (indices among the :ok :reads, in
    history order): unexpected -- 1 to 3 keys become codes >= n_accounts;
    nils -- 1 or 2 balances become nil; wrong -- one balance moves, so the
    total is off by a small amount that differs from read to read; negative --
    an amount above `total` moves between two balances (size >= 2), the sum
    stays; nil_values -- the read's :value is nil. Indices past the last read
    are ignored. Vectorised numpy (100 M rows in seconds). Returns Columns;
    value_table is the account table (0..n_accounts-1, then "x0".."x2")."""
    rng = np.random.default_rng(seed)
    N = int(n_ops)
    i = np.arange(N, dtype=np.int64)
    nem = ((i % 64) == 63) if noise else np.zeros(N, bool)
    is_rd = (rng.random(N) < p_read) & ~nem
    info = rng.random(N) < p_info
    proc = np.where(nem, -1, i % int(n_procs))
    typ = np.zeros((N, 2), np.int64)
    typ[:, 1] = np.where(nem | info, 3, 1)
    typ[:, 0] = np.where(nem, 3, 0)
    fc = np.empty((N, 2), np.int64)
    fc[:, 0] = np.where(nem, 17, np.where(is_rd, 0, 16))
    fc[:, 1] = np.where(nem, 18, fc[:, 0])
    ok_read = is_rd & ~info
    K = int(ok_read.sum())
    if read_sizes is None:
        size = np.full(K, int(n_accounts), np.int64)
    else:
        sz = np.asarray(read_sizes, np.int64)
        if len(sz) == 0 or sz.min() < 0 or sz.max() > n_accounts:
            raise ValueError("read_sizes: sizes in 0..n_accounts")
        size = sz[rng.integers(0, len(sz), K)]

    def at(xs):
        xs = np.asarray(list(xs), np.int64).reshape(-1)
        return xs[(xs >= 0) & (xs < K)]
    nilv = at(nil_values)
    size[nilv] = 0
    off = np.zeros(K + 1, np.int64)
    np.cumsum(size, out=off[1:])
    E = int(off[K])
    rid = np.repeat(np.arange(K, dtype=np.int64), size)
    j = np.arange(E, dtype=np.int64) - off[rid]
    rot = rng.integers(0, max(int(n_accounts), 1), K)
    code = (rot[rid] + j) % max(int(n_accounts), 1)
    bal = np.floor(rng.random(E) * (total // np.maximum(size[rid], 1) + 1)).astype(np.int64) if total > 0 else np.zeros(E, np.int64)
    bal = np.minimum(bal, max(total, 0) // np.maximum(size[rid], 1))
    c = np.zeros(E + 1, np.int64)
    np.cumsum(bal, out=c[1:])
    some = size > 0
    bal[off[:-1][some]] += total - (c[off[1:]] - c[off[:-1]])[some]
    for t, k in enumerate(at(unexpected)):
        m = min(int(size[k]), 1 + t % 3)
        code[off[k] + (size[k] // 2 + np.arange(m)) % max(int(size[k]), 1)] = n_accounts + np.arange(m)
    for t, k in enumerate(at(nils)):
        m = min(int(size[k]), 1 + t % 2)
        bal[off[k] + (size[k] - 1 - np.arange(m))] = JH_NIL
    for t, k in enumerate(at(wrong)):
        if size[k]:
            bal[off[k] + size[k] // 2] += (1 + (t * 7) % 13) * (1 if t % 2 else -1)
    for t, k in enumerate(at(negative)):
        if size[k] < 2:
            raise ValueError("negative: the read needs two accounts")
        d = bal[off[k]] + total + 1 + t % 5
        bal[off[k]] -= d
        bal[off[k + 1] - 1] += d
    val = np.full((N, 2), JH_NIL, np.int64)
    val2 = np.full((N, 2), JH_NIL, np.int64)
    rows = np.nonzero(ok_read)[0]
    val[rows, 1] = off[:-1]
    val2[rows, 1] = size
    val[rows[nilv], 1] = JH_NIL
    aux = np.empty(2 * E, np.int64)
    aux[0::2] = code
    aux[1::2] = bal
    n = 2 * N
    return Columns(n=n, process=np.repeat(proc, 2), type=typ.reshape(-1), f=fc.reshape(-1),
                   key=np.full(n, -1, np.int64), value=val.reshape(-1), value2=val2.reshape(-1), n_keys=0, aux=aux,
                   f_names=list(BANK_F_NAMES), value_table=list(range(int(n_accounts))) + ["x0", "x1", "x2"])


def bank_columns_to_ops(cols):
    """Op maps (with :index) of a bank history's Columns, for the restatements
    and the checker mirror: a read gets its {account balance} map back through
    the account table, every other row a nil :value."""
    from . import bank
    return bank.decode(cols)


LONG_FORK_F_NAMES = ["start", "stop"]    # interned f codes 16, 17 of a long_fork_history
LONG_FORK_STRIDE = 1_000_003             # sparse=True: group g lies at g * n * LONG_FORK_STRIDE


def long_fork_history(n_ops=1000, n=2, n_procs=5, forks=0, repeat_write=None, sparse=False, p_info=0.02,
                      p_fail=0.02, seed=0, tile=1):
    """A long-fork workload for jepsen.tests.long-fork/checker
    (tests/long_fork.clj), encoded as long_fork.encode does: `n_ops` ops of
    `n_procs` processes, an invocation row and a completion row each,
    interleaved. It follows the reference generator's state machine
    (long_fork.clj:114-156): a process that has just written a key reads that
    key's group; otherwise, with probability 1/2, it reads the group of a key
    some process wrote last; otherwise it writes a fresh key (value 1). A
    write takes effect when it completes (:ok always, :info half of the time,
    :fail never) and an :ok read sees exactly the keys in effect, in shuffled
    key order, so the history has no fork. Completions are :fail / :info with
    probability p_fail / p_info. Every 500th op is a nemesis :info :start /
    :stop pair instead.

    forks: that many forks are planted at even distances, each in a fresh
    group of its own by one extra process: two keys written, then two :ok reads
    that each see one of them (n >= 2). repeat_write: the op number at which
    the extra process writes, once more, the first key written so far.
    sparse: groups lie LONG_FORK_STRIDE groups apart. Groups start seven
    below zero, so keys are negative too. tile: the whole history repeated
    that many times with disjoint keys (bench sizes; forks and the repeated
    write repeat with it). Returns Columns; n_ops * tile ops."""
    import random
    from . import _abi as A
    from .history import Columns
    if forks and n < 2:
        raise ValueError("a fork needs a group of at least 2 keys")
    rng = random.Random(seed)
    proc, typ, fc, val, val2, aux = [], [], [], [], [], []
    mul = LONG_FORK_STRIDE if sparse else 1

    def key(k):
        return (k // n - 7) * n * mul + k % n

    def emit(p, t, f, v=-(1 << 63), v2=-(1 << 63)):
        proc.append(p); typ.append(t); fc.append(f); val.append(v); val2.append(v2)

    def emit_read(p, t, ks=None, seen=()):
        if ks is None:
            emit(p, t, A.F_READ, A.NIL, 0)
            return
        emit(p, t, A.F_READ, len(aux) // 2, len(ks))
        for k in ks:
            aux.extend((key(k), 1 if k in seen else A.NIL))

    def group(k):
        ks = list(range(k - k % n, k - k % n + n))
        rng.shuffle(ks)
        return ks

    state = {"next": 0, "first": None}

    def fresh():
        k = state["next"]
        state["next"] += 1
        if state["first"] is None:
            state["first"] = k
        return k

    extra = n_procs
    plant_at = {(i + 1) * n_ops // (forks + 1) for i in range(forks)}
    workers, pending, applied = {}, {}, set()
    started = 0
    while started < n_ops or pending:
        p = rng.randrange(n_procs)
        if p in pending:
            kind, x = pending.pop(p)
            u = rng.random()
            t = A.TYPE_FAIL if u < p_fail else A.TYPE_INFO if u < p_fail + p_info else A.TYPE_OK
            if kind == "w":
                if t == A.TYPE_OK or (t == A.TYPE_INFO and rng.random() < 0.5):
                    applied.add(x)
                emit(p, t, A.F_WRITE, key(x), 1)
            elif t == A.TYPE_OK:
                emit_read(p, t, x, applied)
            else:
                emit_read(p, t)
            continue
        if started >= n_ops:
            continue
        if started in plant_at:
            plant_at.discard(started)
            state["next"] += -state["next"] % n                  # a group of its own
            ks = [fresh() for _ in range(n)]
            for k in ks[:2]:
                emit(extra, A.TYPE_INVOKE, A.F_WRITE, key(k), 1)
                emit(extra, A.TYPE_OK, A.F_WRITE, key(k), 1)
            for k in ks[:2]:
                emit_read(extra, A.TYPE_INVOKE)
                emit_read(extra, A.TYPE_OK, group(k), {k})
        if repeat_write is not None and started == repeat_write:
            k = fresh() if state["first"] is None else state["first"]
            emit(extra, A.TYPE_INVOKE, A.F_WRITE, key(k), 1)
            emit(extra, A.TYPE_OK, A.F_WRITE, key(k), 1)
            if state["next"] == 1 and k == 0 and len(fc) == 2:     # nothing was written before: write it twice
                emit(extra, A.TYPE_INVOKE, A.F_WRITE, key(k), 1)
                emit(extra, A.TYPE_OK, A.F_WRITE, key(k), 1)
        started += 1
        if started % 500 == 0:
            emit(-1, A.TYPE_INFO, A.F_FIRST_INTERNED + (started // 500) % 2)
            emit(-1, A.TYPE_INFO, A.F_FIRST_INTERNED + (started // 500) % 2)
            continue
        k = workers.get(p)
        if k is not None:
            workers[p] = None
            pending[p] = ("r", group(k))
            emit_read(p, A.TYPE_INVOKE)
            continue
        active = [x for x in workers.values() if x is not None]
        if rng.random() < 0.5 and active:
            pending[p] = ("r", group(rng.choice(active)))
            emit_read(p, A.TYPE_INVOKE)
        else:
            k = fresh()
            workers[p] = k
            pending[p] = ("w", k)
            emit(p, A.TYPE_INVOKE, A.F_WRITE, key(k), 1)
    cols = [np.asarray(c, np.int64) for c in (proc, typ, fc, val, val2)]
    auxa = np.asarray(aux, np.int64)
    if tile > 1:
        span = (state["next"] + n + (-state["next"]) % n) * mul          # keys per copy, a multiple of n
        rows, half = len(proc), len(aux) // 2
        is_w = cols[2] == A.F_WRITE
        is_r = (cols[2] == A.F_READ) & (cols[3] != A.NIL)
        shift = np.repeat(np.arange(tile, dtype=np.int64), rows)
        cols = [np.tile(c, tile) for c in cols]
        cols[3] = cols[3] + np.where(np.tile(is_w, tile), shift * span, 0) + np.where(np.tile(is_r, tile), shift * half, 0)
        auxa = np.tile(auxa, tile)
        auxa[0::2] += np.repeat(np.arange(tile, dtype=np.int64), half) * span
    N = len(cols[0])
    return Columns(n=N, process=cols[0], type=cols[1], f=cols[2], key=np.full(N, -1, np.int64), value=cols[3],
                   value2=cols[4], n_keys=0, aux=auxa, f_names=list(LONG_FORK_F_NAMES))


def long_fork_columns_to_ops(cols):
    """Op maps (with :index) of a long-fork history's Columns, for the
    restatements (jepsen_amd/long_fork.py decode)."""
    from . import long_fork
    return long_fork.decode(cols)


# ---------------------------------------------------------------------------
# causal-reverse ("sequential") workload, jepsen/src/jepsen/tests/causal_reverse.clj:100-111
def _causal_reverse_key(rng, ops, n_procs, p_info, n_viol):
    """One key's rows (process, type, f, value, value2; a read's value is its
    offset into the key's own elements) and its elements. Writes of 0, 1, 2, ...
    and reads, mixed evenly over n_procs processes; an :ok read returns every
    completed write plus a random subset of the writes in flight (:info writes
    stay in flight for good). A violating read shows one write and omits one
    that completed before that write's invoke."""
    from . import _abi as A
    rows, aux, n_aux = [], [], 0
    done = []                        # completed writes, in completion order
    flying = []                      # invoked, not (yet) completed
    before = {}                      # write -> how many of `done` were complete at its invoke
    pending = [None] * n_procs
    nxt, invoked = 0, 0
    while invoked < ops or any(x is not None for x in pending):
        p = int(rng.integers(n_procs))
        cur = pending[p]
        if cur is None:
            if invoked >= ops:
                continue
            invoked += 1
            if rng.random() < 0.5:
                pending[p] = ("r", None)
                rows.append((p, A.TYPE_INVOKE, A.F_READ, A.NIL, 0))
            else:
                pending[p] = ("w", nxt)
                before[nxt] = len(done)
                flying.append(nxt)
                rows.append((p, A.TYPE_INVOKE, A.F_WRITE, nxt, A.NIL))
                nxt += 1
            continue
        pending[p] = None
        info = rng.random() < p_info
        if cur[0] == "w":
            if info:
                rows.append((p, A.TYPE_INFO, A.F_WRITE, cur[1], A.NIL))
            else:
                flying.remove(cur[1])
                done.append(cur[1])
                rows.append((p, A.TYPE_OK, A.F_WRITE, cur[1], A.NIL))
            continue
        if info:
            rows.append((p, A.TYPE_INFO, A.F_READ, A.NIL, 0))
            continue
        seen = np.asarray(done + [x for x in flying if rng.random() < 0.5], np.int64)
        if n_viol > 0:
            shown = [x for x in seen.tolist() if before[x] > 0]
            if shown:
                x = shown[int(rng.integers(len(shown)))]
                gone = done[int(rng.integers(before[x]))]
                if gone != x:
                    seen = seen[seen != gone]
                    n_viol -= 1
        rng.shuffle(seen)
        rows.append((p, A.TYPE_OK, A.F_READ, n_aux, len(seen)))
        aux.append(seen)
        n_aux += len(seen)
    return np.asarray(rows, np.int64).reshape(-1, 5), (np.concatenate(aux) if aux else np.zeros(0, np.int64))


def causal_reverse_history(n_keys=64, ops_per_key=500, n_procs=5, violations=0, p_info=0.02, seed=0, tile=1,
                           concurrent=4):
    """A keyed causal-reverse history as Columns (key ids 0 .. n_keys * tile -
    1, `keys` the same numbers): ops_per_key invocations per key, `concurrent`
    keys interleaved at a time as independent/concurrent-generator runs them.
    violations: reads made to violate the write order (at most; spread over
    random keys, each key's at its first reads that can). tile: the block of
    n_keys keys is repeated with fresh key ids and element ranges of its own
    (large benchmark histories; violations are then per block)."""
    from . import _abi as A
    rng = np.random.default_rng(seed)
    viol = np.bincount(rng.integers(n_keys, size=violations), minlength=n_keys) if violations else np.zeros(n_keys, int)
    parts = [_causal_reverse_key(rng, ops_per_key, n_procs, p_info, int(viol[k])) for k in range(n_keys)]
    counts = np.asarray([len(r) for r, _ in parts], np.int64)
    aux_base = np.concatenate([[0], np.cumsum([len(a) for _, a in parts])]).astype(np.int64)
    N = int(counts.sum())
    out = np.empty((N, 5), np.int64)
    keycol = np.empty(N, np.int64)
    at = 0
    for g0 in range(0, n_keys, concurrent):
        ks = np.arange(g0, min(g0 + concurrent, n_keys))
        label = np.repeat(ks, counts[ks])
        rng.shuffle(label)
        slots = at + np.argsort(label, kind="stable")         # key by key, each key's slots ascending
        s0 = 0
        for k in ks:
            rows = parts[k][0].copy()
            rd = (rows[:, 2] == A.F_READ) & (rows[:, 1] == A.TYPE_OK)
            rows[rd, 3] += aux_base[k]
            sl = slots[s0:s0 + counts[k]]
            out[sl] = rows
            keycol[sl] = k
            s0 += counts[k]
        at += len(label)
    auxa = np.concatenate([a for _, a in parts]) if parts else np.zeros(0, np.int64)
    if len(auxa) == 0:
        auxa = np.zeros(1, np.int64)
    if tile > 1:
        rd = np.tile((out[:, 2] == A.F_READ) & (out[:, 1] == A.TYPE_OK), tile)
        shift = np.repeat(np.arange(tile, dtype=np.int64), N)
        keycol = np.tile(keycol, tile) + shift * n_keys
        n_aux = len(auxa)
        out = np.tile(out, (tile, 1))
        out[:, 3] += np.where(rd, shift * n_aux, 0)
        auxa = np.tile(auxa, tile)
    K = n_keys * tile
    return Columns(n=len(out), process=out[:, 0].copy(), type=out[:, 1].copy(), f=out[:, 2].copy(), key=keycol,
                   value=out[:, 3].copy(), value2=out[:, 4].copy(), n_keys=K, aux=auxa, keys=list(range(K)))


def causal_reverse_columns_to_ops(cols):
    """Op maps of a causal-reverse history's Columns (independent tuples for
    keyed rows; jepsen_amd/causal_reverse.py decode)."""
    from . import causal_reverse
    return causal_reverse.decode(cols)


def txn_cycle_history(n_ops=1000, n_procs=10, n_keys=100, anomalies=0, p_info=0.02, seed=0):
    """A transactional history for jepsen.tests.cycle as Columns (include/jh.h,
    "Cycle txns"): n_ops txns of n_procs processes, each one external read and
    one write ([:r k v] [:w k' v'], written values unique per key), taking
    effect at their invocation, so a reader may complete before its writer does
    (back edges) while wr + realtime stay acyclic. A crashed (:info) txn's
    process is replaced, as jepsen replaces it. anomalies: that many :ok txns
    are made to read what a txn invoked after their completion writes (a cycle
    through realtime edges each)."""
    from . import _abi as A
    rng = np.random.default_rng(seed)
    cur = np.full(n_keys, A.NIL, np.int64)
    nxt = np.zeros(n_keys, np.int64)
    proc, typ, val, val2, aux = [], [], [], [], []
    open_ = {}                                   # slot -> (process id, mops)
    pid = list(range(n_procs))
    txn_rows = []                                # (invoke row, completion row, type, aux index)
    started = 0
    slots = rng.integers(n_procs, size=4 * n_ops + 4 * n_procs)
    keys = rng.integers(n_keys, size=(n_ops, 2))
    infos = rng.random(n_ops) < p_info
    at = 0
    while started < n_ops or open_:
        s = int(slots[at % len(slots)])
        at += 1
        if s in open_:
            p, mi, row_i, t_i = open_.pop(s)
            t = A.TYPE_INFO if infos[t_i] else A.TYPE_OK
            txn_rows.append((row_i, len(proc), t, mi))
            proc.append(p); typ.append(t); val.append(mi); val2.append(2)
            if t == A.TYPE_INFO:
                pid[s] += n_procs
        elif started < n_ops:
            kr, kw = int(keys[started, 0]), int(keys[started, 1])
            nxt[kw] += 1
            mi = len(aux) // 3
            aux += [A.F_READ, kr, int(cur[kr]), A.F_WRITE, kw, int(nxt[kw])]
            cur[kw] = nxt[kw]
            open_[s] = (pid[s], mi, len(proc), started)
            proc.append(pid[s]); typ.append(A.TYPE_INVOKE); val.append(A.NIL); val2.append(0)
            started += 1
    oks = [t for t in txn_rows if t[2] == A.TYPE_OK]
    inv_rows = np.asarray([t[0] for t in oks], np.int64)
    for _ in range(anomalies):
        if len(oks) < 2:
            break
        a = oks[int(rng.integers(len(oks) // 2))]
        later = np.nonzero(inv_rows > a[1])[0]
        if len(later) == 0:
            continue
        b = oks[int(later[min(int(rng.integers(8)), len(later) - 1)])]
        aux[3 * a[3] + 1], aux[3 * a[3] + 2] = aux[3 * b[3] + 4], aux[3 * b[3] + 5]
    n = len(proc)
    return Columns(n=n, process=np.asarray(proc, np.int64), type=np.asarray(typ, np.int64),
                   f=np.full(n, A.F_FIRST_INTERNED, np.int64), key=np.full(n, -1, np.int64),
                   value=np.asarray(val, np.int64), value2=np.asarray(val2, np.int64), n_keys=0,
                   aux=np.asarray(aux if aux else [0, 0, 0], np.int64), keys=list(range(n_keys)), f_names=["txn"])


def txn_cycle_columns_to_ops(cols):
    """Op maps of txn_cycle_history's Columns: completions carry their txn as
    [f k v] micro-ops, invocations nil."""
    from . import _abi as A
    out = []
    for i in range(cols.n):
        v = None
        if int(cols.type[i]) != A.TYPE_INVOKE and int(cols.value2[i]) > 0:
            s, c = int(cols.value[i]), int(cols.value2[i])
            v = [["r" if int(cols.aux[3 * j]) == A.F_READ else "w", int(cols.aux[3 * j + 1]),
                  None if int(cols.aux[3 * j + 2]) == A.NIL else int(cols.aux[3 * j + 2])] for j in range(s, s + c)]
        p = int(cols.process[i])
        out.append({"process": p if p >= 0 else "nemesis", "type": ("invoke", "ok", "fail", "info")[int(cols.type[i])],
                    "f": "txn", "value": v})
    return out


def append_history(n_txns=1000, procs=10, keys=100, anomalies=0, p_info=0.02, seed=0, max_len=64):
    """A list-append history for appends-and-reads-graph as Columns (include/jh.h,
    "Append txns"): n_txns txns of `procs` processes, each [:r k v] [:append k' x]
    over `keys` live keys, under a serial schedule: a txn takes effect at its
    invocation, so every dependency follows invocation order and the healthy
    history has no cycle, with or without the realtime edges. A key's elements
    are 1, 2, ... in append order, so a read of length c is [1 .. c]. A key whose
    list reaches max_len is left for a fresh one, so read lengths stay below
    max_len. Invocations carry the txn with a nil read; an :info completion
    (its process is replaced) carries the append alone. anomalies: that many :ok
    txns read a shorter prefix than the state they were given (a stale read: an
    rw edge back to a txn that went before)."""
    from . import _abi as A
    rng = np.random.default_rng(seed)
    live = list(range(keys))                     # slot -> key id
    length = [0] * keys                          # key id -> elements so far
    proc, typ, val, val2 = [], [], [], []
    rk, rlen, ak, av = np.zeros(n_txns, np.int64), np.zeros(n_txns, np.int64), np.zeros(n_txns, np.int64), np.zeros(n_txns, np.int64)
    open_, pid, started, at = {}, list(range(procs)), 0, 0
    slots = rng.integers(procs, size=4 * n_txns + 4 * procs)
    picks = rng.integers(keys, size=(n_txns, 2))
    infos = rng.random(n_txns) < p_info
    ok_txns = []
    while started < n_txns or open_:
        s = int(slots[at % len(slots)])
        at += 1
        if s in open_:
            t = open_.pop(s)
            proc.append(pid[s])
            if infos[t]:
                typ.append(A.TYPE_INFO); val.append(16 * t + 4); val2.append(1)
                pid[s] += procs
            else:
                typ.append(A.TYPE_OK); val.append(16 * t + 8); val2.append(2)
                ok_txns.append(t)
        elif started < n_txns:
            t = started
            kr, kw = live[int(picks[t, 0])], live[int(picks[t, 1])]
            rk[t], rlen[t] = kr, length[kr]
            length[kw] += 1
            ak[t], av[t] = kw, length[kw]
            if length[kw] >= max_len:
                live[int(picks[t, 1])] = len(length)
                length.append(0)
            open_[s] = t
            proc.append(pid[s]); typ.append(A.TYPE_INVOKE); val.append(16 * t); val2.append(2)
            started += 1
    stale = [t for t in ok_txns if rlen[t] >= 2]
    for t in (rng.choice(stale, size=min(anomalies, len(stale)), replace=False).tolist() if stale and anomalies else ()):
        rlen[t] = int(rng.integers(0, rlen[t]))
    # words: per txn [r k _ 0] [append k' x 0] (the invocation) and [r k off len] [append k' x 0] (the :ok completion)
    words = np.zeros((n_txns, 16), np.int64)
    off = 16 * n_txns + np.cumsum(rlen) - rlen
    for base, ln_col in ((0, None), (8, rlen)):
        words[:, base], words[:, base + 1] = A.F_READ, rk
        words[:, base + 4], words[:, base + 5], words[:, base + 6] = A.F_APPEND, ak, av
        if ln_col is not None:
            words[:, base + 2], words[:, base + 3] = off, ln_col
    total = int(rlen.sum())
    elems = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(rlen) - rlen, rlen) + 1
    n = len(proc)
    return Columns(n=n, process=np.asarray(proc, np.int64), type=np.asarray(typ, np.int64),
                   f=np.full(n, A.F_FIRST_INTERNED, np.int64), key=np.full(n, -1, np.int64), value=np.asarray(val, np.int64),
                   value2=np.asarray(val2, np.int64), n_keys=len(length), aux=np.concatenate([words.reshape(-1), elems]),
                   keys=list(range(len(length))), f_names=["txn"])


def append_columns_to_ops(cols):
    """Op maps of Columns in the append txn encoding (append_history's, or
    cycle.encode_append's): every row carries its txn; an empty read is nil."""
    from . import _abi as A
    out = []
    for i in range(cols.n):
        v = None
        if int(cols.value2[i]) > 0 or int(cols.value[i]) != A.NIL:
            s, c = int(cols.value[i]), int(cols.value2[i])
            v = []
            for f, k, a, b in np.asarray(cols.aux[s:s + 4 * c]).reshape(-1, 4).tolist():
                v.append(["r", cols.keys[k], cols.aux[a:a + b].tolist() if b else None] if f == A.F_READ
                         else ["append", cols.keys[k], a])
        p = int(cols.process[i])
        out.append({"process": p if p >= 0 else "nemesis", "type": ("invoke", "ok", "fail", "info")[int(cols.type[i])],
                    "f": "txn", "value": v})
    return out


def monotonic_history(n_ops=1000, procs=10, keys=8, p_read=0.5, stale=0.0, p_info=0.02, seed=0):
    """A history of the increment workload (tidb/src/tidb/monotonic.clj) for
    monotonic-key-graph as Columns (include/jh.h, "Map reads encoding"): n_ops
    ops of `procs` processes over `keys` counters that start at 0. An :inc of k
    returns {k new}; a :read returns the current value of a random non-empty
    subset of the keys. An op takes effect at its invocation, so the healthy
    history has no cycle, alone or with the realtime and process edges. Every
    invoke is completed; an :info completion (its process is replaced) carries
    no map. stale: with that probability a :read returns one of its keys one
    behind. p_read = 0 gives chains of unique values (groups of one row),
    p_read near 1 a few values observed by many rows each (wide groups)."""
    from . import _abi as A
    rng = np.random.default_rng(seed)
    cur = [0] * keys
    proc, typ, f, val, val2, aux = [], [], [], [], [], []
    open_, pid, started, at = {}, list(range(procs)), 0, 0
    slots = rng.integers(procs, size=4 * n_ops + 4 * procs)
    reads = rng.random(n_ops) < p_read
    infos = rng.random(n_ops) < p_info
    stales = rng.random(n_ops) < stale
    inc_key = rng.integers(keys, size=n_ops)
    held = rng.random((n_ops, keys)) < 0.5
    while started < n_ops or open_:
        s = int(slots[at % len(slots)])
        at += 1
        if s in open_:
            t, pairs = open_.pop(s)
            proc.append(pid[s]); f.append(A.F_FIRST_INTERNED + int(reads[t]))
            if infos[t]:
                typ.append(A.TYPE_INFO); val.append(A.NIL); val2.append(0)
                pid[s] += procs
            else:
                typ.append(A.TYPE_OK); val.append(len(aux) // 2); val2.append(len(pairs) // 2)
                aux += pairs
        elif started < n_ops:
            t = started
            if reads[t]:
                ks = np.nonzero(held[t])[0].tolist() or [int(inc_key[t])]
                pairs = [x for k in ks for x in (k, cur[k])]
                behind = [j for j in range(len(ks)) if pairs[2 * j + 1] > 0]
                if stales[t] and behind:
                    pairs[2 * behind[int(rng.integers(len(behind)))] + 1] -= 1
            else:
                k = int(inc_key[t])
                cur[k] += 1
                pairs = [k, cur[k]]
            open_[s] = (t, pairs)
            proc.append(pid[s]); typ.append(A.TYPE_INVOKE); f.append(A.F_FIRST_INTERNED + int(reads[t]))
            val.append(A.NIL); val2.append(0)
            started += 1
    n = len(proc)
    return Columns(n=n, process=np.asarray(proc, np.int64), type=np.asarray(typ, np.int64), f=np.asarray(f, np.int64),
                   key=np.full(n, -1, np.int64), value=np.asarray(val, np.int64), value2=np.asarray(val2, np.int64), n_keys=0,
                   aux=np.asarray(aux + [0, 0], np.int64)[:len(aux)], keys=list(range(keys)), f_names=["inc", "read"])


def monotonic_columns_to_ops(cols):
    """Op maps of Columns in the map reads encoding (monotonic_history's, or
    cycle.encode_map's): an :ok row carries its map, every other row nil."""
    from . import _abi as A
    names = getattr(cols, "f_names", None) or ["read"]
    out = []
    for i in range(cols.n):
        v = None
        if int(cols.type[i]) == A.TYPE_OK and int(cols.value2[i]) > 0:
            s, c = int(cols.value[i]), int(cols.value2[i])
            v = {cols.keys[int(cols.aux[2 * j])]: (None if int(cols.aux[2 * j + 1]) == A.NIL else int(cols.aux[2 * j + 1]))
                 for j in range(s, s + c)}
        p = int(cols.process[i])
        fi = int(cols.f[i]) - A.F_FIRST_INTERNED
        out.append({"process": p if p >= 0 else "nemesis", "type": ("invoke", "ok", "fail", "info")[int(cols.type[i])],
                    "f": names[fi] if 0 <= fi < len(names) else "read", "value": v})
    return out


# ---------------------------------------------------------------------------
# causal workload, jepsen/src/jepsen/tests/causal.clj:118-130
CAUSAL_VIOLATIONS = ("stale-read", "broken-link", "skipped-write", "read-init")


def causal_history(n_keys=64, violations=0, seed=0, p_info=0.02, concurrent=8, n_procs=None):
    """A keyed causal history as Columns in the causal encoding (include/jh.h:
    aux = a (position, link) pair per row; key ids 0 .. n_keys - 1, `keys` the
    same numbers). Every key has one thread and the five ops [ri cw1 r cw2 r],
    an invocation and a completion each; about 2 * `concurrent` keys are in
    flight at a time and their rows interleave. An :ok completion takes the next
    value of a global increasing position and links to the key's previous
    position, the first to :init. With p_info a completion is :info instead, and
    the key's later ops :fail (its :ok ops stay a valid prefix). violations:
    that many distinct keys, complete ones, get one fault each, the kinds of
    CAUSAL_VIOLATIONS in turn: the last read returns the first write, a link
    names another position, the first write writes 2, the read-init returns 7."""
    from . import _abi as A
    rng = np.random.default_rng(seed)
    K, OPS = int(n_keys), 5
    n_procs = int(n_procs or concurrent)
    stop = np.where(rng.random((K, OPS)) < p_info, np.arange(OPS), OPS).min(axis=1)     # the first op that is not :ok
    bad = rng.choice(K, size=min(int(violations), K), replace=False) if violations else np.zeros(0, np.int64)
    stop[bad] = OPS
    f_op = np.asarray([A.F_READ_INIT, A.F_WRITE, A.F_READ, A.F_WRITE, A.F_READ], np.int64)
    v_inv = np.asarray([A.NIL, 1, A.NIL, 2, A.NIL], np.int64)
    v_ok = np.tile(np.asarray([0, 1, 1, 2, 2], np.int64), (K, 1))
    kinds = np.arange(len(bad)) % len(CAUSAL_VIOLATIONS)
    v_ok[bad[kinds == 0], 4] = 1
    v_ok[bad[kinds == 2], 1] = 2
    v_ok[bad[kinds == 3], 0] = 7
    op_idx = np.arange(OPS)[None, :]
    ctype = np.where(op_idx < stop[:, None], A.TYPE_OK, np.where(op_idx == stop[:, None], A.TYPE_INFO, A.TYPE_FAIL))
    # rows: (key, op, half) -> a time; a key's ten rows keep their order
    t = (np.arange(K)[:, None] // max(int(concurrent), 1) * 1.0 + rng.random((K, 1))) * 10 \
        + np.arange(2 * OPS)[None, :] + rng.random((K, 2 * OPS))
    t = np.sort(t, axis=1)
    order = np.argsort(t.ravel(), kind="stable")
    n = K * 2 * OPS
    row_of = np.empty(n, np.int64)
    row_of[order] = np.arange(n)
    row_of = row_of.reshape(K, OPS, 2)
    typ = np.empty(n, np.int64)
    f = np.empty(n, np.int64)
    key = np.empty(n, np.int64)
    val = np.full(n, A.NIL, np.int64)
    aux = np.full(2 * n, A.NIL, np.int64)
    kk = np.repeat(np.arange(K), OPS).reshape(K, OPS)
    for half in (0, 1):
        r = row_of[:, :, half]
        f[r] = f_op[None, :]
        key[r] = kk
        typ[r] = A.TYPE_INVOKE if half == 0 else ctype
    val[row_of[:, :, 0]] = v_inv[None, :]
    comp = row_of[:, :, 1]
    val[comp] = np.where(ctype == A.TYPE_OK, v_ok, v_inv[None, :])
    pos = comp + 1                                            # global and increasing along the history
    link = np.concatenate([np.full((K, 1), A.CAUSAL_INIT, np.int64), pos[:, :-1]], axis=1)
    which = 1 + rng.integers(OPS - 1, size=len(bad))
    sel = kinds == 1
    link[bad[sel], which[sel]] += 1 + 2 * n                   # no row has this position
    okm = ctype == A.TYPE_OK
    aux[2 * comp[okm]] = pos[okm]
    aux[2 * comp[okm] + 1] = link[okm]
    return Columns(n=n, process=key % n_procs, type=typ, f=f, key=key, value=val, value2=np.zeros(n, np.int64), n_keys=K,
                   aux=aux, keys=list(range(K)))


def causal_columns_to_ops(cols):
    """Op maps of a causal history's Columns (independent tuples for keyed
    rows; jepsen_amd/causal.py decode)."""
    from . import causal
    return causal.decode(cols)


# ---------------------------------------------------------------------------
# Adya G2 workload, jepsen/src/jepsen/tests/adya.clj:12-60
def g2_history(n_keys=64, illegal=0, seed=0, p_ok=0.5, p_info=0.1, concurrent=8, nemesis_every=1000):
    """A G2 history as Columns in the G2 encoding (include/jh.h): every key has
    two :insert ops on two threads, [key [nil b-id]] and [key [a-id nil]] with
    globally unique ids (value = the id, value2 = 0 for the first form and 1 for
    the second), an invocation and a completion each, about 2 * `concurrent`
    keys in flight at a time. Each completion is :ok, :fail or :info; only the
    `illegal` keys (distinct, random) have both :ok. A :nemesis :info row stands
    after every `nemesis_every` rows. Key ids 0 .. n_keys - 1 in order of first
    appearance are the keys themselves."""
    from . import _abi as A
    rng = np.random.default_rng(seed)
    K = int(n_keys)
    first_ok = rng.random(K) < p_ok
    second_ok = ~first_ok & (rng.random(K) < p_ok)
    ill = rng.choice(K, size=min(int(illegal), K), replace=False) if illegal else np.zeros(0, np.int64)
    first_ok[ill] = True
    second_ok[ill] = True
    oks = np.stack([first_ok, second_ok], axis=1)
    ctype = np.where(oks, A.TYPE_OK, np.where(rng.random((K, 2)) < p_info, A.TYPE_INFO, A.TYPE_FAIL))
    t_inv = (np.arange(K)[:, None] // max(int(concurrent), 1) * 1.0 + rng.random((K, 1))) * 4 + rng.random((K, 2))
    t = np.stack([t_inv, t_inv + 0.01 + 2 * rng.random((K, 2))], axis=2)       # (key, insert, invoke / completion)
    order = np.argsort(t.ravel(), kind="stable")
    m = 4 * K
    rank = np.empty(m, np.int64)
    rank[order] = np.arange(m)
    every = max(int(nemesis_every), 1)
    row_of = (rank + rank // every).reshape(K, 2, 2)          # a nemesis row after every `every` rows
    n = m + m // every
    typ = np.full(n, A.TYPE_INFO, np.int64)
    f = np.full(n, A.F_FIRST_INTERNED, np.int64)
    key = np.full(n, -1, np.int64)
    proc = np.full(n, -1, np.int64)
    val = np.full(n, A.NIL, np.int64)
    val2 = np.zeros(n, np.int64)
    ids = 1 + np.arange(2 * K).reshape(K, 2)
    # key ids in order of first appearance
    firsts = row_of.reshape(K, 4).min(axis=1)
    kid = np.empty(K, np.int64)
    kid[np.argsort(firsts, kind="stable")] = np.arange(K)
    for half in (0, 1):
        r = row_of[:, :, half]
        f[r] = A.F_INSERT
        key[r] = kid[:, None]
        proc[r] = 2 * (np.arange(K)[:, None] % max(int(concurrent), 1)) + np.arange(2)[None, :]
        typ[r] = A.TYPE_INVOKE if half == 0 else ctype
        val[r] = ids
        val2[r] = np.arange(2)[None, :]
    return Columns(n=n, process=proc, type=typ, f=f, key=key, value=val, value2=val2, n_keys=K, aux=np.zeros(1, np.int64),
                   keys=list(range(K)), f_names=["start"])


def g2_columns_to_ops(cols):
    """Op maps of a G2 history's Columns: an insert's :value is the independent
    tuple [key [nil id]] or [key [id nil]]."""
    from . import _abi as A
    from .history import TYPE_NAMES, tuple_
    out = []
    for i in range(cols.n):
        p = int(cols.process[i])
        op = {"process": p if p >= 0 else "nemesis", "type": TYPE_NAMES[int(cols.type[i])]}
        if int(cols.f[i]) == A.F_INSERT:
            v = int(cols.value[i])
            op["f"] = "insert"
            op["value"] = tuple_(cols.keys[int(cols.key[i])], [v, None] if int(cols.value2[i]) else [None, v])
        else:
            j = int(cols.f[i]) - A.F_FIRST_INTERNED
            op["f"] = cols.f_names[j] if 0 <= j < len(cols.f_names) else "start"
            op["value"] = None
        out.append(op)
    return out


# ---------------------------------------------------------------------------
# independent set workload, aerospike/src/aerospike/set.clj:48-72
def independent_set_history(n_keys=64, adds_per_key=100, threads_per_key=5, p_fail=0.05, p_info=0.02, n_lost_keys=0,
                            n_unexpected_keys=0, seed=0, concurrent=4, p_vector=0.25, nemesis_every=500):
    """A keyed set history as Columns (standard encoding: set reads in aux), the
    independent/concurrent-generator shape of aerospike's set workload: keys run
    in groups of `concurrent`, each on threads_per_key threads; a key is
    adds_per_key :add ops of the elements 0, 1, ... in ascending order (an
    invocation and an :ok / :fail / :info completion each), and after every add
    of every key one final :read per key (invocation and :ok). A read holds the
    key's acknowledged elements and each :info element with probability 1/2;
    n_lost_keys keys miss up to three acknowledged elements and
    n_unexpected_keys keys read up to three elements nobody added. Reads are
    ascending, except that with p_vector a read's elements are shuffled (a vector
    :value). Un-keyed :nemesis :info rows come every nemesis_every rows or so."""
    from . import _abi as A
    rng = np.random.default_rng(seed)
    K, N, T, G = int(n_keys), int(adds_per_key), max(int(threads_per_key), 1), max(int(concurrent), 1)
    u = rng.random((K, N))
    ctype = np.where(u < p_fail, A.TYPE_FAIL, np.where(u < p_fail + p_info, A.TYPE_INFO, A.TYPE_OK))
    # the final reads: N + 3 candidate elements per key
    present = np.zeros((K, N + 3), bool)
    present[:, :N] = (ctype == A.TYPE_OK) | ((ctype == A.TYPE_INFO) & (rng.random((K, N)) < 0.5))
    picks = rng.permutation(K)
    lost_keys, unexp_keys = picks[:min(int(n_lost_keys), K)], picks[::-1][:min(int(n_unexpected_keys), K)]
    if N > 0:
        for k in lost_keys:
            acked = np.nonzero(ctype[k] == A.TYPE_OK)[0]
            present[k, rng.choice(acked, size=min(3, len(acked)), replace=False)] = False
    for j, k in enumerate(unexp_keys):
        present[k, N:N + 1 + j % 3] = True
    rk, re = np.nonzero(present)
    cnt = present.sum(axis=1)
    shuf = rng.random(K) < p_vector
    order = np.lexsort((np.where(shuf[rk], rng.random(len(rk)) * (N + 3), re), rk))
    aux = re[order].astype(np.int64)
    roff = np.concatenate(([0], np.cumsum(cnt)[:-1])).astype(np.int64)
    # times: a key's group starts when the one before it is done; the reads come after every add
    g0 = (np.arange(K) // G * (N + T + 2.0))[:, None]
    t_inv = g0 + np.arange(N)[None, :] + 0.5 * rng.random((K, N))
    t_cmp = t_inv + 0.05 + 0.9 * T * rng.random((K, N))
    t_end = float(t_cmp.max()) + 1.0 if N and K else 1.0
    t_rinv = t_end + (np.arange(K) // G * 4.0) + rng.random(K)
    t_rcmp = t_rinv + 0.05 + rng.random(K)
    n_client = 2 * K * N + 2 * K
    n_nem = n_client // max(int(nemesis_every), 1) if nemesis_every else 0
    t_nem = rng.random(n_nem) * (float(t_rcmp.max()) if K else 1.0)
    times = np.concatenate([t_inv.ravel(), t_cmp.ravel(), t_rinv, t_rcmp, t_nem])
    n = len(times)
    row_of = np.empty(n, np.int64)
    row_of[np.argsort(times, kind="stable")] = np.arange(n)
    kk = np.repeat(np.arange(K), N)
    ee = np.tile(np.arange(N), K)
    proc_add = (kk % G) * T + ee % T
    proc = np.full(n, -1, np.int64)
    typ = np.full(n, A.TYPE_INFO, np.int64)
    f = np.full(n, A.F_FIRST_INTERNED, np.int64)
    key = np.full(n, -1, np.int64)
    val = np.full(n, A.NIL, np.int64)
    val2 = np.full(n, A.NIL, np.int64)
    a, b = K * N, 2 * K * N
    for rows, ty in ((row_of[:a], A.TYPE_INVOKE), (row_of[a:b], ctype.ravel())):
        proc[rows] = proc_add; typ[rows] = ty; f[rows] = A.F_ADD; key[rows] = kk; val[rows] = ee
    ri, rc = row_of[b:b + K], row_of[b + K:b + 2 * K]
    for rows in (ri, rc):
        proc[rows] = (np.arange(K) % G) * T; f[rows] = A.F_READ; key[rows] = np.arange(K)
    typ[ri] = A.TYPE_INVOKE
    typ[rc] = A.TYPE_OK
    val[rc] = roff
    val2[rc] = cnt
    # key ids in first-appearance order, as the encoder interns them
    first = np.full(K, n, np.int64)
    np.minimum.at(first, key[key >= 0], np.nonzero(key >= 0)[0])
    by_first = np.argsort(first, kind="stable")
    new_id = np.empty(K, np.int64)
    new_id[by_first] = np.arange(K)
    key[key >= 0] = new_id[key[key >= 0]]
    return Columns(n=n, process=proc, type=typ, f=f, key=key, value=val, value2=val2, n_keys=K,
                   aux=aux if len(aux) else np.zeros(1, np.int64), keys=by_first.tolist(), f_names=["start"])


def independent_set_columns_to_ops(cols):
    """Op maps of an independent set history's Columns: independent tuples for
    keyed rows, a read's :value the list of its elements in aux order."""
    from . import _abi as A
    from .history import TYPE_NAMES, tuple_
    out = []
    for i in range(cols.n):
        p, fi, k = int(cols.process[i]), int(cols.f[i]), int(cols.key[i])
        op = {"process": p if p >= 0 else "nemesis", "type": TYPE_NAMES[int(cols.type[i])]}
        v = None if int(cols.value[i]) == A.NIL else int(cols.value[i])
        if fi == A.F_ADD:
            op["f"] = "add"
        elif fi == A.F_READ:
            op["f"] = "read"
            if v is not None and int(cols.type[i]) == A.TYPE_OK:
                v = [int(x) for x in cols.aux[v:v + int(cols.value2[i])]]
        else:
            j = fi - A.F_FIRST_INTERNED
            op["f"] = cols.f_names[j] if 0 <= j < len(cols.f_names) else "start"
        op["value"] = tuple_(cols.keys[k], v) if k >= 0 else v
        out.append(op)
    return out


def perf_history(n=4096, procs=5, fs=("read", "write", "cas"), seed=0, p_fail=0.1, p_info=0.05, nemesis_every=1000,
                 dangling=False, mean_latency_ms=20.0, mean_think_ms=5.0):
    """A history for checker/perf as Columns with a `time` attribute (integer
    nanoseconds): about n rows of paired client ops on `procs` processes, each
    process's times increasing, the f drawn from `fs`, a share of :fail and
    :info completions; after every `nemesis_every` client rows a :nemesis :info
    pair, :start and :stop in turn (the two rows of a pair carry their
    neighbour's time). dangling: the last op of the last process never
    completes (an unpaired invoke). Only process, type, f and time mean
    anything; key, value and value2 are zeros."""
    from . import _abi as A
    from .history import KNOWN_F, Columns
    rng = np.random.default_rng(seed)
    P, n_ops = max(int(procs), 1), max(int(n) // 2, 0)
    names, code = [], {}
    for f in list(fs) + ["start", "stop"]:
        if f in KNOWN_F:
            code[f] = KNOWN_F[f]
        elif f not in code:
            code[f] = A.F_FIRST_INTERNED + len(names)
            names.append(f)
    op_p = np.arange(n_ops) % P
    lat = 1 + rng.exponential(mean_latency_ms * 1e6, n_ops).astype(np.int64)
    think = 1 + rng.exponential(mean_think_ms * 1e6, n_ops).astype(np.int64)
    t_inv = np.zeros(n_ops, np.int64)
    for p in range(P):                                        # a process's ops follow one another
        sel = np.nonzero(op_p == p)[0]
        t_inv[sel] = np.cumsum(think[sel] + np.concatenate(([0], lat[sel][:-1])))
    u = rng.random(n_ops)
    ctype = np.where(u < p_fail, A.TYPE_FAIL, np.where(u < p_fail + p_info, A.TYPE_INFO, A.TYPE_OK))
    f_op = np.asarray([code[f] for f in fs], np.int64)[rng.integers(0, len(fs), n_ops)] if n_ops else np.zeros(0, np.int64)
    t = np.concatenate([t_inv, t_inv + lat])
    typ = np.concatenate([np.full(n_ops, A.TYPE_INVOKE), ctype])
    proc = np.concatenate([op_p, op_p])
    f = np.concatenate([f_op, f_op])
    keep = np.ones(2 * n_ops, bool)
    if dangling and n_ops:
        keep[n_ops + np.nonzero(op_p == P - 1)[0][-1]] = False
    order = np.argsort(t, kind="stable")
    order = order[keep[order]]
    t, typ, proc, f = t[order], typ[order], proc[order], f[order]
    every = max(int(nemesis_every), 1)
    cuts = np.arange(every, len(t) + 1, every)                # a nemesis pair after these many client rows
    if len(cuts):
        at = np.repeat(cuts, 2)
        nf = np.repeat(np.where(np.arange(len(cuts)) % 2 == 0, code["start"], code["stop"]), 2)
        t = np.insert(t, at, t[at - 1])
        typ = np.insert(typ, at, A.TYPE_INFO)
        proc = np.insert(proc, at, -1)
        f = np.insert(f, at, nf)
    m = len(t)
    z = np.zeros(m, np.int64)
    cols = Columns(n=m, process=proc.astype(np.int64), type=typ.astype(np.int64), f=f.astype(np.int64), key=z, value=z,
                   value2=z, n_keys=0, aux=np.zeros(1, np.int64), f_names=names)
    cols.time = t.astype(np.int64)
    return cols


def perf_columns_to_ops(cols):
    """Op maps (process, type, f, time, index) of a perf history's Columns."""
    from . import _abi as A
    from .history import KNOWN_F, TYPE_NAMES
    known = {v: k for k, v in KNOWN_F.items()}
    out = []
    for i in range(cols.n):
        p, c = int(cols.process[i]), int(cols.f[i])
        out.append({"process": p if p >= 0 else "nemesis", "type": TYPE_NAMES[int(cols.type[i])],
                    "f": known[c] if c in known else cols.f_names[c - A.F_FIRST_INTERNED], "time": int(cols.time[i]),
                    "index": i})
    return out


# ---------------------------------------------------------------------------
def multi_register_history(n_keys=64, ops_per_key=100, threads=10, regs=3, values=5, p_info=0.02, faulted_keys=(),
                           seed=0, concurrent=4):
    """Op maps of the multi-register workload (yugabyte multi_key_acid.clj:95-127),
    keyed by independent tuples: per key `threads` threads invoke txns -- a
    random non-empty subset of the `regs` registers, all reads ([:r k nil],
    values filled in on the completion) or all writes of values below `values`
    -- and a txn takes effect at a random point between its invocation and its
    completion. With probability p_info an op crashes instead (an :info row; it
    took effect or never will) and its thread goes on as process + threads
    (core.clj:349). A faulted key has one micro-op of one :ok read changed to
    another value; that does not always make the key invalid. faulted_keys: key
    numbers, or how many (spread evenly). Keys run in groups of `concurrent`,
    their rows interleaved."""
    import random
    from .history import tuple_
    rng = random.Random(seed)
    if isinstance(faulted_keys, int):
        faulted_keys = [k * n_keys // faulted_keys for k in range(faulted_keys)] if faulted_keys > 0 else []
    faulted = set(faulted_keys)

    def one_key(k):
        state, out, reads = {}, [], []
        proc = list(range(threads))
        pend = [None] * threads            # [f, txn, applied, result]
        invoked = 0
        while True:
            live = [t for t in range(threads) if pend[t] is not None or invoked < ops_per_key]
            if not live:
                break
            t = rng.choice(live)
            p = pend[t]
            if p is None:
                sub = [r for r in range(regs) if rng.random() < 0.5] or [rng.randrange(regs)]
                if rng.random() < 0.5:
                    f, txn = "read", [["r", r, None] for r in sub]
                else:
                    f, txn = "write", [["w", r, rng.randrange(values)] for r in sub]
                out.append({"process": proc[t], "type": "invoke", "f": f, "value": tuple_(k, txn)})
                pend[t] = [f, txn, False, None]
                invoked += 1
                continue
            crash = rng.random() < p_info
            if not p[2] and not (crash and rng.random() < 0.5):
                p[2] = True                # the txn takes effect
                if p[0] == "read":
                    p[3] = [["r", r, state.get(r)] for _, r, _ in p[1]]
                else:
                    for _, r, v in p[1]:
                        state[r] = v
                    p[3] = p[1]
                if not crash:
                    continue
            if crash:
                out.append({"process": proc[t], "type": "info", "f": p[0], "value": tuple_(k, p[1])})
                proc[t] += threads
            else:
                if p[0] == "read":
                    reads.append(len(out))
                out.append({"process": proc[t], "type": "ok", "f": p[0], "value": tuple_(k, p[3])})
            pend[t] = None
        if k in faulted and reads:
            op = out[rng.choice(reads)]
            txn = [list(m) for m in op["value"].val]
            m = rng.choice(txn)
            m[2] = rng.choice([v for v in range(values) if v != m[2]] or [values])
            op["value"] = tuple_(k, txn)
        return out

    history = []
    for g in range(0, n_keys, max(1, concurrent)):
        parts = [one_key(k) for k in range(g, min(n_keys, g + max(1, concurrent)))]
        at = [0] * len(parts)
        left = [i for i, p in enumerate(parts) if p]
        while left:
            i = rng.choice(left)
            history.append(parts[i][at[i]])
            at[i] += 1
            if at[i] == len(parts[i]):
                left.remove(i)
    return history
