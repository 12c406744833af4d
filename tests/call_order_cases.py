"""Targets and primers of the call-order parity tests (not a test module).

Every flat-scan checker keeps its scratch in grow-only workspace slots of the
context, and hipMalloc does not zero: a checker has to rewrite, on every call,
each counter, histogram, bitmap, tile count and meta struct it reads. The
tests of test_gpu_call_order.py run, on one context, a large history and then
small ones through the same entry point (and through the others), and compare
every call with the CPU references of tests/. This module builds the inputs
and holds, per entry point, the glue between a device call and its reference;
test_call_order_cases.py keeps the builders honest without a device.

Per entry point (an Entry of ENTRIES, in the order of include/jh.h):

  targets   small histories with known reference answers: the module's own
            hand-written cases where it has them, n = 0, n = 1, and one
            history at T - 1, T and T + 1 rows (or keys, or sorted slots,
            whatever the checker's tile counts), T its tile constant.
  dirty     a primer of two tiles plus an odd remainder (or more), larger
            than every target in every dimension the checker sizes a buffer
            by, invalid, with error lists longer than any cap a target is
            called with.
  clean     a primer of the same size that is valid.

A target is called with caps of its own list lengths + SLACK, so a stale entry
of a primer's longer list would show; a primer with caps of exactly its list
lengths. `want` is always the reference's answer, never a device's.
"""
import functools

import numpy as np

import bank_cases
import bank_ref
import causal_cases
import causal_ref
import causal_reverse_cases
import causal_reverse_ref
import counter_ref
import cycle_append_ref
import cycle_cases
import cycle_mono_ref
import cycle_ref
import g2_cases
import g2_ref
import long_fork_cases
import long_fork_ref
import perf_cases
import perf_ref
import scan_cases as S
import set_full_cases
import set_ref
import unique_ids_ref
from jepsen_amd import _abi as A
from jepsen_amd import adya, bank, checker, synth
from jepsen_amd import causal as CM
from jepsen_amd import causal_reverse as CR
from jepsen_amd import cycle as CY
from jepsen_amd import history as H
from jepsen_amd import long_fork as LF
from jepsen_amd import perf as P
from jepsen_amd._native import bits_to_runs
from oracle import queue as Q
from oracle import set_full as SF

SLACK = 3                       # a target's caps: its own list lengths + SLACK
SCAN_TILE = 2048                # CHUNK / CNT_TILE of jh_counter.hip, jh_set.hip, jh_uids.hip, jh_bank.hip, jh_queue.hip
SF_GROUP = 256                  # elements per workgroup of jh_setfull.hip's k_sf_elem
NEM = {"process": "nemesis", "type": "info", "f": "start", "value": None}


def plain(x):
    """numpy arrays and scalars as Python lists and ints, recursively."""
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x


class Case:
    """One input of an entry point: `cols` (Columns) and whatever else the call
    and the reference need (ops, time, n, ...)."""

    def __init__(self, name, cols=None, **kw):
        self.name, self.cols = name, cols
        self.__dict__.update(kw)

    def __repr__(self):
        return f"Case({self.name})"


def head(cols, k, aux_per_row=0):
    """The first k rows of a Columns history; aux whole, or its first
    aux_per_row * k entries."""
    cut = {name: (None if getattr(cols, name) is None else np.ascontiguousarray(getattr(cols, name)[:k]))
           for name in ("process", "type", "f", "key", "value", "value2")}
    aux = cols.aux if not aux_per_row else np.ascontiguousarray(cols.aux[:aux_per_row * k])
    if aux is not None and len(aux) == 0:
        aux = np.zeros(0, np.int64)
    out = H.Columns(n=k, n_keys=cols.n_keys, aux=aux, **cut)
    for name in ("keys", "f_names", "value_table"):
        if getattr(cols, name, None) is not None:
            setattr(out, name, getattr(cols, name))
    return out


def ms_pairs(m):
    """A multiset {value: multiplicity} as jh.h orders its pairs: ascending
    value, nil last."""
    return [[v, c] for v, c in sorted((x for x in m.items() if x[0] is not None))] + \
        ([[None, m[None]]] if None in m else [])


def unscalar(cols, v):
    """A value of a queue history as the op maps hold it: nil, or through the
    value table where encode interned the values."""
    if v == A.NIL:
        return None
    return cols.value_table[v] if getattr(cols, "values_interned", False) else v


def raw_pairs(cols, a):
    """The device's (value, multiplicity) pairs as op-map values. Interned
    values come back in the order of their codes: put into ms_pairs' order (the
    list is whole, a target's cap is above its length)."""
    out = [[unscalar(cols, v), c] for v, c in plain(a)]
    if getattr(cols, "values_interned", False):
        out.sort(key=lambda p: (p[0] is None, 0 if p[0] is None else p[0]))
    return out


class Entry:
    """The glue of one entry point. ref(case, path): the reference's whole
    answer as plain Python; run(ctx, case, path, caps, dev): the device's, in
    the same shape, from host columns or (dev: a hipcols.DevCols, dev_time) from
    device-resident ones; cut(full, caps): the answer a call with these caps
    must give."""
    name = None
    paths = (0,)                # the forced paths; (0,) where the entry point has none
    capped = ()                 # the output lists a cap cuts
    clean_only = ()             # those of them only a valid history fills: the clean primer's is the long one
    error_dims = ()             # dims() that count errors: the dirty primer's alone exceeds the targets'
    on_device = True            # takes a jh_history (jh_scc does not)

    def build(self):
        raise NotImplementedError

    @functools.lru_cache(maxsize=None)
    def cases(self):
        c = self.build()
        assert {"targets", "dirty", "clean"} <= set(c)
        return c

    def all_cases(self):
        c = self.cases()
        return list(c["targets"]) + [c["dirty"], c["clean"]]

    def target(self, name):
        return next(t for t in self.cases()["targets"] if t.name == name)

    def paths_of(self, case):
        return self.paths

    @functools.lru_cache(maxsize=None)
    def full(self, case, path=0):
        return self.ref(case, path)

    def lists(self, full):
        return {k: len(full[k]) for k in self.capped}

    def caps(self, case, path=0):
        slack = 0 if case.name in ("dirty", "clean") else SLACK
        return {k: n + slack for k, n in self.lists(self.full(case, path)).items()}

    def cut(self, full, caps):
        return dict(full, **{k: full[k][:caps[k]] for k in self.capped})

    def want(self, case, path=0, caps=None):
        return self.cut(self.full(case, path), self.caps(case, path) if caps is None else caps)

    def valid(self, full):
        return full["valid"] == A.VALID

    def dims(self, case):
        """The sizes the checker allocates by."""
        d = {"rows": int(case.cols.n)}
        d.update(self.lists(self.full(case, self.paths_of(case)[0])))
        return d

    def check(self, ctx, case, path=0, dev=None, what=""):
        """One device call against the reference, field by field."""
        caps = self.caps(case, path)
        want = self.want(case, path, caps)
        got = self.run(ctx, case, path, caps, dev)
        bad = {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}
        assert not bad, (self.name, case.name, path, what, {k: _short(v) for k, v in bad.items()})
        return want


def _short(v):
    s = repr(v)
    return s if len(s) < 400 else s[:400] + "..."


def _dev(dev, cols):
    return (dev[0], True) if dev is not None else (cols, False)


# -- counter ------------------------------------------------------------------------
class Counter(Entry):
    name = "counter"
    capped = ("reads",)
    VALUES = [1 << 49, -(1 << 49), 5]           # LLONG_MAX / (adds of the primer) > 2^49: inside the overflow guard

    def case(self, name, ops):
        ops, cols = S.encode(ops)
        return Case(name, cols, ops=ops)

    def build(self):
        t = [self.case("n0", []), self.case("n1", S.counter_random(1, 1, [1], 1))]
        for d in (-1, 0, 1):
            n = SCAN_TILE + d
            t.append(self.case(f"T{d:+d}", S.counter_random(n, 3, [1, 2, 3], 100 + n, p_bad=0.0)))
        t.append(self.case("T+1-bad", S.counter_random(SCAN_TILE + 1, 3, [1, -1, 3], 7, p_bad=0.3)))
        n = 4 * SCAN_TILE + 37
        return {"targets": t,
                "dirty": self.case("dirty", S.counter_random(n, 40, self.VALUES, 3, p_read=0.4, p_bad=0.9, p_fail=0.0)),
                "clean": self.case("clean", S.counter_random(n, 40, [1 << 49, 5, 3], 4, p_read=0.4, p_bad=0.0))}

    def ref(self, case, path):
        r = counter_ref.check(case.ops)
        r["reads"] = [[A.NIL if x is None else x for x in t] for t in r["reads"]]
        return r

    def run(self, ctx, case, path, caps, dev):
        cols, on = _dev(dev, case.cols)
        return plain(ctx.check_counter(cols, reads_cap=caps["reads"], on_device=on))


# -- set, set-bitmaps ---------------------------------------------------------------
class Set(Entry):
    name = "set"
    FIELDS = ("valid", "cause", "first_fail_entry", "final_read_entry") + set_ref.COUNTS

    def case(self, name, ops):
        ops, cols = S.encode(ops)
        return Case(name, cols, ops=ops)

    def build(self):
        base = S.set_history(S.gapped(SCAN_TILE // 2 - 1), 11, later_reads=False, n_lost=0, n_unexpected=0)
        assert len(base) == SCAN_TILE
        t = [self.case("n0", []), self.case("n1", [S.inv(0, "add", 5)]),
             self.case("never-read", [S.inv(0, "add", 5), S.ok(0, "add", 5)]),
             self.case("T-1", base[1:]), self.case("T", base), self.case("T+1", base + [S.info(12, "read", None)]),
             self.case("T+1-lost", S.set_history(S.gapped(SCAN_TILE // 2 - 1, vmin=-70), 12, later_reads=False, n_lost=2,
                                                 n_unexpected=1) + [S.info(12, "read", None)])]
        m, far = 2 * SCAN_TILE + 17, (1 << 62) - 40_000
        return {"targets": t,
                "dirty": self.case("dirty", S.set_history(S.gapped(m, vmin=far, run=5, gap=2), 5, order="shuffled", n_lost=300,
                                                          n_unexpected=200, p_info=0.2)),
                "clean": self.case("clean", S.set_history(S.gapped(m, vmin=-far, run=5, gap=2), 6, order="shuffled", n_lost=0,
                                                          n_unexpected=0))}

    def ref(self, case, path):
        r = set_ref.check(case.ops)
        return dict({k: r[k] for k in self.FIELDS}, n_runs=r["n_runs"], runs=r["runs"])

    def lists(self, full):
        return {"runs": max(full["n_runs"])}

    def cut(self, full, caps):
        return dict(full, runs=[r[:caps["runs"]] for r in full["runs"]])

    def run(self, ctx, case, path, caps, dev):
        cols, on = _dev(dev, case.cols)
        r = ctx.check_set(cols, runs_cap=caps["runs"], on_device=on)
        return dict({k: r[k] for k in self.FIELDS}, n_runs=list(r["n_runs"]), runs=plain(r["runs"]))

    def dims(self, case):
        els = [o["value"] for o in case.ops if o["f"] == "add" and o["value"] is not None] + \
            [x for o in case.ops if o["f"] == "read" and o["value"] for x in o["value"]]
        return dict(Entry.dims(self, case), n_aux=len(case.cols.aux), span=max(els) - min(els) + 1 if els else 0)


class SetBitmaps(Set):
    """The sets as bitmaps: called with words for the whole span (the wrapper
    sizes them), compared as the runs of the bits."""
    name = "set-bitmaps"

    def run(self, ctx, case, path, caps, dev):
        cols, on = _dev(dev, case.cols)
        r = ctx.check_set_bitmaps(cols, on_device=on)
        return dict({k: r[k] for k in self.FIELDS}, n_runs=list(r["n_runs"]),
                    runs=[bits_to_runs(r["bits"][i], r["base"]).tolist() for i in range(4)])

    def cut(self, full, caps):
        return full


# -- set-full -----------------------------------------------------------------------
def _flat_worst(m):
    m = dict(m)
    m["worst-stale"] = [[r["element"], r["stable-latency"], r["known"]["index"],
                         r["last-absent"]["index"] if r["last-absent"] else -1] for r in m["worst-stale"]]
    return m


class SetFull(Entry):
    name = "set-full"
    capped = ("lost", "never-read", "stale")

    def case(self, name, ops):
        cols, time = set_full_cases.encode(ops)
        if len(time) == 0:
            time = np.zeros(1, np.int64)
        return Case(name, cols, ops=ops, time=time)

    def synth_case(self, name, **kw):
        cols, time = synth.set_full_history(**kw)
        ops = [dict(o, index=i) for i, o in enumerate(synth.columns_to_ops(cols, time))]
        return Case(name, cols, ops=ops, time=time)

    def build(self):
        t = [self.case("n0", []), self.case("n1", set_full_cases.stamp([set_full_cases.op(0, "invoke", "add", 7)], [5]))]
        for d in (-1, 0, 1):
            t.append(self.case(f"T{d:+d}", set_full_cases.sweep_case(SF_GROUP + d, 2)))
        t.append(self.case("64x64", set_full_cases.sweep_case(64, 64)))
        n = 2 * SCAN_TILE + 37
        return {"targets": t,
                "dirty": self.synth_case("dirty", n_adds=n, n_lost=300, n_stale=300, p_info=0.2, read_every=7, seed=3),
                "clean": self.synth_case("clean", n_adds=n, n_lost=0, n_stale=0, p_info=0.0, p_fail=0.0, read_every=7, seed=4)}

    def ref(self, case, path):
        return plain(_flat_worst(SF.set_full(case.ops, linearizable=True)))

    def valid(self, full):
        return full["valid?"] is True

    def cut(self, full, caps):
        cap = max(caps.values())                # one list_cap for the three lists
        return dict(full, **{k: full[k][:cap] for k in self.capped})

    def run(self, ctx, case, path, caps, dev):
        cols, on = _dev(dev, case.cols)
        time = dev[1] if on else case.time
        r = ctx.check_set_full(cols, time, linearizable=True, list_cap=max(caps.values()), on_device=on)
        return plain(_flat_worst(checker.set_full_result(r, case.ops, case.time)))

    def dims(self, case):
        return dict(Entry.dims(self, case), n_aux=len(case.cols.aux), elements=self.full(case)["attempt-count"])


# -- queues -------------------------------------------------------------------------
MULTISETS = ("lost", "unexpected", "duplicated", "recovered")


class TotalQueue(Entry):
    name = "total-queue"
    capped = MULTISETS
    COUNTS = ("attempt", "acknowledged", "ok", "unexpected", "duplicated", "lost", "recovered")

    def case(self, name, ops):
        return Case(name, S.encode(ops)[1], ops=ops)

    def synth_case(self, name, **kw):
        cols = synth.queue_history(**kw)
        return Case(name, cols, ops=synth.queue_columns_to_ops(cols))

    def build(self):
        long_ = S.queue_history(range(-20, 60), 21, n_ops=1200, p_nil=0.05, p_unexpected=0.002, p_dup=0.002)
        assert len(long_) > SCAN_TILE + 1
        t = [self.case("n0", []), self.case("n1", [S.inv(0, "enqueue", 3)]),
             self.case("nil-values", S.QUEUE_CASES["nil-values"]()), self.case("drains", S.QUEUE_CASES["drains"]()),
             self.case("S-3-clean", S.QUEUE_CASES["S-3-clean"]())]
        t += [self.case(f"T{d:+d}", long_[:SCAN_TILE + d]) for d in (-1, 0, 1)]
        n = 2 * SCAN_TILE + 37
        return {"targets": t,
                "dirty": self.synth_case("dirty", n_enqueues=n, n_lost=300, n_unexpected=300, n_duplicated=300, n_repeat=50,
                                         p_info=0.2, seed=5),
                "clean": self.synth_case("clean", n_enqueues=n, p_info=0.0, seed=6)}

    def ref(self, case, path):
        w = Q.total_queue(case.ops)
        out = {"valid": A.VALID if w["valid?"] else A.INVALID}
        out.update({k + "_count": w[k + "-count"] for k in self.COUNTS})
        out.update({k: ms_pairs(w[k]) for k in MULTISETS})
        out["n_pairs"] = [len(out[k]) for k in MULTISETS]
        return out

    def cut(self, full, caps):
        cap = max(caps.values())
        return dict(full, **{k: full[k][:cap] for k in MULTISETS})

    def run(self, ctx, case, path, caps, dev):
        cols, on = _dev(dev, case.cols)
        r = ctx.check_total_queue(cols, pairs_cap=max(caps.values()), on_device=on)
        out = {k: r[k] for k in ["valid", "n_pairs"] + [c + "_count" for c in self.COUNTS]}
        out.update({k: raw_pairs(case.cols, r[k]) for k in MULTISETS})
        return out

    def dims(self, case):
        vals = [o["value"] for o in case.ops if o["f"] in ("enqueue", "dequeue") and o["value"] is not None]
        return dict(Entry.dims(self, case), n_aux=len(case.cols.aux), span=max(vals) - min(vals) + 1 if vals else 0)


class Queue(TotalQueue):
    """(checker/queue (model/unordered-queue)): the first failing row and its
    value, or the final queue."""
    name = "queue"
    capped = ("final_queue",)
    clean_only = ("final_queue",)

    def ref(self, case, path):
        w = Q.queue(case.ops)
        if w["valid?"]:
            fq = ms_pairs(w["final-queue"])
            return {"valid": A.VALID, "fail_entry": -1, "error": None, "final_queue": fq, "n_final": len(fq)}
        return {"valid": A.INVALID, "fail_entry": w["fail-index"], "error": w["error"], "final_queue": [], "n_final": None}

    def cut(self, full, caps):
        return dict(full, final_queue=full["final_queue"][:caps["final_queue"]])

    def run(self, ctx, case, path, caps, dev):
        cols, on = _dev(dev, case.cols)
        r = ctx.check_queue(cols, pairs_cap=caps["final_queue"], on_device=on)
        if r["valid"] == A.VALID:
            return {"valid": A.VALID, "fail_entry": r["fail_entry"], "error": None, "final_queue": raw_pairs(case.cols, r["final_queue"]),
                    "n_final": r["n_pairs"][0]}
        v = unscalar(case.cols, r["fail_value"])
        return {"valid": r["valid"], "fail_entry": r["fail_entry"], "error": "can't dequeue %s" % (v,), "final_queue": [],
                "n_final": None}

    def dims(self, case):
        d = TotalQueue.dims(self, case)
        d.pop("final_queue")
        return d


# -- unique-ids ---------------------------------------------------------------------
class UniqueIds(Entry):
    name = "unique-ids"
    paths = (1, 2)
    capped = ("duplicated",)
    HAND = {
        "no-generate": [("invoke", None, 0, "read"), ("ok", 5, 0, "read")],
        "only-invokes": [("invoke", None, p, "generate") for p in range(5)],
        "all-nil": [("invoke", None, p, "generate") for p in range(3)] + [("ok", None, p, "generate") for p in range(3)],
        "fail-info-carry-an-acked-id": [("invoke", None, 0, "generate"), ("ok", 4, 0, "generate"), ("invoke", None, 1, "generate"),
                                        ("fail", 4, 1, "generate"), ("invoke", None, 2, "generate"), ("info", 4, 2, "generate"),
                                        ("invoke", None, 3, "generate"), ("ok", 9, 3, "generate")],
        "one-duplicate": [("ok", -12345678901, p, "generate") for p in range(2)] + [("ok", -12345678899, 2, "generate")],
    }

    def hand(self, name):
        ops = [{"process": p, "type": t, "f": f, "value": v} for t, v, p, f in self.HAND[name]]
        cols = H.encode(ops, keyed=False)
        assert not cols.values_interned
        return Case(name, cols)

    def build(self):
        t = [Case("n0", H.encode([], keyed=False))] + [self.hand(name) for name in self.HAND]
        t.append(Case("n1", head(self.hand("one-duplicate").cols, 1)))
        edge = synth.unique_ids_history(n_ops=SCAN_TILE, n_procs=8, dups=((2, 3),), nil_acks=1, seed=2)
        assert edge.n > SCAN_TILE + 1
        t += [Case(f"T{d:+d}", head(edge, SCAN_TILE + d)) for d in (-1, 0, 1)]
        n = 2 * SCAN_TILE + 37
        dirty = synth.unique_ids_history(n_ops=n, n_procs=8, dups=((1500, 2), (60, 3)), nil_acks=9, p_fail=0.0, p_info=0.0, seed=3)
        ids = (dirty.f == unique_ids_ref.f_generate(dirty)) & (dirty.value != A.NIL)
        dirty.value = np.where(ids, dirty.value + (1 << 62), dirty.value)       # ids near 2^62
        clean = synth.unique_ids_history(n_ops=n, n_procs=8, seed=4)
        return {"targets": t, "dirty": Case("dirty", dirty), "clean": Case("clean", clean)}

    def want(self, case, path=0, caps=None):
        caps = self.caps(case, path) if caps is None else caps
        return self.ref(case, path, caps["duplicated"])         # the cap keeps the largest counts: no prefix

    def ref(self, case, path, cap=1 << 30):
        r = unique_ids_ref.ref_cols(case.cols, cap)
        r["duplicated"] = [[k, c] for k, c in r["duplicated"].items()]
        return r

    def valid(self, full):
        return full["valid?"]

    def run(self, ctx, case, path, caps, dev):
        cols, on = _dev(dev, case.cols)
        r = ctx.check_unique_ids(cols, unique_ids_ref.f_generate(case.cols), path=path, dup_cap=caps["duplicated"], on_device=on)
        assert r["path"] in (0, 1, path), r["path"]

        def back(x):
            return None if x == A.NIL else int(x)
        return {"valid?": r["valid"] == A.VALID, "attempted-count": r["attempted_count"],
                "acknowledged-count": r["acknowledged_count"], "duplicated-count": r["duplicated_count"],
                "duplicated": [[back(i), int(c)] for i, c in r["duplicated"]], "range": [back(r["range_lo"]), back(r["range_hi"])]}

    def dims(self, case):
        c = case.cols
        ids = np.asarray(c.value)[(np.asarray(c.f) == unique_ids_ref.f_generate(c)) & (np.asarray(c.type) == A.TYPE_OK)]
        ids = ids[ids != A.NIL]
        return dict(Entry.dims(self, case), acks=self.full(case)["acknowledged-count"],
                    span=int(ids.max()) - int(ids.min()) + 1 if len(ids) else 0)


# -- bank ---------------------------------------------------------------------------
class Bank(Entry):
    name = "bank"
    capped = ("reads",)
    error_dims = ("errors",)

    def build(self):
        t = [Case("n0", bank.encode([], [0, 1, 2])[0], n_acc=3, total=10, negb=False)]
        for name, (test, opts, h, _) in bank_cases.CASES.items():
            cols, _ = bank.encode(h, test["accounts"])
            t.append(Case(name, cols, n_acc=len(set(test["accounts"])), total=test["total-amount"],
                          negb=bool(opts.get("negative-balances?"))))
        edge = synth.bank_history(n_ops=SCAN_TILE // 2 + 8, wrong=[3], nils=[40], seed=2)
        t.append(Case("n1", head(edge, 1), n_acc=8, total=100, negb=False))
        t += [Case(f"T{d:+d}", head(edge, SCAN_TILE + d), n_acc=8, total=100, negb=False) for d in (-1, 0, 1)]
        n = 2 * SCAN_TILE + 19
        every = range(0, n, 4)
        dirty = synth.bank_history(n_ops=n, p_read=1.0, p_info=0.0, noise=False, unexpected=every, nils=[i + 1 for i in every],
                                   wrong=[i + 2 for i in every], negative=[i + 3 for i in every], total=(1 << 61), seed=3)
        clean = synth.bank_history(n_ops=n, p_read=1.0, p_info=0.0, noise=False, total=(1 << 61), seed=4)
        return {"targets": t, "dirty": Case("dirty", dirty, n_acc=8, total=1 << 61, negb=False),
                "clean": Case("clean", clean, n_acc=8, total=1 << 61, negb=False)}

    def ref(self, case, path):
        w = bank_ref.ref_cols(case.cols, case.n_acc, case.total, case.negb, exact=True)
        tri = plain(w.pop("triples"))
        if "raises" in w:
            return {"valid": A.UNKNOWN, "cause": 7, "reads": tri, "n_reads": len(tri), "map": None}
        return {"valid": A.VALID if w["valid?"] else A.INVALID, "cause": 0, "reads": tri, "n_reads": len(tri), "map": plain(w)}

    def run(self, ctx, case, path, caps, dev):
        cols, on = _dev(dev, case.cols)
        r = ctx.check_bank(cols, case.n_acc, case.total, case.negb, reads_cap=caps["reads"], on_device=on)
        errors = {}
        for name, e in zip(A.BANK_TYPES, r["errors"]):
            if e["count"]:
                errors[name] = {"count": e["count"], "first": e["first_row"], "worst": e["worst_row"], "last": e["last_row"]}
                if name == "wrong-total":
                    errors[name].update(lowest=e["lowest_row"], highest=e["highest_row"])
                else:
                    assert (e["lowest_row"], e["highest_row"]) == (-1, -1)
            else:
                assert (e["first_row"], e["last_row"], e["worst_row"], e["lowest_row"], e["highest_row"]) == (-1,) * 5
        m = {"valid?": r["valid"] == A.VALID, "read-count": r["read_count"], "error-count": r["error_count"],
             "first-error": None if r["first_error_row"] < 0 else r["first_error_row"], "errors": errors}
        assert r["entries"] == int(np.asarray(case.cols.value2)[bank.is_read(case.cols)].sum())
        return {"valid": r["valid"], "cause": r["cause"], "reads": plain(r["reads"]), "n_reads": r["n_reads"],
                "map": None if r["valid"] == A.UNKNOWN else m}

    def dims(self, case):
        f = self.full(case)
        return dict(Entry.dims(self, case), n_aux=len(case.cols.aux), errors=f["map"]["error-count"] if f["map"] else 0)


# -- long-fork ----------------------------------------------------------------------
class LongFork(Entry):
    name = "long-fork"
    paths = (1, 2)
    capped = ("forks",)

    def build(self):
        t = [Case("n0", LF.encode([]), n=2)]
        for name, (n, h, _) in long_fork_cases.CASES.items():
            if name not in long_fork_cases.HOST_ONLY:
                t.append(Case(name, LF.encode(h), n=n))
        edge = synth.long_fork_history(n_ops=A.LF_TILE // 2 + 8, n=2, forks=2, seed=2)
        t.append(Case("n1", head(edge, 1), n=2))
        t += [Case(f"T{d:+d}", head(edge, A.LF_TILE + d), n=2) for d in (-1, 0, 1)]
        n = A.LF_TILE + 19                       # ops of two rows each: two tiles and an odd remainder
        return {"targets": t, "dirty": Case("dirty", synth.long_fork_history(n_ops=n, n=3, forks=400, seed=3), n=3),
                "clean": Case("clean", synth.long_fork_history(n_ops=n, n=3, forks=0, seed=4), n=3)}

    def ref(self, case, path):
        w = long_fork_ref.ref_cols(case.cols, case.n)
        assert w["rc"] == A.JH_OK, (case.name, w["rc"])
        early = w["cause"] == A.CAUSE_MULTIPLE_WRITES or w["illegal_kind"] == 1 or w["reads_count"] == 0
        return dict({k: w[k] for k in long_fork_ref.RAW_FIELDS}, forks=plain(w["forks"]), path=0 if early else path)

    def run(self, ctx, case, path, caps, dev):
        cols, on = _dev(dev, case.cols)
        r = ctx.check_long_fork(cols, case.n, path, fork_cap=caps["forks"], on_device=on)
        return dict({k: r[k] for k in long_fork_ref.RAW_FIELDS}, forks=plain(r["forks"]), path=r["path"])

    def dims(self, case):
        return dict(Entry.dims(self, case), n_aux=len(case.cols.aux), reads=self.full(case, 1)["reads_count"])


# -- causal-reverse -----------------------------------------------------------------
class CausalReverse(Entry):
    name = "causal-reverse"
    paths = (A.CR_PATH_LDS, A.CR_PATH_GLOBAL)
    capped = ("errors", "missing")

    def build(self):
        t = []
        for name, h in causal_reverse_cases.CASES.items():
            cols = CR.encode(h)
            if causal_reverse_ref.ref_cols(cols)["rc"] == A.JH_OK:
                t.append(Case("n0" if cols.n == 0 else name, cols))
        if not any(c.name == "n0" for c in t):
            t.insert(0, Case("n0", CR.encode([])))
        edge = synth.causal_reverse_history(n_keys=5, ops_per_key=SCAN_TILE // 10 + 4, violations=2, seed=2)
        assert edge.n > A.CR_TILE + 1
        t.append(Case("n1", head(edge, 1)))
        t += [Case(f"T{d:+d}", head(edge, A.CR_TILE + d)) for d in (-1, 0, 1)]
        K = 16
        per = (2 * A.CR_TILE + 37) // (2 * K) + 1
        return {"targets": t, "dirty": Case("dirty", synth.causal_reverse_history(n_keys=K, ops_per_key=per, violations=400, seed=3)),
                "clean": Case("clean", synth.causal_reverse_history(n_keys=K, ops_per_key=per, violations=0, seed=4))}

    def ref(self, case, path):
        w = causal_reverse_ref.ref_cols(case.cols, path)
        assert w["rc"] == A.JH_OK, (case.name, w["rc"])
        return plain({k: w[k] for k in causal_reverse_ref.RAW_FIELDS + ("key_valid", "errors", "missing")})

    def run(self, ctx, case, path, caps, dev):
        cols, on = _dev(dev, case.cols)
        r = ctx.check_causal_reverse(cols, path, caps["errors"], caps["missing"], on_device=on)
        return plain({k: r[k] for k in causal_reverse_ref.RAW_FIELDS + ("key_valid", "errors", "missing")})

    def dims(self, case):
        return dict(Entry.dims(self, case), n_aux=len(case.cols.aux), n_keys=int(case.cols.n_keys),
                    reads=self.full(case, 1)["read_count"])


# -- cycle: jh_scc and jh_check_cycle -------------------------------------------------
def cycle_paths(n, edges):
    reg = CY.regions(n, sorted(edges))
    big = len(reg) and int((reg[:, 1] - reg[:, 0] + 1).max()) > A.CY_LDS_VERTICES
    return (A.CY_PATH_AUTO, A.CY_PATH_GLOBAL) if big else (A.CY_PATH_AUTO, A.CY_PATH_LDS, A.CY_PATH_GLOBAL)


class Scc(Entry):
    name = "scc"
    paths = (A.CY_PATH_AUTO, A.CY_PATH_LDS, A.CY_PATH_GLOBAL)
    capped = ("sccs",)
    error_dims = ("scc_vertices",)
    on_device = False

    def build(self):
        t = [Case("n0", n=0, edges=()), Case("n1", n=1, edges=()), Case("n1-loop", n=1, edges=((0, 0),))]
        t += [Case(name, n=n, edges=tuple(e)) for name, (n, e) in cycle_cases.GRAPHS.items()]
        t.append(Case("ring-N-1", n=cycle_cases.N - 1, edges=tuple(cycle_cases.ring(cycle_cases.N - 1))))
        n = 2 * cycle_cases.N + 37
        # dirty: every vertex in a ring of 3 .. 40 vertices, the rings linked forward; clean: forward edges only
        dirty, at, k = [], 0, 0
        while at < n:
            size = min(3 + k % 38, n - at)
            if n - at - size in (1, 2):
                size = n - at
            dirty += cycle_cases.ring(size, at) + ([(at - 1, at)] if at else [])
            at, k = at + size, k + 1
        clean = [(i, j) for i in range(n) for j in (i + 1, i + 7, i + 300) if j < n]
        return {"targets": t, "dirty": Case("dirty", n=n, edges=tuple(dirty)), "clean": Case("clean", n=n, edges=tuple(clean))}

    def paths_of(self, case):
        return cycle_paths(case.n, case.edges)

    def ref(self, case, path):
        w = cycle_ref.scc_answer(case.n, list(case.edges))
        reg = CY.regions(case.n, list(case.edges))
        size = (reg[:, 1] - reg[:, 0] + 1) if len(reg) else np.zeros(0, np.int64)
        glob = len(reg) if path == A.CY_PATH_GLOBAL else int((size > A.CY_LDS_VERTICES).sum())
        return dict(w, edge_count=[0, 0, 0, len(case.edges)], regions=len(reg), max_region=int(size.max()) if len(reg) else 0,
                    global_regions=glob, path=0 if not len(reg) else 2 if glob else 1)

    def run(self, ctx, case, path, caps, dev):
        src, dst = [a for a, _ in case.edges], [b for _, b in case.edges]
        r = ctx.scc(case.n, src, dst, path, scc_cap=caps["sccs"])
        out = {k: r[k] for k in ("valid", "scc_count", "scc_vertices", "back_edges", "edge_count", "regions", "max_region",
                                 "global_regions", "path", "sccs")}
        return dict(out, labels=plain(r["labels"]))

    def dims(self, case):
        f = self.full(case)
        return {"rows": case.n, "edges": len(case.edges), "sccs": f["scc_count"], "scc_vertices": f["scc_vertices"]}


class Cycle(Entry):
    """jh_check_cycle with the process, realtime and wr analyzers."""
    name = "cycle"
    paths = (A.CY_PATH_AUTO, A.CY_PATH_LDS, A.CY_PATH_GLOBAL)
    capped = ("sccs", "edges")
    mask = A.CY_PROCESS | A.CY_REALTIME | A.CY_WR
    error_dims = ("scc_vertices",)
    edge_fields = ()

    def case(self, name, ops):
        return Case(name, CY.encode(ops, txns=True), ops=ops)

    def synth_case(self, name, **kw):
        cols = synth.txn_cycle_history(**kw)
        return Case(name, cols, ops=synth.txn_cycle_columns_to_ops(cols))

    def build(self):
        t = [self.case("n0", []), self.case("n1", [cycle_cases.inv(0)]),
             self.case("healthy", cycle_cases.random_history(3, 4, 60, txns=True)),
             self.case("cycles", cycle_cases.random_history(4, 4, 60, txns=True, healthy=False))]
        t += [self.case(name, h) for name, (h, an, _, _, _) in cycle_cases.UNKNOWN_CASES.items()]
        N = cycle_cases.N
        for d in (-1, 0, 1):
            c = self.synth_case(f"T{d:+d}", n_ops=(N + d) // 2, anomalies=2, seed=20 + d)
            if (N + d) % 2:
                c = self.case(c.name, c.ops + [dict(NEM)])
            assert c.cols.n == N + d
            t.append(c)
        n = N + 19
        return {"targets": t, "dirty": self.synth_case("dirty", n_ops=n, anomalies=300, seed=3),
                "clean": self.synth_case("clean", n_ops=n, anomalies=0, seed=4)}

    def reference(self, case):
        return cycle_ref.ref_check(case.ops, self.mask)

    def paths_of(self, case):
        w = self.reference_cached(case)
        return self.paths if "edges" not in w else cycle_paths(len(case.ops), w["edges"])

    @functools.lru_cache(maxsize=None)
    def reference_cached(self, case):
        return self.reference(case)

    def ref(self, case, path):
        w = dict(self.reference_cached(case))
        w.pop("map", None)
        if "edges" not in w:                     # :unknown: the cause and what it names, nothing else
            if w["cause"] in (A.CAUSE_DOUBLE_INVOKE, A.CAUSE_ORPHAN, A.CAUSE_UNMATCHED_INVOKE):
                w.pop("entries", None)           # the pairing fails before the txns are read
            return dict(w, labels=[-1] * len(case.ops), sccs=[], scc_count=0, edges=[])
        w.pop("back_edges", None)
        edges = w.pop("edges")
        return dict(w, unknown_key=None, unknown_value=None, edges=sorted(map(list, edges)), n_edges=sum(w["edge_count"]),
                    back_edges=None)

    def run(self, ctx, case, path, caps, dev):
        cols, on = _dev(dev, case.cols)
        r = ctx.check_cycle(cols, self.mask, path, None, scc_cap=caps["sccs"], rows_cap=max(len(case.ops), 1),
                            edge_cap=caps["edges"], on_device=on)
        keys = getattr(case.cols, "keys", None) or []
        out = {"valid": r["valid"], "cause": r["cause"], "unknown_row": r["unknown_row"], "unknown_rows": r["unknown_rows"],
               "unknown_key": keys[r["unknown_key"]] if r["unknown_key"] != A.NIL else None,
               "unknown_value": None if r["unknown_value"] == A.NIL else r["unknown_value"],
               "labels": plain(r["labels"]), "sccs": r["sccs"], "scc_count": r["scc_count"]}
        for k in self.edge_fields:
            out[k] = r[k]
        if r["valid"] == A.UNKNOWN:
            return dict(out, edges=[])
        edges = plain(r["edges"])
        assert r["back_edges"] == sum(1 for a, b in edges if b < a)
        # the builders may emit one edge more than once: as a set, and the number emitted
        return dict(out, scc_vertices=r["scc_vertices"], edge_count=r["edge_count"], n_edges=len(edges), back_edges=None,
                    edges=sorted(map(list, set(map(tuple, edges)))))

    def cut(self, full, caps):
        return dict(full, sccs=full["sccs"][:caps["sccs"]])           # edges come in no order: never cut (caps >= their number)

    def lists(self, full):
        return {"sccs": len(full["sccs"]), "edges": full.get("n_edges", 0)}

    def dims(self, case):
        f = self.full(case)
        return dict(Entry.dims(self, case), n_aux=len(case.cols.aux) if case.cols.aux is not None else 0,
                    scc_vertices=f.get("scc_vertices", 0))


class CycleAppend(Cycle):
    """jh_check_cycle with the list-append builder (and realtime)."""
    name = "cycle-append"
    mask = A.CY_APPEND | A.CY_REALTIME
    edge_fields = ("entries",)

    def case(self, name, ops):
        return Case(name, CY.encode_append(ops), ops=ops)

    def synth_case(self, name, **kw):
        cols = synth.append_history(**kw)
        return Case(name, cols, ops=synth.append_columns_to_ops(cols))

    def build(self):
        import cycle_append_cases as AC
        t = [self.case("n0", []), self.case("n1", [AC.ok(AC.ap("x", 1))]),
             self.case("healthy", AC.random_append_history(3, 40)), self.case("stale", AC.random_append_history(4, 40, stale=0.4)),
             self.case("long-read", [o for op in AC.long_read_history(257, [0, 1, 63, 64, 65]) for o in (
                 dict(op, type="invoke", value=[[f, k, None if f == "r" else v] for f, k, v in op["value"]]), op)])]
        N = cycle_cases.N
        for d in (-1, 0, 1):
            c = self.synth_case(f"T{d:+d}", n_txns=(N + d) // 2, anomalies=2, keys=20, seed=20 + d)
            if (N + d) % 2:
                c = self.case(c.name, c.ops + [dict(NEM)])
            assert c.cols.n == N + d
            t.append(c)
        # one anomalous schedule makes one SCC of nearly every txn: the dirty primer is many short stale
        # histories over keys of their own, one after the other (the realtime edges between them point forward)
        dirty, b = [], 0
        while len(dirty) < 2 * N + 37:
            for op in AC.random_append_history(100 + b, 40, stale=0.5):
                v = op.get("value")
                dirty.append(dict(op, value=[[f, 1000 * b + k, x] for f, k, x in v]) if v else dict(op))
            b += 1
        return {"targets": t, "dirty": self.case("dirty", dirty),
                "clean": self.synth_case("clean", n_txns=len(dirty) // 2, anomalies=0, seed=4)}

    def reference(self, case):
        return cycle_append_ref.ref_check_append(case.ops, self.mask)


class CycleMono(Cycle):
    """jh_check_cycle with the monotonic-key builder (and process)."""
    name = "cycle-mono"
    mask = A.CY_MONOTONIC | A.CY_PROCESS
    edge_fields = ("entries",)

    def case(self, name, ops):
        return Case(name, CY.encode_map(ops), ops=ops)

    def synth_case(self, name, **kw):
        cols = synth.monotonic_history(**kw)
        return Case(name, cols, ops=synth.monotonic_columns_to_ops(cols))

    def build(self):
        import cycle_mono_cases as MC
        t = [self.case("n0", []), self.case("n1", [MC.ok({"x": 1})]),
             self.case("healthy", MC.random_mono_history(3, 40)), self.case("stale", MC.random_mono_history(4, 60, stale=0.4)),
             self.case("chain", MC.chain(70))]
        N = cycle_cases.N
        for d in (-1, 0, 1):
            c = self.synth_case(f"T{d:+d}", n_ops=(N + d) // 2, stale=0.01, seed=20 + d)
            if (N + d) % 2:
                c = self.case(c.name, c.ops + [dict(NEM)])
            assert c.cols.n == N + d
            t.append(c)
        n = N + 19
        return {"targets": t, "dirty": self.synth_case("dirty", n_ops=n, keys=8, stale=0.3, seed=3),
                "clean": self.synth_case("clean", n_ops=n, keys=8, stale=0.0, seed=4)}

    def reference(self, case):
        return cycle_mono_ref.ref_check_mono(case.ops, self.mask)

    def ref(self, case, path):
        w = Cycle.ref(self, case, path)
        w.pop("unknown_rows", None)              # the monotonic builder names no pair of rows
        return w

    def run(self, ctx, case, path, caps, dev):
        r = Cycle.run(self, ctx, case, path, caps, dev)
        r.pop("unknown_rows", None)
        return r


# -- causal -------------------------------------------------------------------------
class Causal(Entry):
    name = "causal"
    error_dims = ("events",)

    def build(self):
        t = [Case("n0", CM.encode([]))]
        for name, h in causal_cases.CASES.items():
            if name in causal_cases.HOST_ONLY or not h:
                continue
            cols = CM.encode(h)
            if causal_ref.ref_cols(cols)["rc"] == A.JH_OK:
                t.append(Case(name, cols))
        edge = synth.causal_history(n_keys=A.CM_TILE // 4, violations=3, seed=2)
        oks = np.cumsum(np.asarray(edge.type) == A.TYPE_OK)
        assert oks[-1] > A.CM_TILE + 1
        t.append(Case("n1", head(edge, 1, aux_per_row=2)))
        for d in (-1, 0, 1):                     # T :ok rows: the sorted slots of the judge kernel
            k = int(np.searchsorted(oks, A.CM_TILE + d)) + 1
            t.append(Case(f"T{d:+d}", head(edge, k, aux_per_row=2)))
        K = (2 * A.CM_FLAG_TILE + 37) // 10 + 1
        return {"targets": t, "dirty": Case("dirty", synth.causal_history(n_keys=K, violations=K, seed=3)),
                "clean": Case("clean", synth.causal_history(n_keys=K, violations=0, seed=4))}

    def ref(self, case, path):
        w = causal_ref.ref_cols(case.cols)
        assert w["rc"] == A.JH_OK, (case.name, w["rc"])
        return plain({k: w[k] for k in causal_ref.RAW_FIELDS + ("keys",)})

    def run(self, ctx, case, path, caps, dev):
        cols, on = _dev(dev, case.cols)
        r = ctx.check_causal(cols, on_device=on)
        return plain({k: r[k] for k in causal_ref.RAW_FIELDS + ("keys",)})

    def dims(self, case):
        f = self.full(case)
        return {"rows": int(case.cols.n), "n_keys": int(case.cols.n_keys), "ok_rows": f["ok_count"],
                "events": f["invalid_keys"] + f["unknown_keys"]}


# -- adya g2 ------------------------------------------------------------------------
def g2_columns(typ, key, n_keys):
    n = len(typ)
    z = np.zeros(n, np.int64)
    return H.Columns(n=n, process=z.copy(), type=np.asarray(typ, np.int64), f=np.full(n, A.F_INSERT, np.int64),
                     key=np.asarray(key, np.int64), value=z, value2=z.copy(), n_keys=n_keys, aux=np.zeros(1, np.int64),
                     keys=list(range(n_keys)))


class G2(Entry):
    name = "g2"
    capped = ("illegal",)

    def build(self):
        T = A.G2_TILE
        t = [Case("n0" if not h else name, adya.encode(h)) for name, h in g2_cases.CASES.items() if name != "no-inserts"]
        t.append(Case("n1", g2_columns([A.TYPE_OK], [0], 1)))
        for d in (-1, 0, 1):                     # K keys inserted once, the first and the last twice
            K = T + d
            t.append(Case(f"T{d:+d}", g2_columns(np.full(K + 2, A.TYPE_OK), np.concatenate([np.arange(K), [0, K - 1]]), K)))
        t.append(Case("T+1-legal", g2_columns(np.full(T + 1, A.TYPE_OK), np.arange(T + 1), T + 1)))
        K = 2 * T + 37
        rng = np.random.default_rng(5)
        twice = rng.permutation(np.concatenate([np.arange(K), np.arange(K), np.arange(0, K, 3)]))
        once = np.concatenate([rng.permutation(K), rng.permutation(K), np.arange(0, K, 3)])
        typ = np.full(len(once), A.TYPE_OK, np.int64)
        typ[K:] = A.TYPE_FAIL                    # the second and third insert of a key fail
        return {"targets": t, "dirty": Case("dirty", g2_columns(np.full(len(twice), A.TYPE_OK), twice, K)),
                "clean": Case("clean", g2_columns(typ, once, K))}

    def ref(self, case, path):
        w = g2_ref.ref_cols(case.cols)
        assert w["rc"] == A.JH_OK, (case.name, w["rc"])
        return plain({k: w[k] for k in g2_ref.RAW_FIELDS + ("illegal",)})

    def run(self, ctx, case, path, caps, dev):
        cols, on = _dev(dev, case.cols)
        r = ctx.check_g2(cols, caps["illegal"], on_device=on)
        return plain({k: r[k] for k in g2_ref.RAW_FIELDS + ("illegal",)})

    def dims(self, case):
        f = self.full(case)
        return dict(Entry.dims(self, case), n_keys=int(case.cols.n_keys), inserts=f["insert_rows"])


# -- perf ---------------------------------------------------------------------------
class Perf(Entry):
    """jh_perf has no verdict: a history whose invokes all pair counts as
    valid, one with unpaired invokes as invalid."""
    name = "perf"
    capped = perf_ref.LISTS
    clean_only = ("groups",)    # the quantiles need every invoke paired
    F_COUNT = 24

    def build(self):
        t = [Case("n0", P.encode_rows([]), time=np.zeros(0, np.int64))]
        for name, h in perf_cases.CASES.items():
            if h:
                t.append(Case(name, P.encode_rows(h), time=P.time_column(h)))
        edge = synth.perf_history(n=A.PERF_TILE + 40, seed=2, nemesis_every=100)
        assert edge.n > A.PERF_TILE + 1
        t.append(Case("n1", head(edge, 1), time=edge.time[:1]))
        t += [Case(f"T{d:+d}", head(edge, A.PERF_TILE + d), time=edge.time[:A.PERF_TILE + d]) for d in (-1, 0, 1)]
        n = 8 * A.PERF_TILE + 37
        fs = tuple(f"f{i}" for i in range(8))
        dirty = synth.perf_history(n=n, procs=40, fs=fs, seed=3, dangling=True, p_info=0.2, nemesis_every=50, mean_latency_ms=900.0,
                                   mean_think_ms=200.0)
        dirty = head(dirty, dirty.n - dirty.n % 2 - 1)
        dirty.time = synth.perf_history(n=n, procs=40, fs=fs, seed=3, dangling=True, p_info=0.2, nemesis_every=50,
                                        mean_latency_ms=900.0, mean_think_ms=200.0).time[:dirty.n]
        clean = synth.perf_history(n=n, procs=40, fs=fs, seed=4, mean_latency_ms=900.0, mean_think_ms=200.0)
        return {"targets": t, "dirty": Case("dirty", dirty, time=dirty.time), "clean": Case("clean", clean, time=clean.time)}

    def f_count(self, case):
        return max(self.F_COUNT, A.F_FIRST_INTERNED + len(getattr(case.cols, "f_names", None) or []))

    def ref(self, case, path):
        w = perf_ref.ref_cols(case.cols, case.time, f_count=self.f_count(case))
        assert w["rc"] == A.JH_OK, (case.name, w["rc"])
        return plain({k: w[k] for k in perf_ref.SCALARS + perf_ref.LISTS})

    def valid(self, full):
        return full["n_unpaired_invokes"] == 0

    def run(self, ctx, case, path, caps, dev):
        cols, on = _dev(dev, case.cols)
        time = dev[1] if on else np.asarray(case.time, np.int64)
        r = ctx.perf(cols, time, on_device=on, f_count=self.f_count(case), pair_cap=caps["pair"], pt_cap=caps["pt_row"],
                     series_cap=caps["series"], group_cap=caps["groups"], cell_cap=caps["cells"])
        return plain({k: r[k] for k in perf_ref.SCALARS + perf_ref.LISTS})

    def dims(self, case):
        f = self.full(case)
        return dict(Entry.dims(self, case), invokes=f["n_invokes"])


# the entry points in the order of include/jh.h
ENTRIES = [Counter(), Set(), SetBitmaps(), SetFull(), TotalQueue(), Queue(), UniqueIds(), Bank(), LongFork(), CausalReverse(),
           Scc(), Cycle(), CycleAppend(), CycleMono(), Causal(), G2(), Perf()]
BY_NAME = {e.name: e for e in ENTRIES}
NAMES = list(BY_NAME)
# what each passes to stage_history as (need_key, need_aux) (jh_api.hip); None: no history
STAGES = {"counter": (False, False), "set": (False, True), "set-bitmaps": (False, True), "set-full": (False, True),
          "total-queue": (False, True), "queue": (False, False), "unique-ids": (False, False), "bank": (False, True),
          "long-fork": (False, True), "causal-reverse": (True, True), "scc": None, "cycle": (False, True),
          "cycle-append": (False, True), "cycle-mono": (False, True), "causal": (True, True), "g2": (True, False),
          "perf": (False, False)}


def chain(reverse):
    """[(entry, case)]: every entry point once, in the order of include/jh.h
    (or reversed), large and small inputs alternating from a large one: the
    dirty primers forward, the clean ones backward, and between them the
    T + 1 target (the largest small one)."""
    order = ENTRIES[::-1] if reverse else ENTRIES
    out = []
    for i, e in enumerate(order):
        c = e.cases()
        if i % 2 == 0:
            out.append((e, c["clean" if reverse else "dirty"]))
        else:
            out.append((e, next(t for t in c["targets"] if t.name in ("T+1", "ring-N+1"))))
    return out


# The chain gives few checkers a large neighbour that staged a column they do not stage themselves: HANDOFFS
# names, for each such checker, the large calls it is also run directly after (keyed histories, long aux)
KEYED, AUXED = ("causal-reverse", "causal", "g2"), ("bank", "causal-reverse")
HANDOFFS = {name: tuple(dict.fromkeys((() if st[0] else KEYED) + (() if st[1] else AUXED)))
            for name, st in STAGES.items() if st is not None and not all(st)}
