"""Hand-written histories for checker/perf with the plot data worked out by
hand from jepsen/src/jepsen/checker/perf.clj. EXPECT[name][plot] lists the
series as (title, pointtype, data), without the nemesis legend series; a value
that is an exception class is what latency-graph raises after the raw plot."""
import json
import os

S = 10 ** 9
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "perf_reference_cases.json")


def reference_cases():
    with open(GOLD) as fh:
        return json.load(fh)


def op(p, t, f, time, **kw):
    return dict({"process": p, "type": t, "f": f, "time": time}, **kw)


def nem(f, time):
    return [op("nemesis", "info", f, time), op("nemesis", "info", f, time)]


def zeros(titles_pt, xs=(5,)):
    return [(t, pt, [[x, 0] for x in xs]) for t, pt in titles_pt]


CASES, EXPECT = {}, {}

# Two processes, two f. read: 1 s -> 3 s :ok (2000 ms). write: 2 s -> 11 s :fail
# (9000 ms) and 12 s -> 12.5 s :info (500 ms). t-max 12.5 s: the only rate bucket
# is 5 (15 > 12.5), so the completions at 11 s and 12.5 s are dropped. The write
# quantile group (bucket 15) is sorted [500 9000]: floor(2 q) = 1 for every q.
CASES["basic"] = [op(0, "invoke", "read", 1 * S), op(1, "invoke", "write", 2 * S), op(0, "ok", "read", 3 * S),
                  op(1, "fail", "write", 11 * S), op(0, "invoke", "write", 12 * S), op(0, "info", "write", 12 * S + S // 2)]
EXPECT["basic"] = {
    "latency-raw": [(":read ok", 4, [[1.0, 2000.0]]), (":write info", 6, [[12.0, 500.0]]), (":write fail", 6, [[2.0, 9000.0]])],
    "latency-quantiles": [(":read " + q, 4, [[15, 2000.0]]) for q in ("0.5", "0.95", "0.99", "1")]
    + [(":write " + q, 6, [[15, 9000.0]]) for q in ("0.5", "0.95", "0.99", "1")],
    "rate": [(":read ok", 4, [[5, 0.1]]), (":read info", 4, [[5, 0]]), (":read fail", 4, [[5, 0]])]
    + zeros([(":write ok", 6), (":write info", 6), (":write fail", 6)]),
}

# Process 0 invokes twice (the first invoke stays unpaired), process 1 completes
# without an invoke, the nemesis "invokes" and completes (a pair: 1000 ms, f :kill
# sorts first), process :other (a keyword) completes: no client op, not in the rate.
# An unpaired invoke: the raw plot is built, the quantiles throw.
CASES["unpaired"] = [op(0, "invoke", "read", 1 * S), op("nemesis", "invoke", "kill", 2 * S), op(0, "invoke", "read", 3 * S),
                     op(1, "ok", "write", 4 * S), op("nemesis", "info", "kill", 3 * S), op(0, "ok", "read", 5 * S),
                     op("other", "ok", "read", 6 * S)]
EXPECT["unpaired"] = {
    "latency-raw": [(":kill info", 4, [[2.0, 1000.0]]), (":read ok", 6, [[3.0, 2000.0]])],
    "latency-quantiles": TypeError,
    "rate": [(":read ok", 4, [[5, 0.1]]), (":read info", 4, [[5, 0]]), (":read fail", 4, [[5, 0]]),
             (":write ok", 6, [[5, 0.1]]), (":write info", 6, [[5, 0]]), (":write fail", 6, [[5, 0]])],
}

# A completion stamped before its invoke: the latency -1.5 ms is data. Three ops
# of one f in two quantile buckets (0 -> 15, 1 -> 45); rate buckets 5 .. 35 with
# two :ok in the first one: 0.1 + 0.1.
CASES["negative"] = [op(0, "invoke", "add", 2 * S), op(0, "ok", "add", 2 * S - 1500000), op(0, "invoke", "add", 3 * S),
                     op(0, "ok", "add", 4 * S), op(0, "invoke", "add", 31 * S), op(0, "fail", "add", 36 * S)]
EXPECT["negative"] = {
    "latency-raw": [(":add ok", 4, [[2.0, -1.5], [3.0, 1000.0]]), (":add fail", 4, [[31.0, 5000.0]])],
    "latency-quantiles": [(":add " + q, 4, [[15, 1000.0], [45, 5000.0]]) for q in ("0.5", "0.95", "0.99", "1")],
    "rate": [(":add ok", 4, [[5, 0.1 + 0.1], [15, 0], [25, 0], [35, 0]]), (":add info", 4, [[5, 0], [15, 0], [25, 0], [35, 0]]),
             (":add fail", 4, [[5, 0], [15, 0], [25, 0], [35, 0.1]])],
}

# f names of mixed types: polysort puts nil first, then keywords, then longs
# (ClassCastException -> the class names, clojure.lang.Keyword < java.lang.Long).
# Every op runs from 1 s to 6 s: a history that ends before 5 s has no rate bucket
# at all and fails (assert (seq data)).
CASES["mixed-f"] = [op(0, "invoke", 7, 1 * S), op(0, "ok", 7, 6 * S), op(1, "invoke", "b", 1 * S), op(1, "ok", "b", 6 * S),
                    op(2, "invoke", None, 1 * S), op(2, "ok", None, 6 * S), op(3, "invoke", 3, 1 * S), op(3, "ok", 3, 6 * S),
                    op(4, "invoke", "a", 1 * S), op(4, "ok", "a", 6 * S)]
EXPECT["mixed-f"] = {
    "latency-raw": [(t + " ok", pt, [[1.0, 5000.0]]) for t, pt in (("nil", 4), (":a", 6), (":b", 8), ("3", 10), ("7", 12))],
    "latency-quantiles": [(t + " " + q, pt, [[15, 5000.0]]) for t, pt in (("nil", 4), (":a", 6), (":b", 8), ("3", 10), ("7", 12))
                          for q in ("0.5", "0.95", "0.99", "1")],
    "rate": [(t + " " + ty, pt, [[5, 0.1 if ty == "ok" else 0]]) for t, pt in (("nil", 4), (":a", 6), (":b", 8), ("3", 10), ("7", 12))
             for ty in ("ok", "info", "fail")],
}

# Nemesis :start / :stop pairs next to one client op: the legend series and the
# preamble's regions are checked in the tests; the data is the client op's.
CASES["nemesis"] = nem("start", 1 * S) + [op(0, "invoke", "read", 2 * S), op(0, "ok", "read", 3 * S)] + nem("stop", 4 * S) \
    + nem("start", 5 * S)
EXPECT["nemesis"] = {
    "latency-raw": [(":read ok", 4, [[2.0, 1000.0]])],
    "latency-quantiles": [(":read " + q, 4, [[15, 1000.0]]) for q in ("0.5", "0.95", "0.99", "1")],
    "rate": [(":read ok", 4, [[5, 0.1]]), (":read info", 4, [[5, 0]]), (":read fail", 4, [[5, 0]])],
}


def series_of(plot):
    """(title, pointtype, data) of the plot's series but the nemesis legend's."""
    return [(s["title"], s["pointtype"], [list(p) for p in s["data"]]) for s in plot["series"] if "pointtype" in s]
