"""jepsen.checker.perf on MI355X: the latency and rate plots of
(checker/latency-graph), (checker/rate-graph) and (checker/perf).

Mirrors jepsen/src/jepsen/checker/perf.clj and util.clj:606-687 (names,
argument meaning, the plot maps). The product of these checkers is the plot:
the map handed to `plot!` -- "series" (each with "title", "with", "linetype",
"pointtype", "data"), "xrange", "yrange", "logscale", "draw-fewer-on-top?" and
"preamble" (a list of commands, each a list of tokens).

Two paths build the same maps. The host path runs the literal transcriptions
below over op maps. The device path (`device_reduction` and the `*_from_device`
builders) takes the integer outputs of jh_perf (include/jh.h) and assembles the
maps from them; it is taken when the history is `Columns`, or encodes to them
with an integer :time on every op, and falls back on JH_EUNSUPPORTED.

Conventions: an op is a dict with the reference's keyword names as strings
("process", "type", "f", "time"); a Python str f stands for a keyword, so
util/name+ (which, as written, always returns pr-str) gives ":read". Tokens: a
plain str is a bare gnuplot word (a Clojure keyword or symbol), `Q` a quoted
string, `GList` a comma-separated (g/list ...), `GRange` a (g/range a b), a
nested list a space-separated group. Where Clojure yields a ratio this module
yields a `fractions.Fraction`: (bucket-time 5 1) is 5/2.
"""
import decimal
import logging
import math
import shutil
import subprocess
from fractions import Fraction

import numpy as np

from . import _abi as A
from . import history as H
from . import report

log = logging.getLogger(__name__)

DEFAULT_NEMESIS_COLOR = "#cccccc"
NEMESIS_ALPHA = 0.6
TYPES = ["ok", "info", "fail"]                              # perf.clj:173-175
QS = [0.5, 0.95, 0.99, 1]                                   # perf.clj:506; 1 is the integer, as written
ALL = "::all"                                               # perf/rate's ::all key
MAX_EXACT_LATENCY = 1 << 53                                 # the device path's bound on |latency| (latency_ms)


class Q(str):
    """A quoted gnuplot string (a Clojure string among the tokens)."""
    __slots__ = ()


TYPE_COLOR = {"ok": ["rgb", Q("#81BFFC")], "info": ["rgb", Q("#FFA400")], "fail": ["rgb", Q("#FF1E90")]}


class GList(tuple):
    """(g/list a b ...): comma-separated."""
    __slots__ = ()


class GRange(tuple):
    """(g/range a b): [a:b]."""
    __slots__ = ()


# ---------------------------------------------------------------------------
# Clojure arithmetic
def _norm(x):
    return int(x) if isinstance(x, Fraction) and x.denominator == 1 else x


def _div(a, b):
    """(/ a b): a ratio (or a long) for two integers, a double otherwise."""
    if H._is_int(a) and H._is_int(b) or isinstance(a, Fraction) or isinstance(b, Fraction):
        if isinstance(a, float) or isinstance(b, float):
            return float(a) / float(b)
        return _norm(Fraction(a) / Fraction(b))
    return a / b


def _long(x):
    """(long x): truncation toward zero."""
    return int(x) if not isinstance(x, Fraction) else int(math.trunc(x))


def ratio_double(x):
    """(double x). A long converts exactly rounded; a ratio goes through
    Ratio.doubleValue: the BigDecimal quotient at MathContext/DECIMAL64 (16
    significant decimal digits, half-even), then BigDecimal.doubleValue."""
    if isinstance(x, Fraction):
        if x.denominator == 1:
            return float(x.numerator)
        ctx = decimal.Context(prec=16, rounding=decimal.ROUND_HALF_EVEN)
        return float(ctx.divide(decimal.Decimal(x.numerator), decimal.Decimal(x.denominator)))
    return float(x)


def nanos_to_ms(nanos):
    return _div(nanos, 1000000)                             # util.clj:272


def nanos_to_secs(nanos):
    return nanos / 1e9                                      # util.clj:276: a double


def math_round(x):
    """Math/round of a double: floor(x + 1/2), half up."""
    return int(math.floor(x + 0.5))


def _compare(a, b):
    """clojure.core/compare where it is defined; TypeError for ClassCastException."""
    if a is None or b is None:
        return 0 if a is b else (-1 if a is None else 1)
    num = lambda v: isinstance(v, (int, float, Fraction)) and not isinstance(v, bool)   # noqa: E731
    if num(a) and num(b):
        return (a > b) - (a < b)
    if type(a) is not type(b) or isinstance(a, (dict, set, frozenset)):
        raise TypeError("ClassCastException")
    return (a > b) - (a < b)


def _class_name(x):
    """(str (class x)) for the values an :f takes here."""
    if isinstance(x, bool):
        return "class java.lang.Boolean"
    if isinstance(x, Q):
        return "class java.lang.String"
    if isinstance(x, str):
        return "class clojure.lang.Keyword"
    if H._is_int(x):
        return "class java.lang.Long"
    if isinstance(x, float):
        return "class java.lang.Double"
    if x is None:
        return ""
    if isinstance(x, (list, tuple)):
        return "class clojure.lang.PersistentVector"
    return "class " + type(x).__name__


def poly_compare(a, b):
    """util.clj:524-529."""
    try:
        return _compare(a, b)
    except TypeError:
        ca, cb = _class_name(a), _class_name(b)
        return (ca > cb) - (ca < cb)


def polysort(coll):
    """util.clj:531-534."""
    import functools
    return sorted(coll, key=functools.cmp_to_key(poly_compare))


def name_plus(x):
    """util.clj:46-51. The `if` has no else branch and its value is dropped:
    as written the function always returns (pr-str x)."""
    if isinstance(x, Q):
        return '"' + str(x) + '"'
    if isinstance(x, bool):
        return "true" if x else "false"
    if x is None:
        return "nil"
    if isinstance(x, str):
        return ":" + x
    return str(x)


def _name(t):
    return str(t)                                           # (name :ok)


# ---------------------------------------------------------------------------
# util.clj
def history_to_latencies(history):
    """util.clj:606-640: every paired invocation gains "latency" and
    "completion", its completion "latency"."""
    out, invokes = [], {}
    for op in history:
        if op.get("type") == "invoke":
            out.append(op)
            invokes[op.get("process")] = len(out) - 1
        elif op.get("process") in invokes:
            i = invokes.pop(op.get("process"))
            invoke = out[i]
            lat = op["time"] - invoke["time"]
            op = dict(op, latency=lat)
            out[i] = dict(invoke, latency=lat, completion=op)
            out.append(op)
        else:
            out.append(op)
    return out


def nemesis_intervals(history, opts=None):
    """util.clj:642-687."""
    opts = opts or {}
    start = opts["start"] if opts.get("start") is not None else {"start"}
    stop = opts["stop"] if opts.get("stop") is not None else {"stop"}
    ops = [op for op in history if op.get("process") == "nemesis"]
    pairs = [(ops[i], ops[i + 1]) for i in range(0, len(ops) - 1, 2)]
    intervals, starts = [], []
    for a, b in pairs:
        if a.get("f") != b.get("f"):
            continue
        f = a.get("f")
        if f in start:
            starts.append((a, b))
        elif f in stop:
            for s1, s2 in starts:
                intervals += [[s1, a], [s2, b]]
            starts = []
    for s1, s2 in starts:
        intervals += [[s1, None], [s2, None]]
    return intervals


# ---------------------------------------------------------------------------
# perf.clj
def bucket_scale(dt, b):
    return _norm(_long(b) * dt + _div(dt, 2))


def bucket_time(dt, t):
    return bucket_scale(dt, _div(t, dt))


def buckets(dt, tmax=None):
    """The bounded arity: the midpoints <= tmax. (The unbounded one is lazy and
    infinite; it is a generator here.)"""
    if tmax is None:
        def gen():
            i = 0
            while True:
                yield bucket_scale(dt, i)
                i += 1
        return gen()
    out, i = [], 0
    while tmax >= bucket_scale(dt, i):
        out.append(bucket_scale(dt, i))
        i += 1
    return out


def bucket_points(dt, points):
    groups = {}
    for p in points:
        groups.setdefault(bucket_time(dt, p[0]), []).append(p)
    return {k: groups[k] for k in sorted(groups)}


def quantiles(qs, points):
    s = sorted(points)
    if not s:
        return None
    n = len(s)
    return {q: s[min(n - 1, int(math.floor(n * q)))] for q in qs}


def latencies_to_quantiles(dt, qs, points):
    num = lambda v: isinstance(v, (int, float, Fraction)) and not isinstance(v, bool)   # noqa: E731
    assert num(dt)
    assert all(num(q) for q in qs)
    assert all(0 <= q <= 1 for q in qs)
    bs = [[bt, quantiles(qs, [p[1] for p in pts])] for bt, pts in bucket_points(dt, points).items()]
    return {q: [[t, m.get(q)] for t, m in bs] for q in qs}


def _invoke(op):
    return op.get("type") == "invoke"


def invokes_by_type(ops):
    ct = lambda o: (o.get("completion") or {}).get("type")   # noqa: E731
    return {"ok": [o for o in ops if ct(o) == "ok"], "fail": [o for o in ops if ct(o) == "fail"],
            "info": [o for o in ops if ct(o) == "info"]}


def _group_by(fn, coll):
    m = {}
    for x in coll:
        m.setdefault(fn(x), []).append(x)
    return m


def invokes_by_f(history):
    return _group_by(lambda o: o.get("f"), [o for o in history if _invoke(o)])


def invokes_by_f_type(history):
    return {f: invokes_by_type(ops) for f, ops in invokes_by_f(history).items()}


def completions_by_f_type(history):
    by_f = _group_by(lambda o: o.get("f"), [o for o in history if not _invoke(o)])
    return {f: _group_by(lambda o: o.get("type"), ops) for f, ops in by_f.items()}


def rate(history):
    m = {}
    for op in history:
        if _invoke(op):
            continue
        f, t = op.get("f"), op.get("type")
        for a, b in ((f, t), (f, ALL), (ALL, t), (ALL, ALL)):
            d = m.setdefault(a, {})
            d[b] = d.get(b, 0) + 1
    return m


def latency_point(op):
    """[time (s), latency (ms)], both doubles. An op without a :latency throws
    (a NullPointerException in the reference, a TypeError here)."""
    if op.get("latency") is None:
        raise TypeError(f"latency-point: no :latency in {op!r} (NullPointerException)")
    return [float(nanos_to_secs(op["time"])), ratio_double(nanos_to_ms(op["latency"]))]


def fs_to_points(fs):
    return {f: 2 * (2 + i) for i, f in enumerate(fs)}


def qs_to_colors(qs):
    colors = ["red", "orange", "purple", "blue", "green", "grey"]
    return {q: ["rgb", Q(colors[i % len(colors)])] for i, q in enumerate(sorted(qs, reverse=True))}


def nemesis_ops(nemeses, history):
    nemeses = list(nemeses or [])
    assert all(n.get("name") for n in nemeses)
    names = [n["name"] for n in nemeses]
    assert list(dict.fromkeys(names)) == names
    index = {}
    for n in nemeses:
        fs = list(n["start"] if n.get("start") is not None else ["start"]) + \
            list(n["stop"] if n.get("stop") is not None else ["stop"]) + list(n.get("fs") or [])
        for f in fs:
            index[f] = n["name"]
    by = _group_by(lambda o: index.get(o.get("f")), [o for o in history if o.get("process") == "nemesis"])
    out = [dict(n, ops=by[n["name"]]) for n in nemeses if by.get(n["name"])]
    if by.get(None):
        out = [{"name": "nemesis", "ops": by[None]}] + out   # conj on a seq: at the front
    return out


def nemesis_activity(nemeses, history):
    return [dict(n, intervals=nemesis_intervals(n["ops"], n)) for n in nemesis_ops(nemeses, history)]


def interval_to_times(plot, interval):
    a, b = interval
    return [float(nanos_to_secs(a["time"])),
            float(nanos_to_secs(b["time"])) if b else plot["xrange"][1]]


def nemesis_regions(plot, nemeses):
    out = []
    for i, n in enumerate(nemeses):
        color = n.get("fill-color") or n.get("color") or DEFAULT_NEMESIS_COLOR
        transparency = n.get("transparency", NEMESIS_ALPHA)
        height, padding = 0.0834, 0.00615
        bot = 1 - height * (i + 1)
        top = bot + height
        for start, stop in (interval_to_times(plot, iv) for iv in n["intervals"]):
            out.append(["set", "obj", "rect", "from", GList((start, ["graph", bot + padding])),
                        "to", GList((stop, ["graph", top - padding])), "fillcolor", "rgb", Q(color),
                        "fillstyle", "transparent", "solid", transparency, "noborder"])
    return out


def nemesis_lines(plot, nemeses):
    xr = plot.get("xrange")
    keep = (lambda t: xr[0] <= t <= xr[1]) if xr else (lambda t: True)
    out = []
    for n in nemeses:
        color = n.get("line-color") or n.get("color") or DEFAULT_NEMESIS_COLOR
        width = n.get("line-width", Q("1"))
        for t in (float(nanos_to_secs(o["time"])) for o in n["ops"]):
            if keep(t):
                out.append(["set", "arrow", "from", GList((t, ["graph", 0])), "to", GList((t, ["graph", 1])),
                            "lc", "rgb", Q(color), "lw", width, "nohead"])
    return out


def nemesis_series(plot, nemeses):
    return [{"title": n["name"], "with": "lines",
             "linecolor": ["rgb", Q(n.get("fill-color") or n.get("color") or DEFAULT_NEMESIS_COLOR)],
             "linewidth": 6, "data": [[-1, -1]]} for n in nemeses]


def with_nemeses(plot, history, nemeses):
    act = nemesis_activity(nemeses, history)
    plot = dict(plot)
    plot["series"] = list(plot.get("series") or []) + nemesis_series(plot, act)
    plot["preamble"] = list(plot.get("preamble") or []) + nemesis_regions(plot, act) + nemesis_lines(plot, act)
    return plot


def preamble(output_path):
    return [["set", "output", Q(output_path)],
            ["set", "term", "png", "truecolor", "size", GList((900, 400))],
            ["set", "xlabel", Q("Time (s)")],
            ["set", "key", "outside", "top", "right"]]


def latency_preamble(test, output_path):
    return preamble(output_path) + [["set", "title", Q(_test_name(test) + " latency")],
                                    ["set", "ylabel", Q("Latency (ms)")], ["set", "logscale", "y"]]


def rate_preamble(test, output_path):
    return preamble(output_path) + [["set", "title", Q(_test_name(test) + " rate")],
                                    ["set", "ylabel", Q("Throughput (hz)")]]


def _test_name(test):
    n = test.get("name") if isinstance(test, dict) else None
    return "" if n is None else str(n)                      # (str nil) is ""


def _mod(a, b):
    """clojure.core/mod: the sign of the divisor (Python's %)."""
    return a % b


def broaden_range(r):
    """perf.clj:334-357. Math/round is half up, not Python's round; Math/log10
    and Math/pow are the C library's here. There is no JVM on hand to pin the
    last bit of Math/pow against, so xrange and yrange are held to this
    transcription only."""
    a, b = r
    if a == b:
        return [a - 1, a + 1]
    size = abs(b - a)
    grid = _div(size, 10)
    scale = math.pow(10, math_round(math.log10(float(grid))))
    a2 = a - _mod(a, scale)
    m = _mod(b, scale)
    b2 = b if m / scale < 0.001 else scale + (b - _mod(b, scale))
    return [min(a, a2), max(b, b2)]


def with_range(plot):
    data = [p for s in plot["series"] for p in s["data"]]
    assert data, "Assert failed: (seq data)"
    xs, ys = [p[0] for p in data], [p[1] for p in data]
    xmin, xmax, ymin, ymax = min(xs), max(xs), min(ys), max(ys)
    xrange = broaden_range([xmin, xmax])
    yrange = [ymin, ymax] if plot.get("logscale") == "y" else broaden_range([ymin, ymax])
    plot = dict(plot)
    plot["xrange"] = plot["xrange"] if plot.get("xrange") is not None else xrange
    plot["yrange"] = plot["yrange"] if plot.get("yrange") is not None else yrange
    return plot


def legend_part(series):
    part = [Q("-"), "with", series.get("with")]
    for k in ("linetype", "linecolor", "pointtype", "linewidth"):
        if series.get(k) is not None:
            part.append([k, series[k]])
    part.append(["title", Q(series["title"])] if series.get("title") is not None else "notitle")
    return [x for x in part if x is not None]


# ---------------------------------------------------------------------------
# plot!: the gnuplot script, commands in the order perf.clj:404-469 emits them
def _fmt(x):
    if isinstance(x, Q):
        return '"' + str(x).replace("\\", "\\\\").replace('"', '\\"') + '"'
    if isinstance(x, GRange):
        return "[" + _fmt(x[0]) + ":" + _fmt(x[1]) + "]"
    if isinstance(x, GList):
        return ",".join(_fmt(y) for y in x)
    if isinstance(x, (list, tuple)):
        return " ".join(_fmt(y) for y in x)
    if isinstance(x, Fraction):
        return repr(ratio_double(x))
    return str(x)


def plot_commands(opts):
    """(commands, datasets) of plot!, after the draw-fewer-on-top? rewrite."""
    series = list(opts["series"])
    empty = [s for s in series if not s.get("data")]
    assert not empty, "Assert failed: Series has no :data points\n" + repr(empty)
    if opts.get("draw-fewer-on-top?"):
        # sort-by is stable, then reverse: most points first, ties in reverse order
        big = [{k: v for k, v in s.items() if k != "title"}
               for s in reversed(sorted(series, key=lambda s: len(s["data"])))]
        return plot_commands(dict(opts, series=big + [dict(s, data=[[0, -1]]) for s in series],
                                  **{"draw-fewer-on-top?": False}))
    cmds = list(opts.get("preamble") or [])
    if opts.get("logscale"):
        cmds.append(["set", "logscale", opts["logscale"]])
    if opts.get("xrange"):
        cmds.append(["set", "xrange", GRange(opts["xrange"])])
    if opts.get("yrange"):
        cmds.append(["set", "yrange", GRange(opts["yrange"])])
    cmds.append(["plot", GList(legend_part(s) for s in series)])
    return cmds, [s["data"] for s in series]


def plot_script(opts):
    """The script: one command per line, then every dataset inline, each closed
    by a line "e" (gnuplot's '-' data)."""
    cmds, data = plot_commands(opts)
    lines = [_fmt(c) for c in cmds]
    for d in data:
        lines += [" ".join(_fmt(v) for v in p) for p in d]
        lines.append("e")
    return "\n".join(lines) + "\n"


def plot(test, plot_map, opts, name):
    """plot! with its side effects: with a store dir, writes <name>.gp (the
    script) next to the reference's <name>.png and runs gnuplot when there is
    one. A missing gnuplot is logged, not raised (the reference throws
    IllegalStateException): a stated deviation."""
    png = report.store_path(test, (opts or {}).get("subdirectory"), name + ".png")
    if png is None:
        plot_commands(plot_map)                             # plot!'s asserts hold with or without a store dir
        return None
    script = plot_script(plot_map)
    path = png[:-4] + ".gp"
    with open(path, "w") as fh:
        fh.write(script)
    exe = shutil.which("gnuplot")
    if exe is None:
        log.warning("gnuplot is not installed: wrote %s, no %s", path, png)
        return path
    try:
        subprocess.run([exe, path], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    except (OSError, subprocess.CalledProcessError) as e:
        log.warning("gnuplot failed on %s: %s", path, e)
    return path


# ---------------------------------------------------------------------------
# the plot maps, host path (perf.clj:471-584)
def _nemeses(test, opts):
    return (opts or {}).get("nemeses") or ((test or {}).get("plot") or {}).get("nemeses")


def _out(test, opts, name):
    """store/path! of the plot's .png (it makes the directories); the bare
    file name for a test without a store dir."""
    return report.store_path(test, (opts or {}).get("subdirectory"), name + ".png") or name + ".png"


def point_graph(test, history, opts=None):
    history = history_to_latencies(history)
    datasets = invokes_by_f_type(history)
    fs = polysort(datasets.keys())
    pts = fs_to_points(fs)
    series = []
    for f in fs:
        for t in TYPES:
            data = datasets[f].get(t)
            if data:
                series.append({"title": name_plus(f) + " " + _name(t), "with": "points", "linetype": TYPE_COLOR[t],
                               "pointtype": pts[f], "data": [latency_point(o) for o in data]})
    p = {"preamble": latency_preamble(test, _out(test, opts, "latency-raw")), "draw-fewer-on-top?": True, "logscale": "y",
         "series": series}
    return with_nemeses(with_range(p), history, _nemeses(test, opts))


def quantiles_graph(test, history, opts=None):
    history = history_to_latencies(history)
    dt = A.PERF_DT_QUANTILES
    datasets = {f: latencies_to_quantiles(dt, QS, [latency_point(o) for o in ops])
                for f, ops in invokes_by_f(history).items()}
    fs = polysort(datasets.keys())
    pts, colors = fs_to_points(fs), qs_to_colors(QS)
    series = [{"title": name_plus(f) + " " + str(q), "with": "linespoints", "linetype": colors[q],
               "pointtype": pts[f], "data": datasets[f][q]} for f in fs for q in QS]
    p = {"preamble": latency_preamble(test, _out(test, opts, "latency-quantiles")), "series": series, "logscale": "y"}
    return with_nemeses(with_range(p), history, _nemeses(test, opts))


def rate_graph(test, history, opts=None):
    history = list(history)
    dt = A.PERF_DT_RATE
    td = ratio_double(_div(1, dt))
    t_max = nanos_to_secs(max([0] + [o["time"] for o in history]))
    datasets = {}
    for op in history:
        if _invoke(op) or not H._is_int(op.get("process")):
            continue
        m = datasets.setdefault(op.get("f"), {}).setdefault(op.get("type"), {})
        b = bucket_time(dt, nanos_to_secs(op["time"]))
        m[b] = td + (m.get(b) or 0)
    fs = polysort(datasets.keys())
    pts = fs_to_points(fs)
    bs = buckets(dt, t_max)
    series = [{"title": name_plus(f) + " " + _name(t), "with": "linespoints", "linetype": TYPE_COLOR[t],
               "pointtype": pts[f], "data": [[b, datasets[f].get(t, {}).get(b, 0)] for b in bs]}
              for f in fs for t in TYPES]
    p = {"preamble": rate_preamble(test, _out(test, opts, "rate")), "series": series}
    return with_nemeses(with_range(p), history, _nemeses(test, opts))


# ---------------------------------------------------------------------------
# the device path
class Reduction:
    """The outputs of one jh_perf call with what the assembly needs beside
    them: the time column, the f names by code, the f codes that have an
    invoke (paired or not: the reference's datasets, and so its point types,
    cover them all) and the nemesis ops."""

    def __init__(self, raw, time, f_of_code, invoke_fs, nemesis_history):
        self.raw, self.time, self.f_of_code, self.invoke_fs = raw, time, f_of_code, invoke_fs
        self.nemesis_history = nemesis_history


def time_column(ops):
    """The :time column of op maps, or None when an op has no integer :time
    (the device path is then not taken)."""
    t = np.empty(len(ops), np.int64)
    for i, o in enumerate(ops):
        v = o.get("time")
        if not H._is_int(v) or not -(1 << 63) < v < (1 << 63):
            return None
        t[i] = v
    return t


def f_names(cols):
    inv = {v: k for k, v in H.KNOWN_F.items()}
    names = {c: n for c, n in inv.items()}
    for i, n in enumerate(cols.f_names or []):
        names[A.F_FIRST_INTERNED + i] = n
    return names


def nemesis_rows(cols, time, names):
    """The :nemesis ops of a columnar history as op maps (process, type, f,
    time): all that with-nemeses reads."""
    rows = np.nonzero(np.asarray(cols.process)[:cols.n] == -1)[0]
    return [{"process": "nemesis", "type": H.TYPE_NAMES[int(cols.type[r])], "f": names.get(int(cols.f[r]), int(cols.f[r])),
             "time": int(time[r]), "index": int(r)} for r in rows.tolist()]


def encode_rows(ops):
    """Op maps -> Columns with the three columns jh_perf reads (process, type,
    f: history.encode's codes); key, value and value2 are not read and are
    zeros. None when a process is a negative integer: the reference's rate plot
    counts it (integer?), the device's process >= 0 would not."""
    n = len(ops)
    proc, typ, fcol = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.int64)
    other, f_ids, names = {"nemesis": -1}, {}, []
    for i, op in enumerate(ops):
        p = op.get("process")
        if H._is_int(p):
            if p < 0:
                return None
            proc[i] = int(p)
        else:
            if p not in other:
                other[p] = -1 - len(other)
            proc[i] = other[p]
        t = op.get("type")
        if t not in H.TYPES:
            raise ValueError(f"unknown :type {t!r} in op {op!r}")
        typ[i] = H.TYPES[t]
        f = op.get("f")
        if isinstance(f, str) and not isinstance(f, Q) and f in H.KNOWN_F:
            fcol[i] = H.KNOWN_F[f]
        else:
            k = (type(f).__name__, f)
            if k not in f_ids:
                f_ids[k] = A.F_FIRST_INTERNED + len(names)
                names.append(f)
            fcol[i] = f_ids[k]
    z = np.zeros(n, np.int64)
    return H.Columns(n=n, process=proc, type=typ, f=fcol, key=z, value=z, value2=z, n_keys=0, aux=np.zeros(1, np.int64),
                     f_names=names)


def device_reduction(ctx, history, want=A.PERF_ALL):
    """jh_perf over `history` (Columns with a `time` attribute, or op maps).
    None when the device path does not apply: a :time that is no integer or
    lies outside [0, 2^53) (latency_ms is exact below that), an f that cannot
    be interned, JH_EUNSUPPORTED from the library."""
    from . import _native
    if isinstance(history, H.Columns):
        cols, time = history, getattr(history, "time", None)
        if time is None:
            raise ValueError("perf needs the :time of every op: set cols.time")
        time = np.asarray(time, np.int64)
    else:
        ops = list(history)
        time = time_column(ops)
        if time is None:
            return None
        try:
            cols = encode_rows(ops)
        except TypeError:                                   # an unhashable :f
            return None
        if cols is None:
            return None
    if cols.n and (time.min() < 0 or time.max() >= MAX_EXACT_LATENCY):
        return None
    try:
        raw = ctx.perf(cols, time, want=want)
    except _native.JhError as e:
        if e.code != A.JH_EUNSUPPORTED:
            raise
        return None
    names = f_names(cols)
    invoke_fs = set(raw["series"][:, 0].tolist())
    if raw["n_unpaired_invokes"]:
        lone = (np.asarray(cols.type)[:cols.n] == A.TYPE_INVOKE) & (raw["pair"] < 0)
        invoke_fs |= set(np.unique(np.asarray(cols.f)[:cols.n][lone]).tolist())
    return Reduction(raw, time, names, invoke_fs, nemesis_rows(cols, time, names))


def _secs(t):
    return np.asarray(t, np.int64).astype(np.float64) / 1e9     # int64 -> double, one division


def latency_ms(lat):
    """(double (/ latency 1000000)) for |latency| < 2^53: the decimal quotient
    has at most 16 significant digits there, so Ratio.doubleValue is the
    correctly rounded quotient, which is numpy's."""
    return np.asarray(lat, np.int64).astype(np.float64) / 1e6


def point_graph_from_device(test, red, opts=None):
    raw, time = red.raw, red.time
    pair, rows = raw["pair"], raw["pt_row"]
    x = _secs(time[rows]).tolist()
    y = latency_ms(time[pair[rows]] - time[rows]).tolist()
    blocks, at = {}, 0
    for f, t, c in raw["series"].tolist():
        blocks[(red.f_of_code.get(f, f), H.TYPE_NAMES[t])] = (at, at + c)
        at += c
    fs = polysort({red.f_of_code.get(c, c) for c in red.invoke_fs})
    pts = fs_to_points(fs)
    series = []
    for f in fs:
        for t in TYPES:
            if (f, t) in blocks:
                a, b = blocks[(f, t)]
                series.append({"title": name_plus(f) + " " + _name(t), "with": "points", "linetype": TYPE_COLOR[t],
                               "pointtype": pts[f], "data": [list(p) for p in zip(x[a:b], y[a:b])]})
    p = {"preamble": latency_preamble(test, _out(test, opts, "latency-raw")), "draw-fewer-on-top?": True, "logscale": "y",
         "series": series}
    return with_nemeses(with_range(p), red.nemesis_history, _nemeses(test, opts))


def quantiles_graph_from_device(test, red, opts=None):
    raw = red.raw
    dt = A.PERF_DT_QUANTILES
    datasets = {}
    for rec in raw["groups"].tolist():
        f = red.f_of_code.get(rec[0], rec[0])
        mid = bucket_scale(dt, rec[1])
        d = datasets.setdefault(f, {q: [] for q in QS})
        for q, lat in zip(QS, latency_ms(rec[3:7]).tolist()):
            d[q].append([mid, lat])
    fs = polysort(datasets.keys())
    pts, colors = fs_to_points(fs), qs_to_colors(QS)
    series = [{"title": name_plus(f) + " " + str(q), "with": "linespoints", "linetype": colors[q],
               "pointtype": pts[f], "data": datasets[f][q]} for f in fs for q in QS]
    p = {"preamble": latency_preamble(test, _out(test, opts, "latency-quantiles")), "series": series, "logscale": "y"}
    return with_nemeses(with_range(p), red.nemesis_history, _nemeses(test, opts))


def rate_graph_from_device(test, red, opts=None):
    raw = red.raw
    dt = A.PERF_DT_RATE
    td = ratio_double(_div(1, dt))
    cells = raw["cells"]
    cmax = int(cells[:, 3].max()) if len(cells) else 0
    # (+ td (or % 0)) once per op: the c-th partial sum of td, added in order
    run = np.add.accumulate(np.full(cmax, td)) if cmax else np.zeros(0)
    datasets = {}
    for f, t, b, c in cells.tolist():
        datasets.setdefault(red.f_of_code.get(f, f), {}).setdefault(H.TYPE_NAMES[t], {})[bucket_scale(dt, b)] = float(run[c - 1])
    fs = polysort(datasets.keys())
    pts = fs_to_points(fs)
    bs = buckets(dt, nanos_to_secs(int(raw["t_max"])))
    series = [{"title": name_plus(f) + " " + _name(t), "with": "linespoints", "linetype": TYPE_COLOR[t],
               "pointtype": pts[f], "data": [[b, datasets[f].get(t, {}).get(b, 0)] for b in bs]}
              for f in fs for t in TYPES]
    p = {"preamble": rate_preamble(test, _out(test, opts, "rate")), "series": series}
    return with_nemeses(with_range(p), red.nemesis_history, _nemeses(test, opts))
