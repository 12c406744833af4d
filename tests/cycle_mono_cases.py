"""Hand-written group shapes and the seeded generator of increment-workload
histories shared by the monotonic-key tests."""
import random

NEM = {"process": "nemesis", "type": "info", "f": "start", "value": None}


def row(t, value, p=0, f="read"):
    return {"process": p, "type": t, "f": f, "value": value}


def ok(value, p=0):
    return row("ok", value, p)


def groups(*sizes, key="x", first=0):
    """:ok rows of one key: sizes[j] rows hold the value first + j, the values
    dealt out round-robin so that the groups interleave in row order."""
    left, h = list(sizes), []
    while any(left):
        for j in range(len(left)):
            if left[j]:
                left[j] -= 1
                h.append(ok({key: first + j}, p=j))
    return h


def chain(length, key="x"):
    return [ok({key: v}, p=v % 7) for v in range(length)]


def interleaved_chains(n_rows, seed=0):
    """The shape of the reference's big-history-gen: an invoke and a completion
    of a random type per value, keys [:x], [:y] and [:x :y] with chains that
    interleave; the value rises with the row, so it is valid."""
    rng = random.Random(seed)
    h = []
    for v in range(n_rows // 2):
        p, k = rng.randrange(100), rng.choice([("x",), ("y",), ("x", "y")])
        t = rng.choice(["ok"] * 5 + ["fail", "info", "info"])
        f = rng.choice(["inc", "read"])
        h += [row("invoke", {k: v}, p, f), row(t, {k: v}, p, f)]
    return h


def random_mono_history(seed, n_ops=40, n_procs=4, n_keys=3, stale=0.0, p_info=0.05, nemesis=True):
    """The increment workload under a schedule that is serial at invocation time:
    :inc k returns {k new}, :read the current value of a random non-empty subset
    of the keys (stale: with that probability one of its keys, of value > 0, one
    behind). Every invoke is completed; an :info completion carries nil."""
    rng = random.Random(seed)
    h, open_, cur, done = [], {}, {k: 0 for k in range(n_keys)}, 0
    while done < n_ops or open_:
        if nemesis and rng.random() < 0.03:
            h.append(dict(NEM))
            continue
        p = rng.randrange(n_procs)
        if p in open_:
            f, value = open_.pop(p)
            t = "info" if rng.random() < p_info else "ok"
            h.append(row(t, value if t == "ok" else None, p, f))
        elif done < n_ops:
            if rng.random() < 0.5:
                k = rng.randrange(n_keys)
                cur[k] += 1
                f, value = "inc", {k: cur[k]}
            else:
                ks = [k for k in range(n_keys) if rng.random() < 0.5] or [rng.randrange(n_keys)]
                f, value = "read", {k: cur[k] for k in ks}
                behind = [k for k in ks if value[k] > 0]
                if stale and behind and rng.random() < stale:
                    value[rng.choice(behind)] -= 1
            open_[p] = (f, value)
            h.append(row("invoke", None, p, f))
            done += 1
    return h


def seeded(seed):
    """The seeded history of the closed-form tests: even seeds healthy, odd ones stale."""
    rng = random.Random(7000 + seed)
    return random_mono_history(seed, rng.randint(1, 60), rng.randint(1, 5), rng.randint(1, 4), stale=0.3 if seed % 2 else 0.0)
