"""Seeded random list-append histories (valid / stale-prefix / mutated) and the
hand-written edge shapes shared by the list-append tests."""
import random

from jepsen_amd import _abi as A

NEM = {"process": "nemesis", "type": "info", "f": "start", "value": None}


def row(t, *mops, p=0):
    return {"process": p, "type": t, "f": "txn", "value": [list(m) for m in mops]}


def ok(*mops, p=0):
    return row("ok", *mops, p=p)


def r(k, v):
    return ["r", k, v]


def ap(k, v):
    return ["append", k, v]


def appends_of(k, values, t="ok", per_row=1):
    """Rows of type t appending `values` to k, per_row micro-ops a row."""
    values = list(values)
    return [row(t, *[ap(k, v) for v in values[i:i + per_row]]) for i in range(0, len(values), per_row)]


def random_append_history(seed, n_txns, n_procs=4, n_keys=3, stale=0.0, nemesis=True, max_len=12):
    """Txns of 1-4 micro-ops under a serial schedule at completion time: an
    append takes a fresh value of its key, a read returns the key's list (stale:
    with that probability a random prefix of it, which gives rw cycles). Invokes
    carry the txn with nil reads; :fail completions apply nothing; an :info
    completion applies its appends half the time. A key whose list reaches
    max_len is left for a fresh one."""
    rng = random.Random(seed)
    h, open_, state, counter, alias = [], {}, {}, {}, {k: k for k in range(n_keys)}
    fresh = [n_keys]

    def complete(p):
        txn = open_.pop(p)
        t = rng.choice(["ok"] * 5 + ["fail", "info"])
        applies = t == "ok" or (t == "info" and rng.random() < 0.5)
        out, mine = [], {}
        for f, k, v in txn:
            if f == "append":
                out.append([f, k, v])
                if applies:
                    mine.setdefault(k, []).append(v)
            elif t == "fail":
                out.append([f, k, None])
            else:
                cur = state.get(k, []) + mine.get(k, [])
                if stale and rng.random() < stale and not mine.get(k):
                    cur = cur[:rng.randint(0, len(cur))]
                out.append([f, k, list(cur)])
        for k, vs in mine.items():
            state[k] = state.get(k, []) + vs
        h.append({"process": p, "type": t, "f": "txn", "value": out})

    done = 0
    while done < n_txns or open_:
        if nemesis and rng.random() < 0.03:
            h.append(dict(NEM))
            continue
        p = rng.randrange(n_procs)
        if p in open_:
            complete(p)
        elif done < n_txns:
            txn = []
            for _ in range(rng.randint(1, 4)):
                slot = rng.randrange(n_keys)
                if len(state.get(alias[slot], [])) >= max_len:
                    alias[slot] = fresh[0]
                    fresh[0] += 1
                k = alias[slot]
                if rng.random() < 0.5:
                    counter[k] = counter.get(k, 0) + 1
                    txn.append(["append", k, counter[k]])
                else:
                    txn.append(["r", k, None])
            open_[p] = txn
            h.append({"process": p, "type": "invoke", "f": "txn", "value": [list(m) for m in txn]})
            done += 1
    return h


def mutate(h, seed):
    """One or two mutations that aim at causes 13-16 (whether one fires depends
    on the history; the tests ask the transcription)."""
    rng = random.Random(seed)
    h = [dict(op, value=[list(m) for m in op["value"]]) if op.get("value") else dict(op) for op in h]
    for _ in range(rng.randint(1, 2)):
        kind = rng.choice(["dup-append", "dup-element", "order", "fail-writer"])
        rows = [i for i, op in enumerate(h) if op.get("process") != "nemesis" and op.get("value")]
        if not rows:
            return h
        if kind == "dup-append":
            src = [(i, m) for i in rows if h[i]["type"] == "invoke" for m in h[i]["value"] if m[0] == "append"]
            if src:
                _, m = rng.choice(src)
                h[rng.choice([i for i in rows if h[i]["type"] == "invoke"])]["value"].append(list(m))
        elif kind == "dup-element":
            src = [(i, j) for i in rows for j, m in enumerate(h[i]["value"]) if m[0] == "r" and m[2]]
            if src:
                i, j = rng.choice(src)
                v = h[i]["value"][j][2]
                v.insert(rng.randint(0, len(v)), rng.choice(v))
        elif kind == "order":
            src = [(i, j) for i in rows if h[i]["type"] in ("ok", "info") for j, m in enumerate(h[i]["value"]) if m[0] == "r" and m[2]]
            if src:
                i, j = rng.choice(src)
                v = h[i]["value"][j][2]
                v[rng.randrange(len(v))] = 10_000 + rng.randrange(5)
        else:
            src = [i for i in rows if h[i]["type"] == "ok" and any(m[0] == "append" for m in h[i]["value"])]
            if src:
                h[rng.choice(src)]["type"] = "fail"
    return h


def seeded(seed):
    """The seeded history of the closed-form tests: a third healthy, a third
    stale, a third mutated."""
    rng = random.Random(5000 + seed)
    h = random_append_history(seed, rng.randint(1, 40), rng.randint(1, 5), rng.randint(1, 4),
                              stale=0.5 if seed % 3 == 1 else 0.0, max_len=rng.choice([3, 12]))
    return mutate(h, seed) if seed % 3 == 2 else h


def long_read_history(longest, lengths):
    """One key with the list 1..longest, every element appended by an :ok row of
    its own (a reader between two appends of one row would be a cycle), one :ok read of the whole list and one of every length in `lengths`."""
    full = list(range(1, longest + 1))
    return appends_of("x", full) + [ok(r("x", full))] + [ok(r("x", full[:c])) for c in lengths]


def all_causes():
    """A history that holds causes 13, 14, 15 and 16 at once, as parts to leave out."""
    return {
        13: [row("invoke", ap("x", 1)), row("invoke", ap("x", 1))],
        14: [row("fail", r("y", [5, 6, 5]))],
        15: [ok(r("z", [1, 2])), ok(r("z", [1, 3]))],
        16: [ok(r("w", [9]))],
    }
