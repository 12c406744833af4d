"""Round 8: what the reachable-set BFS spends its time on, from a per-key
timeline of a tuning build (JH_DEFER_TIMES=1 JH_TL_CSV=<file>, the last table
of the file: one per call).

    python tools/shape/bfs_pick_report.py <tl.csv> [key ...]

Prints, in ms after phase 2's begin (the first BFS or sequential start):
the invalid keys' BFS starts (min / median / max), the share of the BFS
workgroups' key time spent on keys the BFS did not settle (its run ended
after another engine's), the listed keys' rows, and the keys settled last."""
import csv
import statistics
import sys


def last_table(path):
    rows, cur = [], []
    for r in csv.reader(open(path)):
        if r and r[0] == "key":
            cur = []
            rows = cur
            continue
        cur.append(r)
    cols = "key,explored,valid,deferred_us,p1_inserts,p1_tmax,n_ok,bfs0,bfs1,seq0,seq1,help0,help1".split(",")
    return [dict(zip(cols, (float(x) for x in r))) for r in rows]


def main():
    t = last_table(sys.argv[1])
    want = [int(k) for k in sys.argv[2:]]
    begin = min(x for r in t for x in (r["bfs0"], r["seq0"]) if x > 0)

    def ms(x):
        return round((x - begin) / 1000.0, 2) if x > 0 else None

    def end(r):
        return max(r["bfs1"], r["seq1"], r["help1"])

    def settled_by_bfs(r):
        others = [x for x in (r["seq1"], r["help1"]) if x > 0]
        return r["bfs1"] > 0 and (not others or r["bfs1"] <= min(others))

    inv = [r for r in t if r["valid"] == 2]
    starts = sorted(ms(r["bfs0"]) for r in inv if r["bfs0"] > 0)
    print("deferred keys", len(t), "invalid", len(inv), "of which the BFS started", len(starts))
    print("invalid keys' BFS start, ms after phase 2 begins: min %.2f median %.2f max %.2f" %
          (starts[0], statistics.median(starts), starts[-1]))
    ran = [r for r in t if r["bfs0"] > 0 and r["bfs1"] > 0]
    tot = sum(r["bfs1"] - r["bfs0"] for r in ran)
    lost = sum(r["bfs1"] - r["bfs0"] for r in ran if not settled_by_bfs(r))
    print("BFS key runs %d, settled by the BFS %d; key time %.1f ms, %.1f ms (%.0f %%) on keys it did not settle" %
          (len(ran), sum(settled_by_bfs(r) for r in ran), tot / 1000, lost / 1000, 100 * lost / max(tot, 1)))
    helped = [r for r in t if r["help0"] > 0]
    print("helper mains ran %d keys, %d of them invalid" % (len(helped), sum(r["valid"] == 2 for r in helped)))
    print("phase 2 ends %.2f ms after its begin" % ms(max(end(r) for r in t)))
    print("key,explored,valid,bfs0,bfs1,seq0,seq1,help0,help1,settled")
    tail = sorted(t, key=end)[-8:]
    for r in [r for r in t if int(r["key"]) in want] + tail:
        print(",".join(str(x) for x in [int(r["key"]), int(r["explored"]), int(r["valid"]), ms(r["bfs0"]), ms(r["bfs1"]),
                                        ms(r["seq0"]), ms(r["seq1"]), ms(r["help0"]), ms(r["help1"]), ms(end(r))]))


if __name__ == "__main__":
    main()
