"""What a visibility scope (`Corpus.set_tags` / `set_scope`) costs per query: host-clock timing, from the call to the synchronised result on
the host, of `match_list_top(100)` and of the full `match_list` on the 10 M x 32-byte list with needle "deadbe" and on the paths-shaped list
(1.4 M, needle "linux"), ScoreThenIndexAsc:
    (1)  the corpus WITHOUT tags - the floor, and what every caller had before;
    (2)  tags present, scope (0, 0): must be (1) - a corpus without an active scope takes the launches it took before;
    (3a) scope active, every haystack visible; (3b) half of them; (3c) one in twenty - the drop pass (two launches) behind the scorers, which
         still score the hidden rows;
    (4b) / (4c) a second corpus uploaded from the visible haystacks alone (half, one in twenty) - what applying the scope AHEAD of the scorers
         could reach at best, at the price of a resident copy per scope;
    (5b) / (5c) what a caller does today: the full `match_list` of the whole list, a numpy mask over `index`, the cut.
The device-side variants (1)-(4) ALTERNATE query by query inside one process, in an order that rotates with the query (drift of a shared host
hits all alike, none always runs behind the same neighbour); (5) is timed in a loop of its own behind them - its milliseconds of host work
leave the device idle, and the query that follows such a gap was measured 15 % slower.  The tagged corpus serves (2), (3) and (5) with its
scope set outside the timed window (host only); every variant keeps its own reserved matcher.  `--repeats` repeats of `--queries` queries
per variant, call and list: the median of the repeats' medians and their spread (lowest and highest repeat median), microseconds, one JSON
line each.  Before anything is timed every scoped result is checked against (4)'s with the index map applied, and (5)'s against (3)'s.
`--baseline` times variant (1) alone and uses nothing a build without tags lacks: run it on the parent commit, twice, for the spread the
unscoped call shows between two runs.  `--only 3b --call top` is what a kernel trace is taken of.

    python tools/bench_scope.py [--queries 200] [--repeats 5] [--lists fixed10M,paths1.4M] [--baseline [--package-root DIR]] [--only VARIANT] [--call top|list]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --package-root DIR: import frizbee_amd from DIR - another build of the package, the parent commit's for --baseline
PKG = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1]) if "--package-root" in sys.argv[:-1] else ROOT
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import synth  # noqa: E402

import frizbee_amd as F  # noqa: E402

LIMIT = 100
NAMES = {"1": "(1) no tags", "2": "(2) tags, scope (0,0)", "3a": "(3a) scope active, all visible", "3b": "(3b) scope active, half visible", "3c": "(3c) scope active, 1 in 20 visible",
         "4b": "(4b) corpus of the visible half", "4c": "(4c) corpus of the visible 1 in 20", "5b": "(5b) full match_list + numpy mask, half", "5c": "(5c) full match_list + numpy mask, 1 in 20"}
# tags: bit 0 = outside the visible half, bit 1 = outside the visible one in twenty, bit 2 = nobody
SCOPES = {"2": (0, 0), "3a": (0, 4), "3b": (0, 1), "3c": (0, 2)}


def the_list(name):
    if name == "fixed10M":
        rows, ends = synth.fixed_corpus(b"deadbe", 10_000_000, 32)
        return rows.numpy().reshape(-1), ends, "deadbe", 32
    data, ends = synth.paths_corpus()
    return data, ends, "linux", 0


def sub_packed(data, ends, vis, row):
    """the visible haystacks alone, in their order, in the upload format"""
    if row:
        sub = data.reshape(-1, row)[vis].reshape(-1)
        return np.ascontiguousarray(sub), (np.arange(1, int(vis.sum()) + 1, dtype=np.uint64) * np.uint64(row))
    starts = np.concatenate([[0], ends[:-1]]).astype(np.int64)
    lens = (ends.astype(np.int64) - starts)[vis]
    keep = np.repeat(vis, ends.astype(np.int64) - starts)
    return np.ascontiguousarray(data[keep]), np.cumsum(lens).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=200, help="timed queries per repeat, variant, call and list")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lists", default="fixed10M,paths1.4M")
    ap.add_argument("--baseline", action="store_true", help="variant (1) alone, through calls a build without tags has")
    ap.add_argument("--only", choices=tuple(NAMES), default=None)
    ap.add_argument("--call", choices=("top", "list"), default=None)
    ap.add_argument("--package-root", default=ROOT, help="the directory frizbee_amd is imported from (read before the import)")
    a = ap.parse_args()
    variants = ["1"] if a.baseline else [v for v in NAMES if a.only in (None, v)]
    calls = [c for c in ("top", "list") if a.call in (None, c)]
    cfg = F.Config(pf_lanes=64, sw_lanes=64, sort=F.SortStrategy.ScoreThenIndexAsc)
    for name in a.lists.split(","):
        data, ends, needle, row = the_list(name)
        n = len(ends)
        rng = np.random.default_rng(7)
        tags = ((rng.random(n) < 0.5).astype(np.uint16)) | ((rng.random(n) >= 0.05).astype(np.uint16) << 1)
        vis = {"b": (tags & 1) == 0, "c": (tags & 2) == 0}
        corpora, run = {}, {}
        need = {"plain": {"1"}, "tagged": {"2", "3a", "3b", "3c", "5b", "5c"}, "sub_b": {"4b"}, "sub_c": {"4c"}}
        check = not a.baseline and a.only is None
        for key, users in need.items():
            if not (users & set(variants)) and not (check and key.startswith("sub")):
                continue
            if key.startswith("sub"):
                corpora[key] = F.Corpus(packed=sub_packed(data, ends, vis[key[-1]], row))
            else:
                corpora[key] = F.Corpus(packed=(data, ends))
                if key == "tagged":
                    corpora[key].set_tags(tags)
        # every variant keeps its own reserved matcher: a matcher copies its result speculatively at the previous result's size, so variants that
        # shared one would pay for each other's list lengths (a second copy and wait, 10 us, whenever the previous scope was a sparser one)
        where = {v: key for key, users in need.items() for v in users}
        for v in NAMES:
            if where[v] in corpora:
                run[v] = F.Matcher(needle, cfg)
                run[v].reserve(corpora[where[v]])

        def query(v, call, copy=False):
            m, cp = run[v], corpora[where[v]]
            if v[0] == "5":  # today's caller: the whole list over the link, the mask and the cut on the host
                r = m.match_list(cp, copy=False)
                r = r[vis[v[1]][r["index"]]]
                return (r[:LIMIT].copy(), len(r)) if call == "top" else r.copy()
            return m.match_list_top(cp, LIMIT, copy=copy) if call == "top" else m.match_list(cp, copy=copy)

        def prepare(v):  # outside the timed window: the toggle keystroke, host only
            if v in SCOPES:
                corpora["tagged"].set_scope(*SCOPES[v])
            elif v[0] == "5":
                corpora["tagged"].set_scope(0, 0)

        if check:  # the scoped results against the visible haystacks' own corpus (index map applied), today's host-side filter against the scoped call
            for s in ("b", "c"):
                at = np.flatnonzero(vis[s]).astype(np.uint32)
                prepare("3" + s)
                got_top, got_list = query("3" + s, "top", True), query("3" + s, "list", True)
                want_top, want_list = query("4" + s, "top", True), query("4" + s, "list", True)
                want_list["index"] = at[want_list["index"]]
                wt = want_top[0].copy()
                wt["index"] = at[wt["index"]]
                assert got_list.tolist() == want_list.tolist() and got_top[1] == want_top[1] and got_top[0].tolist() == wt.tolist(), (name, s)
                prepare("5" + s)
                host_top = query("5" + s, "top")
                assert host_top[1] == got_top[1] and host_top[0].tolist() == got_top[0].tolist(), (name, s, "host-side filter")
            prepare("3a")
            assert query("3a", "list", True).tolist() == query("1", "list", True).tolist(), (name, "all visible")
        for call in calls:
            for _ in range(max(a.warmup, 1)):
                for v in variants:
                    prepare(v)
                    query(v, call)
            medians = {v: [] for v in variants}
            found = {}
            groups = [[v for v in variants if v[0] != "5"], [v for v in variants if v[0] == "5"]]
            for group in [g for g in groups if g] * a.repeats:
                t = {v: [] for v in group}
                for q in range(a.queries):
                    for v in group[q % len(group):] + group[:q % len(group)]:
                        prepare(v)
                        t0 = time.perf_counter()
                        r = query(v, call)
                        t[v].append((time.perf_counter() - t0) * 1e6)
                        found[v] = int(r[1]) if call == "top" else len(r)
                for v in group:
                    medians[v].append(float(np.median(t[v])))
            for v in variants:
                r = medians[v]
                print(json.dumps(dict(list=name, items=n, needle=needle, call="match_list_top(100)" if call == "top" else "match_list", variant=NAMES[v], found=found[v],
                                      queries=a.queries * a.repeats, median_us=round(float(np.median(r)), 1), spread_us=[round(min(r), 1), round(max(r), 1)],
                                      repeat_medians_us=[round(x, 1) for x in r])), flush=True)
        del run, corpora


if __name__ == "__main__":
    main()
