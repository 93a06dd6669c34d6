"""What the per-haystack score bias (`Corpus.set_bias`) costs and saves per keystroke: host-clock timing, from the call to the synchronised
result on the host, of the best `limit` records by score + bias on the first 200 000 paths of the paths-shaped list and on the whole list
(1.4 M), limit 100, the needles of a typed query (tools/bench_top_indices.py's) in turn:
    (a) `match_list_top` over the corpus WITHOUT a bias - the floor, and what every caller had before;
    (b) `match_list_top` with a bias of a few dozen (bias_hi 40): a needle keeps its single selection level and radix pass while
        max matrix score + exact bonus + 40 < 256 - with the default scoring (18 per row + 22) needles of up to 10 rows, against 12 unbiased;
    (c) `match_list_top` with a bias that crosses 256 (bias_hi 300: two selection levels and the second radix pass for every needle);
    (d) what a caller has to do without the device-side bias: the full IndexAsc `match_list`, numpy add + clip, stable argsort, cut.
(b) and (d) rank by the same biased score, (c) by its own; (a) is the same query unbiased.  The four ALTERNATE query by query inside one process (drift of
a shared host hits all alike): three corpora of the same list are resident side by side (no bias, small bias, large bias), every path keeps
its own reserved matcher, and the needle changes outside the timed window.  `--repeats` repeats of `--queries` queries per path and list:
the median of the repeats' medians and their spread (lowest and highest repeat median), microseconds, one JSON line per list and path.  Also
reported: the empty prompt over the biased corpus (`Matcher("").match_list_top`; on the device since tools/bench_prompt.py measures it).  Before anything is timed (b) and (c) are
each checked against the host-side ranking (d's code) with their own bias.

    python tools/bench_bias.py [--queries 300] [--repeats 5] [--only a|b|c|d] [--lists 200k,1.4M]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import synth  # noqa: E402

import frizbee_amd as F  # noqa: E402
from bench_top_indices import NEEDLES  # noqa: E402

LIMIT = 100
NAMES = {"a": "(a) unbiased top", "b": "(b) biased top, bias_hi 40", "c": "(c) biased top, bias_hi 300 (two levels)", "d": "(d) match_list + host add + argsort"}


def host_side(m, cp, bias):
    """(d): the whole list over the link, the boost and the ordering on the host"""
    r = m.match_list(cp, copy=False)
    s = np.clip(r["score"].astype(np.int32) + bias[r["index"]], 0, 65535)
    order = np.argsort(-s, kind="stable")[:LIMIT]
    out = r[order].copy()
    out["score"] = s[order]
    return out, len(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=300, help="timed queries per repeat, path and list")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3, help="untimed passes over the needles per path")
    ap.add_argument("--only", choices=tuple(NAMES), default=None, help="one path alone (what a kernel trace is taken of)")
    ap.add_argument("--lists", default="200k,1.4M")
    a = ap.parse_args()
    paths = [p for p in NAMES if a.only in (None, p)]
    data, ends = synth.paths_corpus()
    for name in a.lists.split(","):
        n = {"200k": 200_000, "1.4M": len(ends)}[name]
        packed = (data[: int(ends[n - 1])], ends[:n])
        rng = np.random.default_rng(7)
        small = rng.integers(-40, 41, n).astype(np.int16)  # frecency of a few dozen
        large = np.where(rng.random(n) < 0.02, 300, small).astype(np.int16)  # "file is open": across 256
        corpora = {"a": F.Corpus(packed=packed), "b": F.Corpus(packed=packed), "c": F.Corpus(packed=packed)}
        corpora["b"].set_bias(small)
        corpora["c"].set_bias(large)
        corpora["d"] = corpora["a"]
        run = {}
        for p in paths:
            cfg = F.Config(pf_lanes=64, sw_lanes=64, sort=F.SortStrategy.IndexAsc if p == "d" else F.SortStrategy.ScoreThenIndexAsc)
            m = F.Matcher(max(NEEDLES, key=len), cfg)
            m.reserve(corpora[p])
            run[p] = m

        def query(p):
            return host_side(run[p], corpora[p], small.astype(np.int32)) if p == "d" else run[p].match_list_top(corpora[p], LIMIT, copy=False)

        for _ in range(max(a.warmup, 1)):
            for needle in NEEDLES:
                got = {}
                for p in paths:
                    run[p].set_pattern(needle)
                    got[p] = query(p)
                for p, bias in (("b", small), ("c", large)):  # the device-side bias and the host-side one rank alike, on one selection level and on two
                    if p in got and "d" in run:
                        want = host_side(run["d"], corpora["a"], bias.astype(np.int32))
                        assert got[p][1] == want[1] and got[p][0].tolist() == want[0].tolist(), (p, needle)
        medians = {p: [] for p in paths}
        for _ in range(a.repeats):
            t = {p: [] for p in paths}
            for q in range(a.queries):
                needle = NEEDLES[q % len(NEEDLES)]
                for p in paths:
                    run[p].set_pattern(needle)
                    t0 = time.perf_counter()
                    query(p)
                    t[p].append((time.perf_counter() - t0) * 1e6)
            for p in paths:
                medians[p].append(float(np.median(t[p])))
        for p in paths:
            r = medians[p]
            print(json.dumps(dict(list="paths " + name, items=n, limit=LIMIT, path=NAMES[p], queries=a.queries * a.repeats, median_us=round(float(np.median(r)), 1),
                                  spread_us=[round(min(r), 1), round(max(r), 1)], repeat_medians_us=[round(x, 1) for x in r],
                                  bias_hi=corpora[p].bias_info()["bias_hi"])), flush=True)
        if a.only is None:  # the empty prompt, "most frecent first" (its own tool: tools/bench_prompt.py)
            e = F.Matcher("", F.Config(pf_lanes=64))
            ts = []
            for _ in range(max(3, a.repeats * 4)):
                t0 = time.perf_counter()
                e.match_list_top(corpora["c"], LIMIT)
                ts.append((time.perf_counter() - t0) * 1e6)
            print(json.dumps(dict(list="paths " + name, items=n, limit=LIMIT, path="empty prompt over the biased corpus", queries=len(ts),
                                  median_us=round(float(np.median(ts)), 1), spread_us=[round(min(ts), 1), round(max(ts), 1)])), flush=True)
        del run, corpora


if __name__ == "__main__":
    main()
