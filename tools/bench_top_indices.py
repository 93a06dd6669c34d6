"""What a picker pays per keystroke for "the best `limit` matches with their matched characters": host-clock timing, from the call to the
synchronised result on the host, of
    (a) `match_list_top` followed by `match_list_indices` over its head - the two-call composition, and
    (b) `match_list_top_indices` - the fused call, after `reserve` and `reserve_top_indices`
on the first 200 000 paths of the paths-shaped list and on the whole list (1.4 M), limit 100, the needles of a typed query
(tests/test_gpu_multi_requery.py's KEYS without their separators: s, sr, src, .. srclinuxtest) in turn.  Every shape is warmed up first; (a)
and (b) ALTERNATE query by query inside one process (drift of a shared host hits both alike); the needle changes outside the timed window
(`set_pattern`, the same for both).  `--repeats` repeats of `--queries` queries per path and list: the median of the repeats' medians and
their spread (lowest and highest repeat median), microseconds, one JSON line per list and path.  On a tree whose library has no fused
call the tool reports (a) only.

    python tools/bench_top_indices.py [--queries 600] [--repeats 5] [--only a|b] [--lists 200k,1.4M]
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

KEYS = ["s", "sr", "src", "src l", "src li", "src lin", "src linux", "src linux !", "src linux !t", "src linux !test"]
NEEDLES = list(dict.fromkeys(k.replace(" ", "").replace("!", "") for k in KEYS))
LIMIT = 100


def composed(m, cp):
    head, found = m.match_list_top(cp, LIMIT, copy=False)
    return len(m.match_list_indices(cp, head["index"][:LIMIT])) if len(head) else 0


def fused(m, cp):
    return len(m.match_list_top_indices(cp, LIMIT)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=600, help="timed queries per repeat, path and list")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3, help="untimed passes over the needles per path")
    ap.add_argument("--only", choices=("a", "b"), default=None, help="one path alone (what a kernel trace is taken of)")
    ap.add_argument("--lists", default="200k,1.4M")
    a = ap.parse_args()
    have_fused = hasattr(F.Matcher, "match_list_top_indices")
    paths = [p for p in ("a", "b") if (a.only in (None, p)) and (p == "a" or have_fused)]
    if not have_fused:
        print(json.dumps(dict(note="this tree has no match_list_top_indices: path (a) only")), flush=True)
    data, ends = synth.paths_corpus()
    cfg = F.Config(pf_lanes=64, sw_lanes=64)
    for name in a.lists.split(","):
        n = {"200k": 200_000, "1.4M": len(ends)}[name]
        cp = F.Corpus(packed=(data[: int(ends[n - 1])], ends[:n]))
        run = {}
        for p in paths:  # a matcher per path: each keeps its own buffers, as two pickers would
            m = F.Matcher(max(NEEDLES, key=len), cfg)
            m.reserve(cp)
            if p == "b":
                m.reserve_top_indices(cp, LIMIT, max(len(x) for x in NEEDLES))
            run[p] = (m, composed if p == "a" else fused)
        records = {}
        for _ in range(a.warmup):
            for needle in NEEDLES:
                for p in paths:
                    run[p][0].set_pattern(needle)
                    records[(p, needle)] = run[p][1](run[p][0], cp)
        if len(paths) == 2 and a.warmup:
            assert all(records[("a", x)] == records[("b", x)] for x in NEEDLES), records
        medians = {p: [] for p in paths}
        for _ in range(a.repeats):
            t = {p: [] for p in paths}
            for q in range(a.queries):
                needle = NEEDLES[q % len(NEEDLES)]
                for p in paths:
                    m, fn = run[p]
                    m.set_pattern(needle)
                    t0 = time.perf_counter()
                    fn(m, cp)
                    t[p].append((time.perf_counter() - t0) * 1e6)
            for p in paths:
                medians[p].append(float(np.median(t[p])))
        for p in paths:
            r = medians[p]
            print(json.dumps(dict(list="paths " + name, items=n, limit=LIMIT, path="(a) top + indices" if p == "a" else "(b) top_indices", queries=a.queries * a.repeats,
                                  median_us=round(float(np.median(r)), 1), spread_us=[round(min(r), 1), round(max(r), 1)], repeat_medians_us=[round(x, 1) for x in r],
                                  records=sum(records.get((p, x), 0) for x in NEEDLES))), flush=True)
        del run, cp


if __name__ == "__main__":
    main()
