"""What a picker pays per keystroke for "the best `limit` matches with their matched characters" when the query is query syntax (a
`from_patterns` matcher): host-clock timing, from the call to the synchronised result on the host, of
    (a) `MultiMatcher.match_list_top` followed by `MultiMatcher.match_list_indices` over its head - two public calls, which is what the
        host composition fzb_multi_match_list_top_indices does inside (P + 1 round trips for P patterns), and
    (b) `MultiMatcher.match_list_top_indices` - the device-fused call (one wait), after `reserve` and `reserve_top_indices`
on the first 200 000 paths of the paths-shaped list and on the whole list (1.4 M), limit 100, the typed query of
tests/test_gpu_multi_requery.py's KEYS WITH their separators (s, sr, src, src l, .. src linux !test: one to three patterns, one of them
negated) in turn.  Every shape is warmed up first; (a) and (b) ALTERNATE query by query inside one process (drift of a shared host hits both
alike); the patterns change outside the timed window (`set_patterns`, the same for both).  `--repeats` repeats of `--queries` queries per
path and list: the median of the repeats' medians and their spread (lowest and highest repeat median), microseconds - one JSON line per
list and path over all keys, and one per list, path and key.  `--root DIR` imports the package from another tree (a build of an earlier
commit, whose `match_list_top_indices` is then what (b) times; `reserve_top_indices` is called where the tree has it).

    python tools/bench_multi_top_indices.py [--queries 600] [--repeats 5] [--only a|b] [--lists 200k,1.4M] [--root DIR]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["s", "sr", "src", "src l", "src li", "src lin", "src linux", "src linux !", "src linux !t", "src linux !test"]
LIMIT = 100


def composed(F, m, cp):
    head, found = m.match_list_top(cp, LIMIT, copy=False)
    return len(m.match_list_indices(cp, head["index"][:LIMIT])) if len(head) else 0


def fused(F, m, cp):
    return len(m.match_list_top_indices(cp, LIMIT)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=600, help="timed queries per repeat, path and list")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3, help="untimed passes over the keys per path")
    ap.add_argument("--only", choices=("a", "b"), default=None, help="one path alone (what a kernel trace is taken of)")
    ap.add_argument("--lists", default="200k,1.4M")
    ap.add_argument("--root", default=ROOT, help="the tree frizbee_amd is imported from")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    import synth

    import frizbee_amd as F

    is_fused = "fzb_multi_match_list_top_indices_fused" in F.SYMBOLS
    paths = [p for p in ("a", "b") if a.only in (None, p)]
    print(json.dumps(dict(package=os.path.dirname(os.path.abspath(F.__file__)), b_is="device-fused" if is_fused else "host composition")), flush=True)
    data, ends = synth.paths_corpus()
    cfg = F.Config(pf_lanes=64, sw_lanes=64)
    pats = {k: F.parse_query(k) for k in KEYS}
    npat = {k: len(pats[k]) for k in KEYS}
    longest = max(len(x) for k in KEYS for x in k.replace("!", "").split())
    for name in a.lists.split(","):
        n = {"200k": 200_000, "1.4M": len(ends)}[name]
        cp = F.Corpus(packed=(data[: int(ends[n - 1])], ends[:n]))
        run = {}
        for p in paths:  # a matcher per path: each keeps its own buffers, as two pickers would
            m = F.MultiMatcher(pats[KEYS[-1]], cfg)  # the most patterns first: the slots every later query needs
            m.reserve(cp)
            if p == "b" and hasattr(m, "reserve_top_indices"):
                m.reserve_top_indices(cp, LIMIT, longest)
            run[p] = (m, composed if p == "a" else fused)
        records = {}
        for _ in range(a.warmup):
            for key in KEYS:
                for p in paths:
                    run[p][0].set_patterns(pats[key])
                    records[(p, key)] = run[p][1](F, run[p][0], cp)
        if len(paths) == 2 and a.warmup:
            assert all(records[("a", k)] == records[("b", k)] for k in KEYS), records
        medians = {p: [] for p in paths}
        key_medians = {(p, k): [] for p in paths for k in KEYS}
        for _ in range(a.repeats):
            t = {(p, k): [] for p in paths for k in KEYS}
            for q in range(a.queries):
                key = KEYS[q % len(KEYS)]
                for p in paths:
                    m, fn = run[p]
                    m.set_patterns(pats[key])
                    t0 = time.perf_counter()
                    fn(F, m, cp)
                    t[(p, key)].append((time.perf_counter() - t0) * 1e6)
            for p in paths:
                medians[p].append(float(np.median(np.concatenate([t[(p, k)] for k in KEYS]))))
                for k in KEYS:
                    if t[(p, k)]:
                        key_medians[(p, k)].append(float(np.median(t[(p, k)])))
        label = {"a": "(a) top + indices", "b": "(b) top_indices"}
        for p in paths:
            r = medians[p]
            print(json.dumps(dict(list="paths " + name, items=n, limit=LIMIT, path=label[p], queries=a.queries * a.repeats, median_us=round(float(np.median(r)), 1),
                                  spread_us=[round(min(r), 1), round(max(r), 1)], repeat_medians_us=[round(x, 1) for x in r], records=sum(records.get((p, k), 0) for k in KEYS))), flush=True)
        for k in KEYS:
            for p in paths:
                r = key_medians[(p, k)]
                if r:
                    print(json.dumps(dict(list="paths " + name, key=k, patterns=npat[k], path=label[p], median_us=round(float(np.median(r)), 1),
                                          spread_us=[round(min(r), 1), round(max(r), 1)])), flush=True)
        del run, cp


if __name__ == "__main__":
    main()
