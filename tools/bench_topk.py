"""Host-clock timing of the top-`limit` queries next to `match_list` on the same resident lists: warm-up, then `--calls` synchronous calls
per variant with the variants ALTERNATED inside one process (so that drift of a shared host hits all of them alike); medians, the
min-max spread and the 10th / 90th percentiles (a shared host's hiccups land in the maximum), microseconds.  Lists: C2 (10 M x 32 B, 'deadbe'), the 1.4 M paths-shaped list and the 100 k paths list ('linux'; the query
`src linux !test` as a multi-pattern matcher on the two paths lists), and C2 as 8 oversubscribed shards.  One JSON line per variant.

    python tools/bench_topk.py [--calls 200] [--small]      (--small: lists a tenth of the size, for a quick look)
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


def timed(variants, calls, warmup=10):
    """variants: {name: callable -> number of records}.  Returns {name: (median, min, max, records)} in microseconds."""
    names = list(variants)
    recs = {}
    for _ in range(warmup):
        for nm in names:
            recs[nm] = variants[nm]()
    t = {nm: [] for nm in names}
    for _ in range(calls):
        for nm in names:
            t0 = time.perf_counter()
            variants[nm]()
            t[nm].append((time.perf_counter() - t0) * 1e6)
    return {nm: (float(np.median(t[nm])), float(np.min(t[nm])), float(np.max(t[nm])), recs[nm], float(np.percentile(t[nm], 10)), float(np.percentile(t[nm], 90))) for nm in names}


def report(title, found, res):
    for nm, (med, lo, hi, n, p10, p90) in res.items():
        print(json.dumps(dict(list=title, found=found, variant=nm, records=n, median_us=round(med, 1), min_us=round(lo, 1), max_us=round(hi, 1), p10_us=round(p10, 1),
                              p90_us=round(p90, 1))), flush=True)


def resident(title, m, cp, calls):
    found = len(m.match_list(cp))
    limits = (100, 10_000, max(found, 1) * 2)
    v = {"match_list": lambda: len(m.match_list(cp, copy=False))}
    for limit in limits:
        v["top(%s)" % ("limit>=found" if limit == limits[-1] else limit)] = lambda limit=limit: len(m.match_list_top(cp, limit, copy=False)[0])
    report(title, found, timed(v, calls))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--only-c2", action="store_true", help="the C2 list alone (what a kernel trace is taken of)")
    a = ap.parse_args()
    div = 10 if a.small else 1
    cfg = F.Config(pf_lanes=64, sw_lanes=64)
    rows, ends = synth.fixed_corpus(b"deadbe", 10_000_000 // div, 32)
    c2 = (rows.numpy().reshape(-1), ends)
    cp = F.Corpus(packed=c2)
    m = F.Matcher("deadbe", cfg)
    m.reserve(cp)
    resident("C2 10M x 32B 'deadbe'", m, cp, a.calls)
    del cp
    if a.only_c2:
        return
    for npaths, name in ((1_406_941 // div, "paths 1.4M"), (100_000 // div, "paths 100k")):
        data, pends = synth.paths_corpus(b"linux", npaths)
        pc = F.Corpus(packed=(data, pends))
        m = F.Matcher("linux", cfg)
        m.reserve(pc)
        resident(name + " 'linux'", m, pc, a.calls)
        mm = F.MultiMatcher(F.parse_query("src linux !test"), F.Config(pf_lanes=64))
        mm.reserve(pc)
        resident(name + " multi 'src linux !test'", mm, pc, a.calls)
        del pc
    sc = F.ShardedCorpus(packed=c2, ndev=8, oversubscribe=8 > F.device_count())
    m = F.Matcher("deadbe", cfg)
    found = len(m.match_list_parallel_sharded(sc))
    report("C2 as 8 shards", found, timed({"match_list_parallel_sharded": lambda: len(m.match_list_parallel_sharded(sc, copy=False)),
                                           "top_sharded(100)": lambda: len(m.match_list_top_sharded(sc, 100, copy=False)[0])}, a.calls))


if __name__ == "__main__":
    main()
