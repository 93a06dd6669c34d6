"""The multi-pattern matcher's interactive loop: a picker re-parses the query on every keystroke.  Over the paths list (synth.paths_corpus,
1.4 M paths) and a 100 k slice, the keystroke sequence below is replayed three ways - a fresh MultiMatcher per keystroke, set_patterns on one
reserved matcher, and the sharded form (8 shards oversubscribed on the visible devices) against the unsharded query - and each keystroke's
time is printed: host wall time of the whole step, and HIP events on the null stream around it (every entry point here is synchronous, so
the two differ by host work only).  Usage on a GPU box: python tools/bench_multi.py [--reps R]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import frizbee_amd as F  # noqa: E402
import synth  # noqa: E402

KEYS = ["s", "sr", "src", "src l", "src li", "src lin", "src linux", "src linux !", "src linux !t", "src linux !test"]


def timed(fn):
    """(result, host ms, device ms between events on the null stream)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return r, (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)


def replay(step, reps):
    """per keystroke: median host ms, median event ms, matches"""
    host, ev, n = [[] for _ in KEYS], [[] for _ in KEYS], [0] * len(KEYS)
    for _ in range(reps):
        for k, q in enumerate(KEYS):
            r, h, e = timed(lambda: step(q))
            host[k].append(h)
            ev[k].append(e)
            n[k] = len(r)
    return [(float(np.median(host[k])), float(np.median(ev[k])), n[k]) for k in range(len(KEYS))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.init()
    data, ends = synth.paths_corpus()
    cfg = F.Config(pf_lanes=64)
    for n in (100_000, len(ends)):
        e = ends[:n]
        d = data[: int(e[-1])]
        cp = F.Corpus(packed=(d, e))
        sc = F.ShardedCorpus(packed=(d, e), ndev=8, by_bytes=True, oversubscribe=True)

        fresh = replay(lambda q: F.MultiMatcher(F.parse_query(q), cfg).match_list(cp, copy=False), args.reps)
        m = F.MultiMatcher([], cfg)
        for q in KEYS:
            m.set_patterns(F.parse_query(q))
            m.match_list(cp)
        m.reserve(cp)
        allocs = F.device_allocs()

        def requery(q):
            m.set_patterns(F.parse_query(q))
            return m.match_list(cp, copy=False)
        reuse = replay(requery, args.reps)
        allocs = F.device_allocs() - allocs
        ms = F.MultiMatcher([], cfg)

        def sharded(q):
            ms.set_patterns(F.parse_query(q))
            return ms.match_list_parallel_sharded(sc, copy=False)
        shard = replay(sharded, args.reps)
        print(f"\n{n} paths ({args.reps} replays, medians; device allocations during the set_patterns replays: {allocs})")
        print(f"{'keystroke':<18} {'matches':>8} | {'fresh host':>10} {'fresh ev':>9} | {'set_pat host':>12} {'set_pat ev':>10} | {'8 shards host':>13} {'8 shards ev':>11}")
        for k, q in enumerate(KEYS):
            assert fresh[k][2] == reuse[k][2] == shard[k][2], (q, fresh[k][2], reuse[k][2], shard[k][2])
            print(f"{q!r:<18} {fresh[k][2]:>8} | {fresh[k][0]:>10.3f} {fresh[k][1]:>9.3f} | {reuse[k][0]:>12.3f} {reuse[k][1]:>10.3f} | {shard[k][0]:>13.3f} {shard[k][1]:>11.3f}")
        tot = lambda rows, i: sum(r[i] for r in rows)
        print(f"{'sequence total':<18} {'':>8} | {tot(fresh, 0):>10.3f} {tot(fresh, 1):>9.3f} | {tot(reuse, 0):>12.3f} {tot(reuse, 1):>10.3f} | {tot(shard, 0):>13.3f} {tot(shard, 1):>11.3f}")
        print("shard report:", ms.shard_report(), flush=True)


if __name__ == "__main__":
    main()
