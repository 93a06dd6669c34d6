"""What the matched positions of a grouped query cost: `MultiMatcher.match_list_top_indices_groups_device(limit)` and the host form,
ScoreThenIndexAsc, at `limit` 20 and 100, for `rs$ | py$ | go$` and `linux rs$ | py$ !test` on the paths-shaped list (1.4 M) and for
`dead | beef | cafe ...` at 2, 4 and 8 alternatives on the 10 M x 32-byte list.  Per row, measured in the same run on the same build:
    (groups_device / groups_host)  the new call - device time between two events around back-to-back calls, and the host form's wall time;
    (top_device)       the grouped `match_list_top_device` alone: the difference is what the positions cost;
    (ungrouped_device) an ungrouped fused `match_list_top_indices_device` with as many plain patterns (an AND of them: its head, and so
                       its tail, may be shorter - `ungrouped_found` says how long);
    (caller_today)     what a caller does today for the same result: the grouped `match_list_top`, then one single-pattern
                       `match_list_indices` over that head per non-negated pattern, unioned under the carrier rule in numpy - wall time.
The variants alternate repeat by repeat; the median of `--repeats` repeats and [lowest, highest], microseconds, one JSON line per row; with
FZB_DEBUG_CUS set (to the device's own number of compute units, say) also the launches of one grouped call per query.  `--check` (the default) holds the new call's records and positions to that numpy union first.

    python tools/bench_anyof_indices.py [--calls 10] [--repeats 5] [--lists paths1.4M,fixed10M] [--no-check]
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
import torch  # noqa: E402

import frizbee_amd as F  # noqa: E402

LIMITS = (20, 100)
FUZZY = ["dead", "beef", "cafe", "dbe", "ead", "deb", "adb", "eadb"]
QUERIES = {
    "paths1.4M": ["rs$ | py$ | go$", "linux rs$ | py$ !test"],
    "fixed10M": [" | ".join(FUZZY[:k]) for k in (2, 4, 8)],
}


def the_list(name):
    if name == "fixed10M":
        rows, ends = synth.fixed_corpus(b"deadbe", 10_000_000, 32)
        return rows.numpy().reshape(-1), ends
    return synth.paths_corpus()


def caller_today(cp, grouped, solo, pats, group_of, limit):
    """-> ([(index, score, exact, positions)], found): the ranked head from the grouped matcher, every non-negated pattern's positions over
    that head from its own matcher, the carrier rule and the descending unique union on the host"""
    head, found = grouped.match_list_top(cp, limit)
    sel = head["index"].astype(np.uint32)
    per = {}
    for j, m in solo.items():
        per[j] = {r.index: (r.score << 1 | int(r.exact), r.indices) for r in m.match_list_indices(cp, selection=sel)} if len(sel) else {}
    out = []
    for k, h in enumerate(head):
        seen = set()
        for g in sorted(set(group_of)):
            members = [j for j in range(len(pats)) if group_of[j] == g and j in solo]
            best, best_key = None, -1
            for j in members:
                hit = per[j].get(k)
                if hit is not None and hit[0] > best_key:
                    best, best_key = j, hit[0]
            if best is not None:
                seen.update(per[best][k][1])
        out.append((int(h["index"]), int(h["score"]), bool(h["exact"]), sorted(seen, reverse=True)))
    return out, found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls between the two events")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lists", default="paths1.4M,fixed10M")
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    cfg = F.Config(pf_lanes=64, sw_lanes=0, sort=F.SortStrategy.ScoreThenIndexAsc)
    cfg_asc = F.Config(pf_lanes=64, sw_lanes=0, sort=F.SortStrategy.IndexAsc)
    top = max(LIMITS)
    recs_dev = torch.zeros((top + 8) * 16, dtype=torch.uint8, device="cuda")
    pos_dev = torch.zeros(top * 64 + 64, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(16, dtype=torch.int32, device="cuda")
    for name in a.lists.split(","):
        data, ends = the_list(name)
        cp = F.Corpus(packed=(data, ends))
        n = len(cp)
        for text in QUERIES[name]:
            pats, group_of = F.parse_query_groups(text)
            k = max(group_of.count(g) for g in group_of)
            grouped = F.MultiMatcher(pats, cfg, groups=group_of)
            grouped.reserve(cp)
            grouped.reserve_top_indices_groups(cp, top, 8)
            ug = grouped.groups_positions_stride()
            plain = F.MultiMatcher(pats, cfg)
            plain.reserve(cp)
            plain.reserve_top_indices(cp, top, 8)
            u = sum(max(1, len(p.needle.encode())) for p in pats if not p.negated)
            solo = {j: F.MultiMatcher([F.Pattern(p.needle, matching=p.matching)], cfg_asc) for j, p in enumerate(pats) if not p.negated}
            ungrouped_found = plain.match_list_top(cp, 1)[1]
            for limit in LIMITS:
                if not a.no_check:
                    want = caller_today(cp, grouped, solo, pats, group_of, limit)
                    got, found = grouped.match_list_top_indices_groups(cp, limit)
                    got = [(r.index, r.score, bool(r.exact), list(r.indices)) for r in got]
                    assert (got, found) == want, (name, text, limit, [(g, w) for g, w in zip(got, want[0]) if g != w][:3], found, want[1])
                    print(json.dumps(dict(list=name, query=text, limit=limit, check="device records and positions == numpy union", found=found)), flush=True)

                def device_us(call):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(a.calls):
                        call()
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1) * 1e3 / a.calls

                def wall_us(call, calls):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        call()
                    return (time.perf_counter() - t0) * 1e6 / calls

                variants = {
                    "groups_device": lambda: device_us(lambda: grouped.match_list_top_indices_groups_device(cp, limit, recs_dev.data_ptr(), limit, pos_dev.data_ptr(), limit * ug,
                                                                                                            cnt.data_ptr())),
                    "groups_host": lambda: wall_us(lambda: grouped.match_list_top_indices_groups(cp, limit), a.calls),
                    "top_device": lambda: device_us(lambda: grouped.match_list_top_device(cp, limit, recs_dev.data_ptr(), limit, cnt.data_ptr())),
                    "ungrouped_device": lambda: device_us(lambda: plain.match_list_top_indices_device(cp, limit, recs_dev.data_ptr(), limit, pos_dev.data_ptr(), limit * u, cnt.data_ptr())),
                    "caller_today": lambda: wall_us(lambda: caller_today(cp, grouped, solo, pats, group_of, limit), 2),
                }
                times = {v: [] for v in variants}
                for rep in range(a.warmup + a.repeats):
                    for v, fn in variants.items():
                        t = fn()
                        if rep >= a.warmup:
                            times[v].append(t)
                for v, t in times.items():
                    print(json.dumps(dict(list=name, items=n, query=text, alternatives=k, sources=len(solo), variant=v, limit=limit, calls=a.calls, repeats=a.repeats,
                                          ungrouped_found=ungrouped_found, median_us=round(float(np.median(t)), 1), spread_us=[round(min(t), 1), round(max(t), 1)])), flush=True)
            if os.environ.get("FZB_DEBUG_CUS"):  # (the library records its launches only under that switch)
                F.launch_grids()
                grouped.match_list_top_indices_groups(cp, top)
                print(json.dumps(dict(list=name, query=text, limit=top, launches={kern: v[2] for kern, v in F.launch_grids().items()})), flush=True)
            del grouped, plain, solo
        del cp


if __name__ == "__main__":
    main()
