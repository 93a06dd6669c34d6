"""What a candidate set costs and gains under QUERY SYNTAX (`MultiMatcher.match_list_top_device(subset=..., capture=...)`, `NarrowingQuery`),
on the paths-shaped 1.4 M list (`src linux !test`) and the 10 M x 32-byte list (`dead be !x`).  Three parts, one JSON line per row, a header
line with the GPU and the ROCm version:

  restrict   DEVICE time of `match_list_top_device(100)` (two events around `--iters` back-to-back asynchronous calls, divided by the calls;
             the variants ALTERNATE repeat by repeat inside one process; median [lowest, highest] of `--repeats` repeats, microseconds): over
             the whole list; over a `Subset.from_scope` of one haystack in twenty and of one half; under the equivalent `set_scope` (the drop
             pass behind the composition); over a second corpus of the visible haystacks alone.  The claim to check: subset <= scoped query
             on the one-in-twenty restriction.
  keystroke  the query typed character by character through `NarrowingQuery(max_fraction=1.0)` against the same loop with max_fraction=0.0
             (never narrowing): HOST time per keystroke of `query(text, 100)` - the call a picker makes, its one wait included -, the two
             loops alternating, median [lowest, highest] over the repeats; with the candidate count and fraction of every narrowed step.
             NarrowingQuery.DEFAULT_MAX_FRACTION = 0.8 x the largest fraction at which the narrowed step was not slower, 0.0 if none.

Before anything is timed every restricted result is checked against the scoped query's, every narrowed one against the un-narrowed one's.

  capture    what a capture costs a composition: the whole-list call without one, with one written by the launch of the final copy
             (k_copy_capture_records) and with the copy and the capture as two launches; device times as in `restrict`.

    python tools/bench_multi_subset.py [--parts restrict,capture,keystroke] [--iters 50] [--repeats 5] [--key-repeats 30] [--lists fixed10M,paths1.4M]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import frizbee_amd as F  # noqa: E402
from bench_scope import sub_packed, the_list  # noqa: E402
from bench_subset import LIMIT, Call, alternate, emit  # noqa: E402

QUERY = {"fixed10M": "dead be !x", "paths1.4M": "src linux !test"}


def part_restrict(a, name, cfg):
    data, ends, _, row = the_list(name)
    n = len(ends)
    query = QUERY[name]
    rng = np.random.default_rng(7)
    tags = ((rng.random(n) < 0.5).astype(np.uint16)) | ((rng.random(n) >= 0.05).astype(np.uint16) << 1)  # bench_scope's: bit 0 = outside the half, bit 1 = outside the 1 in 20
    cp = F.Corpus(packed=(data, ends))
    cp.set_tags(tags)
    m = F.MultiMatcher(F.parse_query(query), cfg)
    m.reserve(cp)
    sub = F.Subset(cp)
    whole = Call(m, cp)
    for label, exclude in (("1 in 20 visible", 2), ("half visible", 1)):
        vis = (tags & exclude) == 0
        second = F.Corpus(packed=sub_packed(data, ends, vis, row))
        m2 = F.MultiMatcher(F.parse_query(query), cfg)
        m2.reserve(second)
        sub.from_scope(0, exclude)
        assert len(sub) == int(vis.sum())
        scoped, own, over = Call(m, cp), Call(m2, second), Call(m, cp, subset=sub)
        cp.set_scope(0, exclude)
        want = scoped.result()
        cp.set_scope(0, 0)
        got = over.result()
        assert got[1] == want[1] and got[0].tolist() == want[0].tolist(), (name, label)
        unscoped = lambda: cp.set_scope(0, 0)  # noqa: E731
        r = alternate({"whole": (whole, unscoped), "scoped": (scoped, lambda: cp.set_scope(0, exclude)), "second_corpus": (own, None), "from_scope": (over, unscoped)}, a.iters, a.repeats)
        emit(part="restrict", list=name, items=n, query=query, visibility=label, visible=int(vis.sum()), found=want[1], limit=LIMIT, iters=a.iters, repeats=a.repeats,
             whole_list_us=r["whole"], scoped_query_us=r["scoped"], second_corpus_of_the_visible_us=r["second_corpus"], query_over_subset_from_scope_us=r["from_scope"],
             subset_not_slower_than_scoped=bool(r["from_scope"][0] <= r["scoped"][0]))
        del second, m2
    cp.set_scope(0, 0)


def part_capture(a, name, cfg):
    """what a capture costs a composition: the whole-list call without one, with one written by the final copy's launch, and with the copy and
    the capture as two launches (the fzb_debug_set_fused_capture hook)"""
    data, ends, _, _ = the_list(name)
    query = QUERY[name]
    cp = F.Corpus(packed=(data, ends))
    m = F.MultiMatcher(F.parse_query(query), cfg)
    m.reserve(cp)
    cap = F.Subset(cp)
    plain, capturing = Call(m, cp), Call(m, cp, capture=cap)
    fused = lambda on: (lambda: F.lib().fzb_debug_set_fused_capture(on))  # noqa: E731
    want = plain.result()
    for on in (0, 1):
        fused(on)()
        got = capturing.result()
        assert got[1] == want[1] and got[0].tolist() == want[0].tolist() and len(cap) == want[1], (name, on)
    r = alternate({"none": (plain, None), "fused": (capturing, fused(1)), "two_launches": (capturing, fused(0))}, a.iters, a.repeats)
    fused(1)()
    emit(part="capture", list=name, items=len(cp), query=query, found=want[1], limit=LIMIT, iters=a.iters, repeats=a.repeats, without_capture_us=r["none"],
         capture_in_the_final_copy_us=r["fused"], copy_then_capture_us=r["two_launches"], fused_saves_us=round(r["two_launches"][0] - r["fused"][0], 1))


def part_keystroke(a, name, cfg):
    data, ends, _, _ = the_list(name)
    query = QUERY[name]
    cp = F.Corpus(packed=(data, ends))
    n = len(cp)
    loops = {"narrowing": F.NarrowingQuery(cp, cfg, max_fraction=1.0), "never": F.NarrowingQuery(cp, cfg, max_fraction=0.0)}
    for nq in loops.values():
        nq.matcher.set_patterns(query)
        nq.matcher.reserve(cp)
    steps = [query[:k] for k in range(1, len(query) + 1)]
    times = {k: [[] for _ in steps] for k in loops}
    narrowed, candidates, found = [False] * len(steps), [None] * len(steps), [0] * len(steps)
    first = {}
    for r in range(a.key_repeats + 1):  # (the first pass warms up and checks)
        for name_ in (("narrowing", "never") if r % 2 else ("never", "narrowing")):
            nq = loops[name_]
            nq.reset()
            got = []
            for i, text in enumerate(steps):
                before = nq.subsets[nq._cur].info()["count"] if nq._cur is not None else None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = nq.query(text, LIMIT)
                dt = (time.perf_counter() - t0) * 1e6
                if r:
                    times[name_][i].append(dt)
                else:
                    got.append(res)
                if name_ == "narrowing":
                    narrowed[i], candidates[i], found[i] = nq.last_narrowed, before if nq.last_narrowed else None, res[1]
            if r == 0:
                first[name_] = got
    for i, text in enumerate(steps):
        assert first["narrowing"][i][1] == first["never"][i][1] and first["narrowing"][i][0].tolist() == first["never"][i][0].tolist(), (name, text)
    best = 0.0
    for i, text in enumerate(steps):
        med = {k: (round(float(np.median(times[k][i])), 1), round(min(times[k][i]), 1), round(max(times[k][i]), 1)) for k in times}
        if narrowed[i] and med["narrowing"][0] <= med["never"][0]:
            best = max(best, candidates[i] / n)
        emit(part="keystroke", list=name, items=n, query=text, limit=LIMIT, found=found[i], narrowed=narrowed[i], candidates=candidates[i],
             fraction=None if candidates[i] is None else round(candidates[i] / n, 4), repeats=a.key_repeats, narrowing_loop_host_us=med["narrowing"], never_narrowing_host_us=med["never"])
    total = {k: round(float(np.median(np.sum(np.array(times[k]), axis=0))), 1) for k in times}
    emit(part="keystroke", list=name, whole_loop_narrowing_host_us=total["narrowing"], whole_loop_never_host_us=total["never"], largest_fraction_not_slower=round(best, 4),
         max_fraction_candidate=round(0.8 * best, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="restrict,capture,keystroke")
    ap.add_argument("--iters", type=int, default=50, help="back-to-back calls between the two events")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--key-repeats", type=int, default=30, help="timed passes of each keystroke loop")
    ap.add_argument("--lists", default="fixed10M,paths1.4M")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_subset.py measures on the device: it needs the GPU")
    emit(gpu=torch.cuda.get_device_name(0), rocm=torch.version.hip, torch=torch.__version__, iters=a.iters, repeats=a.repeats, key_repeats=a.key_repeats, limit=LIMIT,
         timing="restrict: device events around back-to-back match_list_top_device calls; keystroke: host time of NarrowingQuery.query; median [lowest, highest] / median of the repeats, us")
    cfg = F.Config(pf_lanes=64, sw_lanes=64, sort=F.SortStrategy.ScoreThenIndexAsc)
    for name in a.lists.split(","):
        for part in a.parts.split(","):
            dict(restrict=part_restrict, capture=part_capture, keystroke=part_keystroke)[part](a, name, cfg)


if __name__ == "__main__":
    main()
