"""What a facet sink (`Facets`, `Matcher.set_facets`) costs per query: device time between two events around 50 back-to-back
`match_list_top_device(100)` calls on the 10 M x 32-byte list with needle "deadbe" and on the paths-shaped list (1.4 M, needle "linux"),
ScoreThenIndexAsc, with the scope off and with a scope that hides half of the list:
    (a) the call with no sink attached - the path every caller had before sinks existed;
    (b) the same call with a sink attached: the record form's launch with the scope off, the count fused into the flag pass under a scope;
    (c) what a caller without the feature does: the same call, then a second, UNSCOPED `match_list` copied back and the tags gathered and
        counted in numpy (its host work lies between the two events too: the device idles behind it).
The variants alternate repeat by repeat (a, b, c, a, b, c, ...), each on its own reserved matcher over the same corpus; `--repeats` repeats:
the median of the repeats and [lowest, highest], microseconds per call, one JSON line per row and variant.  `--check` (the default) holds
(b)'s counts against (c)'s before anything is timed.  `--baseline` times (a) alone through calls every build has: run it with
`--package-root DIR` on a build of the parent commit for the parent's figure of the same call in the same run.

    python tools/bench_facets.py [--calls 50] [--repeats 9] [--lists fixed10M,paths1.4M] [--baseline [--package-root DIR]] [--no-check]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --package-root DIR: import frizbee_amd from DIR - another build of the package, the parent commit's for --baseline
PKG = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1]) if "--package-root" in sys.argv[:-1] else ROOT
sys.path.insert(0, PKG)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import synth  # noqa: E402
import torch  # noqa: E402

import frizbee_amd as F  # noqa: E402

LIMIT = 100
NAMES = {"a": "(a) no sink", "b": "(b) sink attached", "c": "(c) no sink + unscoped match_list + numpy"}


def the_list(name):
    if name == "fixed10M":
        rows, ends = synth.fixed_corpus(b"deadbe", 10_000_000, 32)
        return rows.numpy().reshape(-1), ends, "deadbe"
    data, ends = synth.paths_corpus()
    return data, ends, "linux"


def numpy_counts(records, tags, require, exclude):
    """the 34 words from a full, unscoped record list: the gather and the counting a caller does on the host"""
    t = tags[records["index"]].astype(np.uint32)
    vis = ((t & require) == require) & ((t & exclude) == 0)
    out = np.zeros(34, np.uint32)
    out[0], out[1] = len(t), int(vis.sum())
    for b in range(16):
        has = (t >> b) & 1
        out[2 + b] = int(has.sum())
        out[18 + b] = int(has[vis].sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="back-to-back calls between the two events")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lists", default="fixed10M,paths1.4M")
    ap.add_argument("--baseline", action="store_true", help="variant (a) alone, through calls a build without sinks has")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--package-root", default=ROOT, help="the directory frizbee_amd is imported from (read before the import)")
    a = ap.parse_args()
    variants = ["a"] if a.baseline else list(NAMES)
    cfg = F.Config(pf_lanes=64, sw_lanes=64, sort=F.SortStrategy.ScoreThenIndexAsc)
    out = torch.zeros((LIMIT + 8) * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    for name in a.lists.split(","):
        data, ends, needle = the_list(name)
        n = len(ends)
        rng = np.random.default_rng(7)
        tags = rng.integers(0, 65536, n).astype(np.uint16)  # bit 0: the hidden half
        cp = F.Corpus(packed=(data, ends))
        cp.set_tags(tags)
        run = {v: F.Matcher(needle, cfg) for v in variants}
        sink = None
        if "b" in run:
            sink = F.Facets(cp)
            run["b"].set_facets(sink)
        for m in run.values():
            m.reserve(cp)
        for row, scope in (("scope off", (0, 0)), ("scope hides half", (0, 1))):

            def call(v):
                run[v].match_list_top_device(cp, LIMIT, out.data_ptr(), LIMIT, cnt.data_ptr())
                if v == "c":  # today's caller: a second, unscoped query over the link, the gather and the counting on the host
                    cp.set_scope(0, 0)
                    full = run[v].match_list(cp, copy=False)
                    cp.set_scope(*scope)
                    return numpy_counts(full, tags, *scope)
                return None

            cp.set_scope(*scope)
            if not a.no_check and not a.baseline:
                want = call("c")
                call("b")
                got = sink.read_words()
                torch.cuda.synchronize()
                assert got.tolist() == want.tolist() and int(cnt[1]) == int(want[1]), (name, row, got.tolist(), want.tolist(), cnt.tolist())
            times = {v: [] for v in variants}
            for rep in range(a.warmup + a.repeats):
                for v in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(a.calls):
                        call(v)
                    e1.record()
                    e1.synchronize()
                    if rep >= a.warmup:
                        times[v].append(e0.elapsed_time(e1) * 1e3 / a.calls)
            torch.cuda.synchronize()
            for v in variants:
                r = times[v]
                print(json.dumps(dict(list=name, items=n, needle=needle, row=row, variant=NAMES[v], found=int(cnt[1]), calls=a.calls, repeats=a.repeats,
                                      median_us=round(float(np.median(r)), 1), spread_us=[round(min(r), 1), round(max(r), 1)])), flush=True)
        del run, sink, cp


if __name__ == "__main__":
    main()
