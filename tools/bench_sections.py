"""What a picker's sections cost per keystroke: device time between two events around back-to-back calls, `limit` 20, ScoreThenIndexAsc, on
the 10 M x 32-byte list with needle "deadbe" and on the paths-shaped list (1.4 M, needle "linux"), random 16-bit tags, for S = 1, 4, 8
sections (S = 1 is (0, 0), "everything"; the others are the first 4 / all 8 of the test suite's sections):
    (plain)      one unsectioned `match_list_top_device(20)` - the call every caller has;
    (sectioned)  ONE `match_list_top_sections_device(sections, 20)`: the filter and the scorers run once, the selection and the ordering
                 run for the S sections together (kernels_sections.hip);
    (today)      what a caller without the feature does for S sections: S x (`set_scope(require, exclude)` + `match_list_top_device(20)`).
The variants alternate repeat by repeat, each on its own reserved matcher over the same corpus; the median of `--repeats` repeats and
[lowest, highest], microseconds per call (per S calls for "today"), one JSON line per row.  The two targets are judged in the same run
against the build's own plain calls: S = 4 sectioned <= two scoped top calls ("today" over the sections (1, 0) and (2, 1), its own row), and
S = 1 sectioned within 15 us of (plain).  `--check` (the default) holds the device's heads and counts against a numpy model over the full index-ordered `match_list`
before anything is timed.

    python tools/bench_sections.py [--calls 50] [--repeats 9] [--lists fixed10M,paths1.4M] [--no-check]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import synth  # noqa: E402
import torch  # noqa: E402

import frizbee_amd as F  # noqa: E402

LIMIT = 20
EIGHT = [(1, 0), (2, 1), (0, 0), (0xF0, 0), (1, 1), (1, 0), (0xFFF, 0), (0, 0x8000)]
SECTIONS = {1: [(0, 0)], 4: EIGHT[:4], 8: EIGHT}
TWO_SCOPED = EIGHT[:2]  # the yardstick of the S = 4 target: two top calls under a scope each


def the_list(name):
    if name == "fixed10M":
        rows, ends = synth.fixed_corpus(b"deadbe", 10_000_000, 32)
        return rows.numpy().reshape(-1), ends, "deadbe"
    data, ends = synth.paths_corpus()
    return data, ends, "linux"


def model(index_asc, tags, sections, limit):
    """[(head, found)] from the full index-ordered list: the section's records, stable sort by descending score, cut"""
    t = tags[index_asc["index"]].astype(np.uint32)
    out = []
    for require, exclude in sections:
        sel = index_asc[((t & require) == require) & ((t & exclude) == 0)]
        sel = sel[np.argsort(-sel["score"].astype(np.int64), kind="stable")]
        out.append((sel[:limit], len(sel)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="back-to-back calls between the two events")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lists", default="fixed10M,paths1.4M")
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    cfg = F.Config(pf_lanes=64, sw_lanes=64, sort=F.SortStrategy.ScoreThenIndexAsc)
    out = torch.zeros((8 * LIMIT + 8) * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(16, dtype=torch.int32, device="cuda")
    for name in a.lists.split(","):
        data, ends, needle = the_list(name)
        n = len(ends)
        tags = np.random.default_rng(7).integers(0, 65536, n).astype(np.uint16)
        cp = F.Corpus(packed=(data, ends))
        cp.set_tags(tags)
        run = {v: F.Matcher(needle, cfg) for v in ("plain", "sectioned", "today")}
        for m in run.values():
            m.reserve(cp)

        def call(v, sections):
            if v == "plain":
                run[v].match_list_top_device(cp, LIMIT, out.data_ptr(), LIMIT, cnt.data_ptr())
            elif v == "sectioned":
                run[v].match_list_top_sections_device(cp, sections, LIMIT, out.data_ptr(), len(sections) * LIMIT, cnt.data_ptr())
            else:
                for require, exclude in sections:
                    cp.set_scope(require, exclude)
                    run[v].match_list_top_device(cp, LIMIT, out.data_ptr(), LIMIT, cnt.data_ptr())
                cp.set_scope(0, 0)

        if not a.no_check:
            full = F.Matcher(needle, F.Config(pf_lanes=64, sw_lanes=64, sort=F.SortStrategy.IndexAsc)).match_list(cp)
            for S, sections in SECTIONS.items():
                want = model(full, tags, sections, LIMIT)
                call("sectioned", sections)
                torch.cuda.synchronize()
                recs, words = out.cpu().numpy().view(F.MATCH_DTYPE), cnt.tolist()
                for s, (head, found) in enumerate(want):
                    got = recs[s * LIMIT:s * LIMIT + words[2 * s]]
                    assert words[2 * s + 1] == found and got.tolist() == head.tolist(), (name, S, s, words[2 * s:2 * s + 2], found, got[:3], head[:3])
                host = run["sectioned"].match_list_top_sections(cp, sections, LIMIT)
                assert [(r.tolist(), f) for r, f in host] == [(h.tolist(), f) for h, f in want], (name, S, "host form")
            print(json.dumps(dict(list=name, check="device heads == numpy model", matches=len(full))), flush=True)
        rows = [("plain", 1), ("today", 2)] + [(v, S) for S in SECTIONS for v in ("sectioned", "today")]
        times = {r: [] for r in rows}
        for rep in range(a.warmup + a.repeats):
            for v, S in rows:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.calls):
                    call(v, TWO_SCOPED if S == 2 else SECTIONS[S])
                e1.record()
                e1.synchronize()
                if rep >= a.warmup:
                    times[(v, S)].append(e0.elapsed_time(e1) * 1e3 / a.calls)
        torch.cuda.synchronize()
        med = {r: float(np.median(t)) for r, t in times.items()}
        for (v, S), t in times.items():
            print(json.dumps(dict(list=name, items=n, needle=needle, variant=v, sections=S, limit=LIMIT, calls=a.calls, repeats=a.repeats, median_us=round(med[(v, S)], 1),
                                  spread_us=[round(min(t), 1), round(max(t), 1)])), flush=True)
        two_scoped = med[("today", 2)]
        print(json.dumps(dict(list=name, target="S = 4 sectioned <= two scoped top calls", sectioned_us=round(med[("sectioned", 4)], 1), two_scoped_us=round(two_scoped, 1),
                              met=bool(med[("sectioned", 4)] <= two_scoped))), flush=True)
        print(json.dumps(dict(list=name, target="S = 1 sectioned within 15 us of plain", sectioned_us=round(med[("sectioned", 1)], 1), plain_us=round(med[("plain", 1)], 1),
                              over_us=round(med[("sectioned", 1)] - med[("plain", 1)], 1), met=bool(med[("sectioned", 1)] - med[("plain", 1)] <= 15.0))), flush=True)
        del run, cp


if __name__ == "__main__":
    main()
