"""What a picker's HIGHLIGHTED sections cost per keystroke: `limit` 20, ScoreThenIndexAsc, on the 10 M x 32-byte list with needle "deadbe" and on
the paths-shaped list (1.4 M, needle "linux"), random 16-bit tags, no bias and no scope (so that baseline (ii) exists), for S = 1, 4, 8
sections (S = 1 is (0, 0), "everything"; the others are the first 4 / all 8 of the test suite's sections):
    (new)        ONE `match_list_top_sections_indices(sections, 20)` - `_device` form for the device time, host form for the host time;
    (i)          `match_list_top_sections[_device]` alone: the difference to (new) is the cost of the positions;
    (ii)         what a caller has without the feature and without bias or scope: `match_list_top_sections`, then `match_list_indices` over
                 the concatenated heads - two calls, two waits (host forms only: the second call needs the first one's result on the host);
    (iii)        S x (`set_scope(require, exclude)` + `match_list_top_indices[_device](20)`);
    (top)        one unsectioned `match_list_top_indices[_device](20)`: the yardstick of S = 1.
Two figures per row, microseconds per call (per S calls for (iii)): `device_us` - between two events around back-to-back calls - for the
rows made of `_device` forms, and `host_us` - wall clock from the first enqueue to the result on the host (host forms; one wait per call, two
for (ii)) - for the rows made of host forms.  The variants alternate repeat by repeat, each on its own reserved matcher over the same corpus;
the median of `--repeats` repeats and [lowest, highest], one JSON line per row.  `--check` (the default) holds the new call's records against
a numpy model over the full index-ordered `match_list` and its positions against `match_list_indices` over the model's heads before anything
is timed.

    python tools/bench_sections_indices.py [--calls 50] [--repeats 9] [--lists fixed10M,paths1.4M] [--no-check]
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
import torch  # noqa: E402
from bench_sections import LIMIT, SECTIONS, model, the_list  # noqa: E402

import frizbee_amd as F  # noqa: E402

DEVICE_ROWS = ("new", "i", "iii", "top")
HOST_ROWS = ("new", "i", "ii", "iii", "top")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lists", default="fixed10M,paths1.4M")
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    cfg = F.Config(pf_lanes=64, sw_lanes=64, sort=F.SortStrategy.ScoreThenIndexAsc)
    for name in a.lists.split(","):
        data, ends, needle = the_list(name)
        n, stride = len(ends), len(needle)
        tags = np.random.default_rng(7).integers(0, 65536, n).astype(np.uint16)
        cp = F.Corpus(packed=(data, ends))
        cp.set_tags(tags)
        out = torch.zeros((8 * LIMIT + 8) * 16, dtype=torch.uint8, device="cuda")
        pos = torch.zeros((8 * LIMIT + 8) * stride, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(24, dtype=torch.int32, device="cuda")
        run = {v: F.Matcher(needle, cfg) for v in set(DEVICE_ROWS) | set(HOST_ROWS)}
        for m in run.values():
            m.reserve(cp)
            m.reserve_top_indices(cp, 8 * LIMIT, stride)

        def device_call(v, sections):
            S = len(sections)
            if v == "new":
                run[v].match_list_top_sections_indices_device(cp, sections, LIMIT, out.data_ptr(), S * LIMIT, pos.data_ptr(), S * LIMIT * stride, cnt.data_ptr())
            elif v == "i":
                run[v].match_list_top_sections_device(cp, sections, LIMIT, out.data_ptr(), S * LIMIT, cnt.data_ptr())
            elif v == "top":
                run[v].match_list_top_indices_device(cp, LIMIT, out.data_ptr(), LIMIT, pos.data_ptr(), LIMIT * stride, cnt.data_ptr())
            else:
                for require, exclude in sections:
                    cp.set_scope(require, exclude)
                    run[v].match_list_top_indices_device(cp, LIMIT, out.data_ptr(), LIMIT, pos.data_ptr(), LIMIT * stride, cnt.data_ptr())
                cp.set_scope(0, 0)

        def host_call(v, sections):
            if v == "new":
                return run[v].match_list_top_sections_indices(cp, sections, LIMIT)
            if v == "i":
                return run[v].match_list_top_sections(cp, sections, LIMIT)
            if v == "top":
                return run[v].match_list_top_indices(cp, LIMIT)
            if v == "ii":
                heads = run[v].match_list_top_sections(cp, sections, LIMIT)
                sel = np.concatenate([r["index"] for r, _ in heads]).astype(np.uint32)
                return heads, run[v].match_list_indices(cp, selection=sel)
            got = []
            for require, exclude in sections:
                cp.set_scope(require, exclude)
                got.append(run[v].match_list_top_indices(cp, LIMIT))
            cp.set_scope(0, 0)
            return got

        if not a.no_check:
            index_cfg = F.Config(pf_lanes=64, sw_lanes=64, sort=F.SortStrategy.IndexAsc)
            full = F.Matcher(needle, index_cfg).match_list(cp)
            for S, sections in SECTIONS.items():
                want = model(full, tags, sections, LIMIT)
                got = host_call("new", sections)
                for s, ((head, found), (recs, f)) in enumerate(zip(want, got)):
                    assert f == found and [(m.index, m.score, m.exact) for m in recs] == [(int(r["index"]), int(r["score"]), bool(r["exact"])) for r in head], (name, S, s)
                    if len(head):  # positions: the list-order call over the model's head, one haystack per index
                        ref = F.Matcher(needle, index_cfg).match_list_indices(cp, selection=head["index"].astype(np.uint32))
                        assert [m.indices for m in recs] == [m.indices for m in ref], (name, S, s, "positions")
                device_call("new", sections)
                torch.cuda.synchronize()
                words = cnt.tolist()
                kept = [len(h) for h, _ in want]
                assert words[0:2 * S:2] == kept and words[1:2 * S:2] == [f for _, f in want] and words[2 * S] == sum(kept) and words[2 * S + 3] == 0, (name, S, words)
                dev = out.cpu().numpy()[: sum(kept) * 16].view(F.MATCH_INDICES_DTYPE)
                assert dev["index"].tolist() == [int(i) for h, _ in want for i in h["index"]] and int(words[2 * S + 2]) == int(dev["positions_len"].sum()), (name, S, "device form")
            print(json.dumps(dict(list=name, check="heads == numpy model, positions == match_list_indices over the heads", matches=len(full))), flush=True)

        rows = [(kind, v, S) for S in SECTIONS for kind, names in (("device", DEVICE_ROWS), ("host", HOST_ROWS)) for v in names if v != "top" or S == 1]
        times = {r: [] for r in rows}
        for rep in range(a.warmup + a.repeats):
            for kind, v, S in rows:
                torch.cuda.synchronize()
                if kind == "device":
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.calls):
                        device_call(v, SECTIONS[S])
                    e1.record()
                    e1.synchronize()
                    t = e0.elapsed_time(e1) * 1e3 / a.calls
                else:
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        host_call(v, SECTIONS[S])
                    t = (time.perf_counter() - t0) * 1e6 / a.calls
                if rep >= a.warmup:
                    times[(kind, v, S)].append(t)
        torch.cuda.synchronize()
        med = {r: float(np.median(t)) for r, t in times.items()}
        for (kind, v, S), t in times.items():
            print(json.dumps({"list": name, "items": n, "needle": needle, "variant": v, "sections": S, "limit": LIMIT, "calls": a.calls, "repeats": a.repeats,
                              kind + "_us": round(med[(kind, v, S)], 1), "spread_us": [round(min(t), 1), round(max(t), 1)]}), flush=True)
        for S in SECTIONS:
            print(json.dumps(dict(list=name, sections=S, positions_cost_device_us=round(med[("device", "new", S)] - med[("device", "i", S)], 1),
                                  host_new_us=round(med[("host", "new", S)], 1), host_two_calls_us=round(med[("host", "ii", S)], 1),
                                  host_scoped_calls_us=round(med[("host", "iii", S)], 1), beats_two_calls=bool(med[("host", "new", S)] < med[("host", "ii", S)]),
                                  beats_scoped_calls=bool(med[("host", "new", S)] < med[("host", "iii", S)]))), flush=True)
        over = med[("device", "new", 1)] - med[("device", "top", 1)]
        print(json.dumps(dict(list=name, target="S = 1 within 2 x 3.8 us of match_list_top_indices_device", new_us=round(med[("device", "new", 1)], 1),
                              top_indices_us=round(med[("device", "top", 1)], 1), over_us=round(over, 1), met=bool(over <= 7.6))), flush=True)
        del run, cp


if __name__ == "__main__":
    main()
