"""What an any-of group (`a | b`) costs: `match_list_top_device(100)` of a grouped `MultiMatcher`, ScoreThenIndexAsc, for a group alone
(`rs$ | py$ | go$` ...) and for a group between a base pattern and a negated one (`linux rs$ | py$ !test` ...), at 2, 4 and 8 alternatives, on
the paths-shaped list (1.4 M, literal suffixes) and on the 10 M x 32-byte list (fuzzy `dead | beef | cafe` ...).  Per row, measured in the
same run on the same build:
    (grouped)   ONE grouped call - device time between two events around back-to-back calls, and the host form's wall time per call;
    (singles)   the sum of k single-pattern `match_list_top_device(100)` calls, one per alternative: a LOWER BOUND that does no union;
    (host)      what a caller without the feature does: k full `match_list` calls (every match over PCIe), a numpy union by index with
                max, the other terms applied the same way, a stable argsort and a cut - wall time.
The variants alternate repeat by repeat; the median of `--repeats` repeats and [lowest, highest], microseconds, one JSON line per row.
`--check` (the default) holds the device's head and `found` against that numpy union before anything is timed.

    python tools/bench_anyof.py [--calls 20] [--repeats 7] [--lists paths1.4M,fixed10M] [--no-check]
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

LIMIT = 100
KS = (2, 4, 8)
ALTS = {
    "paths1.4M": ["rs$", "py$", "go$", "md$", "cc$", "js$", "ts$", "sh$"],
    "fixed10M": ["dead", "beef", "cafe", "dbe", "ead", "deb", "adb", "eadb"],
}
AROUND = {"paths1.4M": ("linux", "!test"), "fixed10M": ("de", "!zq")}  # (base pattern, negated pattern) of the second query


def the_list(name):
    if name == "fixed10M":
        rows, ends = synth.fixed_corpus(b"deadbe", 10_000_000, 32)
        return rows.numpy().reshape(-1), ends
    return synth.paths_corpus()


def queries(name):
    """[(label, query text)]"""
    out = []
    for k in KS:
        group = " | ".join(ALTS[name][:k])
        out.append(("group", k, group))
        out.append(("and_not", k, "%s %s %s" % (AROUND[name][0], group, AROUND[name][1])))
    return out


def solo_matchers(cp, cfg_asc, pats):
    """one IndexAsc matcher per pattern, its negation dropped: what the emulation keeps between keystrokes"""
    return [F.MultiMatcher([F.Pattern(p.needle, matching=p.matching)], cfg_asc) for p in pats]  # (their buffers are made in the warm-up repeat)


def host_union(cp, solo, pats, group_of):
    """the emulation: one full match_list per pattern, composed by index in numpy -> the index-ordered records"""
    n = len(cp)
    score = np.zeros(n, np.int64)
    exact = np.zeros(n, bool)
    alive = np.ones(n, bool)
    terms = {}
    for p, g, m in zip(pats, group_of, solo):
        terms.setdefault(g, []).append((p, m))
    for g in sorted(terms):
        key = np.zeros(n, np.int64)  # 0 = no hit; else 1 << 17 | score << 1 | exact: the maximum is the rule
        negated = terms[g][0][0].negated
        for p, m in terms[g]:
            r = m.match_list(cp)
            k = (1 << 17) | (r["score"].astype(np.int64) << 1) | r["exact"]
            key[r["index"]] = np.maximum(key[r["index"]], k)
        hit = key != 0
        if negated:
            alive &= ~hit
        else:
            alive &= hit
            score = np.minimum(score + ((key >> 1) & 0xFFFF), 65535)
            exact |= (key & 1).astype(bool)
    idx = np.flatnonzero(alive)
    out = np.zeros(len(idx), F.MATCH_DTYPE)
    out["index"], out["score"], out["exact"] = idx, score[idx], exact[idx]
    return out


def head_of(index_asc, limit):
    return index_asc[np.argsort(-index_asc["score"].astype(np.int64), kind="stable")][:limit]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls between the two events")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lists", default="paths1.4M,fixed10M")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="skip the host emulation's timing (it copies every match of every alternative)")
    a = ap.parse_args()
    cfg = F.Config(pf_lanes=64, sw_lanes=0, sort=F.SortStrategy.ScoreThenIndexAsc)
    cfg_asc = F.Config(pf_lanes=64, sw_lanes=0, sort=F.SortStrategy.IndexAsc)
    out = torch.zeros((LIMIT + 8) * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(16, dtype=torch.int32, device="cuda")
    for name in a.lists.split(","):
        data, ends = the_list(name)
        cp = F.Corpus(packed=(data, ends))
        n = len(cp)
        for label, k, text in queries(name):
            pats, group_of = F.parse_query_groups(text)
            assert max(group_of.count(g) for g in group_of) == k, (text, group_of)
            grouped = F.MultiMatcher(pats, cfg, groups=group_of)
            grouped.reserve(cp)
            alts = [p for p, g in zip(pats, group_of) if group_of.count(g) > 1]
            singles = [F.MultiMatcher([p], cfg) for p in alts]
            solo = solo_matchers(cp, cfg_asc, pats)
            if not a.no_check:
                want = host_union(cp, solo, pats, group_of)
                grouped.match_list_top_device(cp, LIMIT, out.data_ptr(), LIMIT, cnt.data_ptr())
                torch.cuda.synchronize()
                words = cnt.tolist()
                got = out.cpu().numpy()[: words[0] * 8].view(F.MATCH_DTYPE)
                assert words[1] == len(want) and got.tolist() == head_of(want, LIMIT).tolist(), (name, text, words[:2], len(want), got[:3], head_of(want, 3))
                recs, found = grouped.match_list_top(cp, LIMIT)
                assert found == len(want) and recs.tolist() == head_of(want, LIMIT).tolist(), (name, text, "host form")
                print(json.dumps(dict(list=name, query=text, check="device head == numpy union", found=len(want))), flush=True)

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
                "grouped_device": lambda: device_us(lambda: grouped.match_list_top_device(cp, LIMIT, out.data_ptr(), LIMIT, cnt.data_ptr())),
                "grouped_host": lambda: wall_us(lambda: grouped.match_list_top(cp, LIMIT), a.calls),
                "singles_device": lambda: device_us(lambda: [m.match_list_top_device(cp, LIMIT, out.data_ptr(), LIMIT, cnt.data_ptr()) for m in singles]),
                "singles_host": lambda: wall_us(lambda: [m.match_list_top(cp, LIMIT) for m in singles], a.calls),
            }
            if not a.no_host:
                variants["host_union"] = lambda: wall_us(lambda: head_of(host_union(cp, solo, pats, group_of), LIMIT), 1)
            times = {v: [] for v in variants}
            for rep in range(a.warmup + a.repeats):
                for v, fn in variants.items():
                    t = fn()
                    if rep >= a.warmup:
                        times[v].append(t)
            for v, t in times.items():
                print(json.dumps(dict(list=name, items=n, query=text, form=label, alternatives=k, variant=v, limit=LIMIT, calls=a.calls, repeats=a.repeats,
                                      median_us=round(float(np.median(t)), 1), spread_us=[round(min(t), 1), round(max(t), 1)])), flush=True)
            del grouped, singles, solo
        del cp


if __name__ == "__main__":
    main()
