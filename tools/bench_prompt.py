"""What the picker's first frame costs - the empty prompt, `Matcher("").match_list_top(corpus, 100)` over a corpus with a score bias, an
active scope or a candidate set: host-clock timing from the call to the synchronised result on the host, limit 100, on the first 200 000
paths of the paths-shaped list, on the whole list (1.4 M) and on 10 M uniform haystacks of 32 bytes:
    (a) `Matcher("")` over a biased corpus ("most frecent first");
    (b) the same with a scope that hides half of the list ("the visible files");
    (c) the same over `Subset.from_scope`, one haystack in twenty, + the bias ("this folder");
    (d) `MultiMatcher([])` over the corpus of (a) and of (b): the composition's no-pattern path - identity records, the scope drop,
        k_bias_apply, the top stage - which does the same job with more launches; reported as (d/a) and (d/b);
    (e) the biased one-letter query `s`, for scale: what every keystroke after the first frame costs.
The rows ALTERNATE query by query inside one process (drift of a shared host hits all alike); every row keeps its own reserved matcher.
It warms up first; then `--repeats` repeats of `--queries` queries per row and list: the median of the repeats' medians and their spread
(lowest and highest repeat median), microseconds, one JSON line per list and row.  `--check` compares (a) to (c) with a numpy model at the
timed sizes before anything is timed.  Uses the host forms only, so it runs on a commit from before the device-side prompt as well.

    python tools/bench_prompt.py [--queries 50] [--repeats 5] [--check] [--only a|b|c|da|db|e] [--lists 200k,1.4M,10M]
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

LIMIT = 100
HALF = (0, 1)  # (require, exclude): tag bit 0 hides a haystack
FOLDER = (2, 0)  # tag bit 1: "this folder", one in twenty
NAMES = {"a": "(a) Matcher('') over bias", "b": "(b) Matcher('') over bias + scope hiding half", "c": "(c) Matcher('') over Subset.from_scope (1 in 20) + bias",
         "da": "(d/a) MultiMatcher([]) over bias", "db": "(d/b) MultiMatcher([]) over bias + scope hiding half", "e": "(e) biased one-letter query 's'"}


def model(n, bias, keep, limit):
    """ScoreThenIndexAsc over the kept haystacks: (the first `limit` records, found)"""
    idx = np.flatnonzero(keep) if keep is not None else np.arange(n)
    s = np.clip(bias[idx].astype(np.int64), 0, 65535)
    order = np.argsort(-s, kind="stable")[:limit]
    out = np.zeros(len(order), F.MATCH_DTYPE)
    out["index"], out["score"] = idx[order], s[order]
    return out, len(idx)


def build(name):
    if name == "10M":
        rows, ends = synth.fixed_corpus(b"deadbe", 10_000_000, 32, seed=7)
        return (rows.numpy().reshape(-1), ends), 10_000_000, "uniform 10M x 32 B"
    data, ends = synth.paths_corpus()
    n = {"200k": 200_000, "1.4M": len(ends)}[name]
    return (data[: int(ends[n - 1])], ends[:n]), n, "paths " + name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=50, help="timed queries per repeat, row and list")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5, help="untimed queries per row")
    ap.add_argument("--check", action="store_true", help="rows (a) to (c) against a numpy model, before anything is timed")
    ap.add_argument("--only", choices=tuple(NAMES), default=None, help="one row alone (what a kernel trace is taken of)")
    ap.add_argument("--lists", default="200k,1.4M,10M")
    a = ap.parse_args()
    rows = [r for r in NAMES if a.only in (None, r)]
    for name in a.lists.split(","):
        packed, n, title = build(name)
        rng = np.random.default_rng(7)
        bias = rng.integers(-40, 41, n).astype(np.int16)  # frecency of a few dozen
        bias = np.where(rng.random(n) < 0.02, 300, bias).astype(np.int16)  # "file is open": across 256
        tags = ((rng.random(n) < 0.5).astype(np.uint16) | ((rng.random(n) < 0.05).astype(np.uint16) << 1)).astype(np.uint16)
        plain, scoped = F.Corpus(packed=packed), F.Corpus(packed=packed)
        for cp in (plain, scoped):
            cp.set_bias(bias)
            cp.set_tags(tags)
        scoped.set_scope(*HALF)
        folder = F.Subset(plain)
        folder.from_scope(*FOLDER)
        cfg = F.Config(pf_lanes=64, sw_lanes=64)
        empty = {r: F.Matcher("", cfg) for r in "abc"}
        multi = {r: F.MultiMatcher([], cfg) for r in ("da", "db")}
        letter = F.Matcher("s", cfg)
        corpus = {"a": plain, "b": scoped, "c": plain, "da": plain, "db": scoped, "e": plain}
        for r, m in list(empty.items()) + list(multi.items()) + [("e", letter)]:
            m.reserve(corpus[r])
        run = {
            "a": lambda: empty["a"].match_list_top(plain, LIMIT, copy=False),
            "b": lambda: empty["b"].match_list_top(scoped, LIMIT, copy=False),
            "c": lambda: empty["c"].match_list_top(plain, LIMIT, copy=False, subset=folder),
            "da": lambda: multi["da"].match_list_top(plain, LIMIT, copy=False),
            "db": lambda: multi["db"].match_list_top(scoped, LIMIT, copy=False),
            "e": lambda: letter.match_list_top(plain, LIMIT, copy=False),
        }
        if a.check:
            for r, keep in (("a", None), ("b", (tags & 1) == 0), ("c", (tags & 2) != 0), ("da", None), ("db", (tags & 1) == 0)):
                if r in rows:
                    got, found = run[r]()
                    want, visible = model(n, bias, keep, LIMIT)
                    assert found == visible and got.tolist() == want.tolist(), (title, r, found, visible)
            print(json.dumps(dict(list=title, items=n, check="rows a, b, c and d equal the numpy model")), flush=True)
        for _ in range(max(a.warmup, 1)):
            for r in rows:
                run[r]()
        medians = {r: [] for r in rows}
        for _ in range(a.repeats):
            t = {r: [] for r in rows}
            for _q in range(a.queries):
                for r in rows:
                    t0 = time.perf_counter()
                    run[r]()
                    t[r].append((time.perf_counter() - t0) * 1e6)
            for r in rows:
                medians[r].append(float(np.median(t[r])))
        for r in rows:
            m = medians[r]
            print(json.dumps(dict(list=title, items=n, limit=LIMIT, row=NAMES[r], queries=a.queries * a.repeats, median_us=round(float(np.median(m)), 1),
                                  spread_us=[round(min(m), 1), round(max(m), 1)], repeat_medians_us=[round(x, 1) for x in m])), flush=True)
        del run, empty, multi, letter, folder, plain, scoped, corpus


if __name__ == "__main__":
    main()
