"""Editing a resident list: `Corpus.remove` / `Corpus.replace` against the only route a corpus that cannot be edited offers for the same
edit - free it and upload the edited list again - on the C2 list (10 M x 32 bytes) and on the paths-shaped 1.4 M-item list: removing one
item, a random 1 %, a random 50 % and a contiguous 10 % at the front, and replacing 1 000 random items.  After each edit the query times
on the edited corpus against a freshly uploaded copy of the edited list - and, as the control that says how much two equivalent corpora
differ anyway, a SECOND fresh upload - with the three corpora alternated inside one process.  Host clock, milliseconds / microseconds,
medians with the 10th / 90th percentiles; one JSON line per figure.  (Every repetition of an edit starts from a fresh upload of the
unedited list, which is not timed.)

    python tools/bench_corpus_edit.py [--reps 7] [--calls 200] [--small] [--lists c2,paths]     (--small: a tenth of each list)
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


def out(**kw):
    print(json.dumps(kw), flush=True)


def pct(ts):
    return dict(median=round(float(np.median(ts)), 3), p10=round(float(np.percentile(ts, 10)), 3), p90=round(float(np.percentile(ts, 90)), 3))


def slack(data):
    return np.ascontiguousarray(np.concatenate([data, np.zeros(1, np.uint8)]))


def removed(data, ends, drop):
    """the upload format of the list without the haystacks `drop`"""
    keep = np.ones(len(ends), bool)
    keep[drop] = False
    lens = np.diff(ends, prepend=np.uint64(0)).astype(np.int64)
    return slack(data[:int(ends[-1])][np.repeat(keep, lens)]), np.cumsum(lens[keep], dtype=np.uint64)


def replaced(data, ends, at, new_data, new_ends):
    """the upload format of the list with haystack at[k] = item k of the batch"""
    order = np.argsort(at)
    lens = np.diff(ends, prepend=np.uint64(0)).astype(np.int64)
    nlens = np.diff(new_ends, prepend=np.uint64(0)).astype(np.int64)
    parts, prev = [], 0
    for k in order:
        i = int(at[k])
        parts.append(data[prev:int(ends[i]) - int(lens[i])])
        b0 = int(new_ends[k]) - int(nlens[k])
        parts.append(new_data[b0:b0 + int(nlens[k])])
        prev = int(ends[i])
    parts.append(data[prev:int(ends[-1])])
    lens[at] = nlens
    return slack(np.concatenate(parts)), np.cumsum(lens, dtype=np.uint64)


def edits(data, ends, rng):
    n = len(ends)
    yield "remove 1 item", dict(drop=np.array([n // 2], np.uint32))
    yield "remove a random 1 %", dict(drop=rng.choice(n, n // 100, replace=False).astype(np.uint32))
    yield "remove a random 50 %", dict(drop=rng.choice(n, n // 2, replace=False).astype(np.uint32))
    yield "remove the first 10 %", dict(drop=np.arange(n // 10, dtype=np.uint32))
    # 1 000 items take the content of 1 000 others (on the ragged list: other lengths)
    at, src = rng.choice(n, 1000, replace=False).astype(np.uint32), rng.choice(n, 1000, replace=False)
    lens = np.diff(ends, prepend=np.uint64(0)).astype(np.int64)
    batch = np.concatenate([data[int(ends[i]) - int(lens[i]):int(ends[i])] for i in src])
    yield "replace 1 000 random items", dict(at=at, batch=(slack(batch), np.cumsum(lens[src], dtype=np.uint64)))


def run(name, data, ends, needle, reps, calls):
    rng = np.random.default_rng(7)
    m = F.Matcher(needle, F.Config(pf_lanes=64, sw_lanes=64))
    F.Corpus(packed=(data, ends))  # warm-up: the runtime's first allocation and copy
    for title, e in edits(data, ends, rng):
        if "drop" in e:
            new = removed(data, ends, e["drop"])
            apply = lambda cp: cp.remove(e["drop"])  # noqa: E731
        else:
            new = replaced(data, ends, e["at"], *e["batch"])
            apply = lambda cp: cp.replace(e["at"], packed=e["batch"])  # noqa: E731
        t_edit, t_up = [], []
        for _ in range(reps):
            cp = F.Corpus(packed=(data, ends))
            t0 = time.perf_counter()
            apply(cp)
            t_edit.append((time.perf_counter() - t0) * 1e3)
            ei = cp.edit_info()
            del cp
            cp = F.Corpus(packed=(data, ends))
            t0 = time.perf_counter()
            del cp  # fzb_corpus_free + fzb_corpus_upload of the edited list
            cp = F.Corpus(packed=new)
            t_up.append((time.perf_counter() - t0) * 1e3)
            del cp
        out(measure="edit", list=name, items=len(ends), edit=title, edit_ms=pct(t_edit), reupload_ms=pct(t_up), speedup=round(float(np.median(t_up) / np.median(t_edit)), 2),
            first=ei["first"], bytes_written=ei["bytes_written"], view_tiles=ei["view_tiles"], temp_bytes=ei["temp_bytes"])
        cps = {"edited": F.Corpus(packed=(data, ends)), "fresh": F.Corpus(packed=new), "fresh (control)": F.Corpus(packed=new)}
        apply(cps["edited"])
        for cp in cps.values():
            m.reserve(cp)
        want = m.match_list(cps["fresh"])
        assert len(cps["edited"]) == len(new[1]) and m.match_list(cps["edited"]).tolist() == want.tolist(), title
        for query, fn in (("match_list_top(100)", lambda cp: m.match_list_top(cp, 100, copy=False)), ("match_list", lambda cp: m.match_list(cp, copy=False))):
            t = {k: [] for k in cps}
            for it in range(calls + 10):
                for k, cp in cps.items():
                    t0 = time.perf_counter()
                    fn(cp)
                    if it >= 10:
                        t[k].append((time.perf_counter() - t0) * 1e6)
            for k in cps:
                out(measure="query", list=name, edit=title, query=query, corpus=k, found=len(want), us=pct(t[k]))
        del cps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--lists", default="c2,paths")
    a = ap.parse_args()
    import torch
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    div = 10 if a.small else 1
    if "c2" in a.lists.split(","):
        rows, ends = synth.fixed_corpus(b"deadbe", 10_000_000 // div, 32, device=dev)
        run("C2 (32-byte haystacks)", slack(rows.cpu().numpy().reshape(-1)), np.asarray(ends, np.uint64), "deadbe", a.reps, a.calls)
    if "paths" in a.lists.split(","):
        data, ends = synth.paths_corpus(b"linux", 1_406_941 // div, device=dev)
        run("paths", slack(np.asarray(data, np.uint8).reshape(-1)), np.asarray(ends, np.uint64), "linux", a.reps, a.calls)


if __name__ == "__main__":
    main()
