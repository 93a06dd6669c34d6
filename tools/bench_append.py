"""Ingesting a list in batches: `Corpus.append` against what a frozen corpus forces (a fresh upload of everything seen so far after
every batch) and against the floor (one upload of the complete list), on the paths-shaped 1.4 M-item list, in batches of 4 096 and
65 536; then the query times on the appended corpus against a freshly uploaded copy of the same list - and, as the control that says how
much two equivalent corpora differ anyway, a SECOND fresh upload - with the three corpora alternated inside one process.  Host clock,
milliseconds / microseconds, medians with the 10th / 90th percentiles; one JSON line per figure.

    python tools/bench_append.py [--calls 200] [--small] [--no-reupload]     (--small: a tenth of the list)
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


def batches(data, ends, size):
    """[(bytes of the batch (+ a byte of slack), its end offsets counted from its first byte)]"""
    res, n = [], len(ends)
    for lo in range(0, n, size):
        hi = min(n, lo + size)
        b0 = int(ends[lo - 1]) if lo else 0
        res.append((np.ascontiguousarray(data[b0:int(ends[hi - 1]) + 1]), (ends[lo:hi] - np.uint64(b0)).astype(np.uint64)))
    return res


def pct(ts):
    return dict(median=round(float(np.median(ts)), 3), p10=round(float(np.percentile(ts, 10)), 3), p90=round(float(np.percentile(ts, 90)), 3))


def ingest(data, ends, size, reupload):
    n = len(ends)
    parts = batches(data, ends, size)
    t0 = time.perf_counter()
    whole = F.Corpus(packed=(data, ends))
    floor_ms = (time.perf_counter() - t0) * 1e3
    del whole
    for reserve in (False, True):
        cp = F.Corpus([])
        if reserve:
            cp.reserve(n, int(ends[-1]) + 15 * n)
        per = []
        t0 = time.perf_counter()
        for b, e in parts:
            t1 = time.perf_counter()
            cp.append(packed=(b, e))
            per.append((time.perf_counter() - t1) * 1e3)
        total = (time.perf_counter() - t0) * 1e3
        info = cp.info()
        out(measure="ingest", items=n, batch=size, batches=len(parts), variant="append" + (" (reserved)" if reserve else ""), total_ms=round(total, 2),
            per_batch_ms=pct(per), regrows=info["regrows"], has_view=info["has_view"], floor_one_upload_ms=round(floor_ms, 2))
        del cp
    if reupload:
        per = []
        t0 = time.perf_counter()
        for k in range(len(parts)):
            hi = min(n, (k + 1) * size)
            t1 = time.perf_counter()
            cp = F.Corpus(packed=(data[:int(ends[hi - 1]) + 1], ends[:hi]))
            per.append((time.perf_counter() - t1) * 1e3)
            del cp
        out(measure="ingest", items=n, batch=size, batches=len(parts), variant="re-upload everything after each batch", total_ms=round((time.perf_counter() - t0) * 1e3, 2),
            per_batch_ms=pct(per), floor_one_upload_ms=round(floor_ms, 2))


def queries(data, ends, size, calls):
    cps = {"appended": F.Corpus([]), "fresh": F.Corpus(packed=(data, ends)), "fresh (control)": F.Corpus(packed=(data, ends))}
    for b, e in batches(data, ends, size):
        cps["appended"].append(packed=(b, e))
    m = F.Matcher("linux", F.Config(pf_lanes=64, sw_lanes=64))
    for cp in cps.values():
        m.reserve(cp)
    want = m.match_list(cps["fresh"])
    assert m.match_list(cps["appended"]).tolist() == want.tolist()
    for title, fn in (("match_list_top(100)", lambda cp: m.match_list_top(cp, 100, copy=False)), ("match_list", lambda cp: m.match_list(cp, copy=False))):
        t = {k: [] for k in cps}
        for it in range(calls + 10):
            for k, cp in cps.items():
                t0 = time.perf_counter()
                fn(cp)
                if it >= 10:
                    t[k].append((time.perf_counter() - t0) * 1e6)
        for k in cps:
            out(measure="query", query=title, batch=size, corpus=k, found=len(want), us=pct(t[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-reupload", action="store_true", help="skip the re-upload variant (O(batches x n): the slow one)")
    a = ap.parse_args()
    n = 1_406_941 // (10 if a.small else 1)
    data, ends = synth.paths_corpus(b"linux", n)
    data = np.ascontiguousarray(np.concatenate([np.asarray(data, np.uint8).reshape(-1), np.zeros(1, np.uint8)]))
    ends = np.asarray(ends, np.uint64)
    F.Corpus(packed=(data, ends))  # warm-up: the runtime's first allocation and copy
    for size in (4096, 65536):
        ingest(data, ends, size, not a.no_reupload)
    for size in (4096, 65536):
        queries(data, ends, size, a.calls)


if __name__ == "__main__":
    main()
