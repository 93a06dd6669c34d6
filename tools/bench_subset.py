"""What a candidate set (`Subset`, `Matcher.match_list_top_device(subset=..., capture=...)`) costs and gains per query.  Every time is a DEVICE
time: two events on the query's stream around `--iters` back-to-back calls of the asynchronous `_device` form (no host wait inside the
window), divided by the calls; variants that are compared ALTERNATE repeat by repeat inside one process; `--repeats` repeats, the median
and the spread (lowest and highest repeat) in microseconds.  Three parts, one JSON line per row, a header line with the GPU and the ROCm
version:

  filter     the two item-list filters behind the SAME narrowed call - same corpus, same item list, same needle, only the filter kernel
             differs (k1_items under FZB_NO_ITEMS_DFA=1, k1_items_dfa through the fzb_debug_set_items_dfa_min hook), so the difference of
             the two call times is the difference of the two kernels - for 1 k .. 5 M candidates drawn evenly from the 10 M x 32-byte list
             (with and without letter signatures) and from the paths-shaped list (1.4 M).  The crossover goes into
             FZB_ITEMS_DFA_MIN_SHORT / _RAGGED (kernels_filter.hip).
  keystroke  the prefixes of the needle typed one letter at a time, limit 100: the whole-list call (`subset=None`: what the parent commit
             runs), the same with a capture, and the call narrowed to the previous keystroke's capture (capturing again), with the
             candidate count and fraction beside it.  NarrowingMatcher.DEFAULT_MAX_FRACTION = 0.8 x the largest fraction at which the
             narrowed call was not slower than the whole-list call.
  scope      profiles/scope.txt's rows as device times - the scoped query (the drop pass behind the scorers), a second corpus of the visible
             haystacks alone - and a third column: the query over `Subset.from_scope` at the same visibility (half, one in twenty).

Before anything is timed every narrowed result is checked against the whole-list call's.

    python tools/bench_subset.py [--parts filter,keystroke,scope] [--iters 50] [--repeats 5] [--lists fixed10M,paths1.4M] [--items-dfa-min N]
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
from bench_scope import sub_packed, the_list  # noqa: E402

LIMIT = 100


def knobs(no_items_dfa=False, items_dfa_min=0, no_signature=False):
    for name, on in (("FZB_NO_ITEMS_DFA", no_items_dfa), ("FZB_NO_SIGNATURE", no_signature)):
        if on:
            os.environ[name] = "1"
        else:
            os.environ.pop(name, None)
    F.lib().fzb_debug_set_items_dfa_min(items_dfa_min)
    F.lib().fzb_debug_reload_knobs()


class Call:
    """one `match_list_top_device` call with its own output buffers"""

    def __init__(self, m, cp, subset=None, capture=None):
        self.m, self.cp, self.subset, self.capture = m, cp, subset, capture
        self.out = torch.zeros((LIMIT + 1) * 8, dtype=torch.uint8, device="cuda")
        self.cnt = torch.zeros(4, dtype=torch.int32, device="cuda")

    def __call__(self):
        self.m.match_list_top_device(self.cp, LIMIT, self.out.data_ptr(), LIMIT, self.cnt.data_ptr(), subset=self.subset, capture=self.capture)

    def result(self):
        self()
        torch.cuda.synchronize()
        w = self.cnt.tolist()
        return self.out.cpu().numpy()[: w[0] * 8].view(F.MATCH_DTYPE).copy(), w[1]


def device_us(fn, iters, before=None):
    if before:
        before()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters


def alternate(variants, iters, repeats):
    """variants: name -> (fn, before); returns name -> (median, lowest, highest) over the repeats, the variants taking turns"""
    t = {k: [] for k in variants}
    names = list(variants)
    for r in range(repeats):
        for k in names[r % len(names):] + names[:r % len(names)]:
            fn, before = variants[k]
            t[k].append(device_us(fn, iters, before))
    return {k: (round(float(np.median(v)), 1), round(min(v), 1), round(max(v), 1)) for k, v in t.items()}


def emit(**row):
    print(json.dumps(row), flush=True)


def part_filter(a, name, cfg):
    for no_sig in ((False, True) if name == "fixed10M" else (False,)):
        knobs(no_signature=no_sig)
        data, ends, needle, _ = the_list(name)
        cp = F.Corpus(packed=(data, ends))
        n = len(cp)
        m = F.Matcher(needle, cfg)
        m.reserve(cp)
        sub = F.Subset(cp)
        whole = Call(m, cp)
        for k in (1_000, 10_000, 100_000, 1_000_000, 5_000_000):
            if k > n:
                continue
            idx = np.unique(np.linspace(0, n - 1, k).astype(np.uint32))
            sub.set_indices(idx)
            call = Call(m, cp, subset=sub)
            knobs(no_items_dfa=True, no_signature=no_sig)
            want = call.result()
            knobs(items_dfa_min=1, no_signature=no_sig)
            got = call.result()
            assert got[1] == want[1] and got[0].tolist() == want[0].tolist(), (name, k)
            r = alternate({"k1_items": (call, lambda: knobs(no_items_dfa=True, no_signature=no_sig)), "k1_items_dfa": (call, lambda: knobs(items_dfa_min=1, no_signature=no_sig)),
                           "whole_list": (whole, None)}, a.iters, a.repeats)
            emit(part="filter", list=name, items=n, signatures=bool(cp.signature_info()[0]), needle=needle, candidates=len(idx), found=want[1], iters=a.iters, repeats=a.repeats,
                 narrowed_call_k1_items_us=r["k1_items"], narrowed_call_k1_items_dfa_us=r["k1_items_dfa"], whole_list_call_us=r["whole_list"],
                 kernel_difference_us=round(r["k1_items"][0] - r["k1_items_dfa"][0], 1))
        del sub, m, cp
    knobs()


def part_keystroke(a, name, cfg):
    knobs(items_dfa_min=a.items_dfa_min)
    data, ends, needle, _ = the_list(name)
    cp = F.Corpus(packed=(data, ends))
    n = len(cp)
    m = F.Matcher(needle[:1], cfg)
    m.reserve(cp)
    prev, cur = F.Subset(cp), F.Subset(cp)
    best = 0.0
    for k in range(1, len(needle) + 1):
        m.set_pattern(needle[:k])
        whole, with_capture = Call(m, cp), Call(m, cp, capture=cur)
        want = whole.result()
        variants = {"whole_list": (whole, None), "whole_list_with_capture": (with_capture, None)}
        candidates = None
        if k > 1:
            narrowed = Call(m, cp, subset=prev, capture=cur)
            got = narrowed.result()
            assert got[1] == want[1] and got[0].tolist() == want[0].tolist(), (name, needle[:k])
            variants["narrowed"] = (narrowed, None)
            candidates = len(prev)
        r = alternate(variants, a.iters, a.repeats)
        if candidates is not None and r["narrowed"][0] <= r["whole_list"][0]:
            best = max(best, candidates / n)
        emit(part="keystroke", list=name, items=n, needle=needle[:k], limit=LIMIT, found=want[1], candidates=candidates, fraction=None if candidates is None else round(candidates / n, 4),
             iters=a.iters, repeats=a.repeats, whole_list_us=r["whole_list"], whole_list_with_capture_us=r["whole_list_with_capture"], narrowed_us=r.get("narrowed"))
        with_capture.result()  # the capture the next keystroke narrows from
        prev, cur = cur, prev
    emit(part="keystroke", list=name, largest_fraction_not_slower=round(best, 4), max_fraction_candidate=round(0.8 * best, 4))
    knobs()


def part_scope(a, name, cfg):
    knobs(items_dfa_min=a.items_dfa_min)
    data, ends, needle, row = the_list(name)
    n = len(ends)
    rng = np.random.default_rng(7)
    tags = ((rng.random(n) < 0.5).astype(np.uint16)) | ((rng.random(n) >= 0.05).astype(np.uint16) << 1)  # bench_scope's: bit 0 = outside the half, bit 1 = outside the 1 in 20
    cp = F.Corpus(packed=(data, ends))
    cp.set_tags(tags)
    m = F.Matcher(needle, cfg)
    m.reserve(cp)
    sub = F.Subset(cp)
    for label, exclude in (("half visible", 1), ("1 in 20 visible", 2)):
        vis = (tags & exclude) == 0
        second = F.Corpus(packed=sub_packed(data, ends, vis, row))
        m2 = F.Matcher(needle, cfg)
        m2.reserve(second)
        sub.from_scope(0, exclude)
        assert len(sub) == int(vis.sum())
        scoped, own, over = Call(m, cp), Call(m2, second), Call(m, cp, subset=sub)
        cp.set_scope(0, exclude)
        want = scoped.result()
        cp.set_scope(0, 0)
        got = over.result()
        assert got[1] == want[1] and got[0].tolist() == want[0].tolist(), (name, label)
        r = alternate({"scoped": (scoped, lambda: cp.set_scope(0, exclude)), "second_corpus": (own, None), "from_scope": (over, lambda: cp.set_scope(0, 0))}, a.iters, a.repeats)
        emit(part="scope", list=name, items=n, needle=needle, visibility=label, visible=int(vis.sum()), found=want[1], iters=a.iters, repeats=a.repeats, scoped_query_us=r["scoped"],
             second_corpus_of_the_visible_us=r["second_corpus"], query_over_subset_from_scope_us=r["from_scope"])
        del second, m2
    cp.set_scope(0, 0)
    knobs()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="filter,keystroke,scope")
    ap.add_argument("--iters", type=int, default=50, help="back-to-back calls between the two events")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lists", default="fixed10M,paths1.4M")
    ap.add_argument("--items-dfa-min", type=int, default=0, help="the keystroke and scope parts: k1_items_dfa from this many candidates on (0: the library's default)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_subset.py measures device times: it needs the GPU")
    emit(gpu=torch.cuda.get_device_name(0), rocm=torch.version.hip, torch=torch.__version__, iters=a.iters, repeats=a.repeats, limit=LIMIT, items_dfa_min=a.items_dfa_min,
         timing="device events around back-to-back match_list_top_device calls; median [lowest, highest] of the repeats, us")
    cfg = F.Config(pf_lanes=64, sw_lanes=64, sort=F.SortStrategy.ScoreThenIndexAsc)
    for name in a.lists.split(","):
        for part in a.parts.split(","):
            dict(filter=part_filter, keystroke=part_keystroke, scope=part_scope)[part](a, name, cfg)


if __name__ == "__main__":
    main()
