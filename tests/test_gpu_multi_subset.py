"""Candidate sets on the `from_patterns` forms (fzb_multi_match_list_subset and its siblings): a query-syntax query over a device-resident
subset of a corpus, and the capture of the COMPOSITION's match set.  The contract is the subset's sentence unchanged: the query over subset S
returns what it returns over an upload of the haystacks of S alone, every index mapped back to the full list's.  So every expected value is
`O.MultiMatcher` over the sub-list plus the (monotone) index map - with the bias and the reference's ordering rule added in numpy where a
bias is present -; never this library's own unrestricted result."""
import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from test_gpu_scope import mapped, mapped_indices, sub_list, top_indices_tuples, visible
from test_gpu_score_bias import biased, same
from test_gpu_small_device import device_of
from test_gpu_subset import N, Lists, device_top, filter_kernel, mask_of, subsets, unpack  # noqa: F401  (unpack: the lists' maker)
from test_gpu_topk import SORTS, assert_top, limits_around

pytestmark = pytest.mark.gpu
SHAPES = ("empty", "first", "all", "run_1025", "clustered_50", "random_quarter")
UNI = "إن"
# name -> the oracle's patterns (parse_query strings unless noted)
QUERIES = {
    "two": O.parse_query("dead be"), "base_negated": O.parse_query("dead !be"), "single": O.parse_query("deadbe"), "single_negated": O.parse_query("!de"),
    "all_negated": O.parse_query("!de !ad"), "literal": O.parse_query("^d be$"), "typo": [O.P("deadbe", max_typos=1), O.P("ad", negated=True)],
    "unicode": O.parse_query(UNI), "none": O.parse_query(""),
}
CASES = [(w, q) for w in ("uniform32", "paths") for q in QUERIES if q != "unicode"] + [("utf8", "unicode"), ("utf8", "none"), ("utf8", "all_negated")]


def hip_patterns(opats):
    return [F.Pattern(p["needle"], negated=p["negated"], max_typos=None if p["max_typos"] == O.INHERIT else p["max_typos"],
                      matching=None if p.get("matching") is None else F.Matching[p["matching"]]) for p in opats]


def pair(opats, sort="ScoreThenIndexAsc"):
    """(HIP matcher, oracle matcher) of one pattern list under one sort"""
    return F.MultiMatcher(hip_patterns(opats), F.Config(sort=F.SortStrategy[sort], pf_lanes=64)), O.MultiMatcher(opats, lanes=(64, 64, 32), sort=sort)


_WANT = {}


def oracle_over(which, qname, sname, sort):
    """the oracle over the sub-list, mapped back: (records in `sort` order, ordered matched-indices items); computed once per key"""
    key = (which, qname, sname, sort)
    if key not in _WANT:
        hs = Lists.get(which)
        vis = mask_of(subsets(len(hs))[sname], len(hs))
        lst = sub_list(hs, vis)
        om = O.MultiMatcher(QUERIES[qname], lanes=(64, 64, 32), sort=sort)
        recs = mapped(om.match_list(lst), vis) if lst else np.zeros(0, F.MATCH_DTYPE)
        items = mapped_indices(om.match_list_indices_ordered(lst), vis) if lst else []
        _WANT[key] = (recs, items)
    return _WANT[key]


def test_every_query_says_something():
    """for every query but the one without a pattern, the oracle's result over the whole list is neither empty nor the whole list on some list"""
    for qname in QUERIES:
        if qname == "none":
            continue
        sizes = [len(oracle_over(w, qname, "all", "IndexAsc")[0]) for w, q in CASES if q == qname]
        assert any(0 < s < N for s in sizes), (qname, sizes)


@pytest.mark.parametrize("which,qname", CASES)
def test_every_form_over_subsets_equals_the_oracle_over_the_sub_list(which, qname):
    hs = Lists.get(which)
    cp = F.Corpus(hs)
    sub, cap = F.Subset(cp), F.Subset(cp)
    for sname in SHAPES:
        idx = subsets(len(hs))[sname]
        sub.set_indices(idx)
        # all four sorts on one list and the two shapes with many records; the default elsewhere
        sorts = SORTS if which == "uniform32" and sname in ("all", "random_quarter") else ("ScoreThenIndexAsc",)
        for sort in sorts:
            ctx = (which, qname, sname, sort)
            fm = pair(QUERIES[qname], sort)[0]
            want, items = oracle_over(which, qname, sname, sort)
            found = len(want)
            captured = np.sort(want["index"]).astype(np.uint32)
            same(fm.match_list(cp, subset=sub, capture=cap), want, ctx)
            info = cap.info()
            assert info["known"] == 1 and info["count"] == found and np.array_equal(cap.read(), captured), (ctx, info, "capture of match_list")
            for limit in limits_around(found):
                assert_top(fm.match_list_top(cp, limit, subset=sub, capture=cap), want, limit, ctx)
                assert np.array_equal(cap.read(), captured), (ctx, limit, "capture of match_list_top")  # whatever the limit and the sort
                recs, nfound = fm.match_list_top_indices(cp, limit, subset=sub)
                assert nfound == found and top_indices_tuples(recs) == items[:limit], (ctx, limit)
            recs, nfound = fm.match_list_top_indices(cp, 3, subset=sub, capture=cap)
            assert nfound == found and cap.info()["known"] == 1 and np.array_equal(cap.read(), captured), (ctx, "capture of top_indices")
            if qname == "none":
                with pytest.raises(F.FrizbeeError, match="no pattern") as e:
                    device_top(fm, cp, 5, subset=sub)
                assert e.value.code == 1
                continue
            limit = max(1, found // 2)
            got, words = device_top(fm, cp, limit, subset=sub, capture=cap)
            assert words[:2] == [min(limit, found), found] and words[2:] == [-1, -1], (ctx, words)
            same(got, want[:limit], (ctx, "device"))
            assert cap.info()["known"] == 0  # the _device form leaves the count on the device ...
            assert len(cap) == found and np.array_equal(cap.read(), captured), (ctx, "capture of the _device form")  # ... until it is asked for


def test_the_item_list_filter_kernels_agree_under_a_composition():
    """the base pattern's 0-typo ASCII pipeline over a candidate set takes either item-list filter: the same records and capture"""
    hs = Lists.get("uniform32")
    cp = F.Corpus(hs)
    sub, cap = F.Subset(cp), F.Subset(cp)
    sub.set_indices(subsets(len(hs))["random_quarter"])
    want = oracle_over("uniform32", "base_negated", "random_quarter", "ScoreThenIndexAsc")[0]
    for kernel in ("items", "items_dfa"):
        with filter_kernel(kernel):
            fm = pair(QUERIES["base_negated"])[0]
            same(fm.match_list(cp, subset=sub, capture=cap), want, kernel)
            assert np.array_equal(cap.read(), np.sort(want["index"])), kernel


def test_the_fused_capture_equals_the_two_launches():
    """a composition captures in the launch that writes its final records; the hook restores the copy and the capture as two launches: the
    same records, counts and capture, on a plain and on a scoped corpus"""
    hs = Lists.get("uniform32")
    rng = np.random.default_rng(3)
    tags = rng.integers(0, 2, len(hs)).astype(np.uint16)
    with device_of(2):
        cp = F.Corpus(hs)
        cp.set_tags(tags)
        sub, cap = F.Subset(cp), F.Subset(cp)
        sub.set_indices(subsets(len(hs))["random_quarter"])
        try:
            for qname in ("two", "base_negated", "all_negated", "typo"):
                for exclude in (0, 1):
                    cp.set_scope(0, exclude)
                    seen = {}
                    for fused in (1, 0):
                        F.lib().fzb_debug_set_fused_capture(fused)
                        fm = pair(QUERIES[qname])[0]
                        F.launch_grids()
                        recs = fm.match_list(cp, subset=sub, capture=cap)
                        grids = F.launch_grids()
                        info = cap.info()
                        top = fm.match_list_top(cp, 10, subset=sub, capture=cap)
                        seen[fused] = (recs.tobytes(), info, cap.read().tobytes(), top[0].tobytes(), top[1], cap.info())
                        names = {"k_copy_capture_records"} if fused else {"k_copy_records", "k_subset_capture"}
                        assert names <= set(grids) and not ({"k_copy_capture_records", "k_copy_records", "k_subset_capture"} - names) & set(grids), (qname, fused, sorted(grids))
                    assert seen[0] == seen[1] and seen[1][1]["known"] == 1, (qname, exclude)
                    want = oracle_over("uniform32", qname, "random_quarter", "ScoreThenIndexAsc")[0]
                    assert np.array_equal(np.frombuffer(seen[1][2], np.uint32), np.sort(want["index"])), (qname, exclude)
        finally:
            F.lib().fzb_debug_set_fused_capture(1)


@pytest.mark.parametrize("qname", ("base_negated", "all_negated", "none"))
@pytest.mark.parametrize("sort", SORTS)
def test_bias_and_scope_on_top_of_a_subset(sort, qname):
    """subset ∩ visible with a bias crossing 256: the oracle over visible ∩ S, bias and ordering in numpy; the capture is what the composition
    accepted inside the subset, whatever the terms, the limit and the sort"""
    hs = Lists.get("uniform32")
    n = len(hs)
    rng = np.random.default_rng(31)
    tags = rng.integers(0, 4, n).astype(np.uint16)
    bias = rng.choice([0, 200, -32768, -5, 7], n).astype(np.int16)
    idx = np.flatnonzero(rng.random(n) < 0.5)
    in_sub, vis = mask_of(idx, n), visible(tags, 0, 1)
    both = in_sub & vis
    om = O.MultiMatcher(QUERIES[qname], lanes=(64, 64, 32), sort="IndexAsc")
    want = biased(mapped(om.match_list(sub_list(hs, both)), both), bias, sort)
    accepted = np.sort(mapped(om.match_list(sub_list(hs, in_sub)), in_sub)["index"]).astype(np.uint32)
    assert len(want) > 20 and int(want["score"].max()) >= 200 and len(accepted) > len(want)
    cp = F.Corpus(hs)
    cp.set_bias(bias)
    cp.set_tags(tags)
    cp.set_scope(exclude=1)
    sub, cap = F.Subset(cp), F.Subset(cp)
    sub.set_indices(idx)
    fm = pair(QUERIES[qname], sort)[0]
    same(fm.match_list(cp, subset=sub, capture=cap), want, (qname, sort))
    assert np.array_equal(cap.read(), accepted)
    for limit in limits_around(len(want)):
        assert_top(fm.match_list_top(cp, limit, subset=sub, capture=cap), want, limit, (qname, sort))
        assert np.array_equal(cap.read(), accepted), (qname, sort, limit)
    recs, nfound = fm.match_list_top_indices(cp, 7, subset=sub, capture=cap)
    assert nfound == len(want) and [(m.index, m.score) for m in recs] == [(int(r["index"]), int(r["score"])) for r in want[:7]], (qname, sort)
    assert np.array_equal(cap.read(), accepted)
    cp.set_scope(0, 0)
    cp.set_bias(None)
    fm.match_list_top(cp, 1, subset=sub, capture=cap)
    assert np.array_equal(cap.read(), accepted)  # unchanged by limit, sort, bias and scope


def test_a_capture_is_the_input_of_the_next_query():
    """two chained steps, `dead` -> `dead be` -> `dead be !ad`: each runs over the previous capture and equals the oracle over the ORIGINAL list"""
    for which in ("uniform32", "paths"):
        hs = Lists.get(which)
        cp = F.Corpus(hs)
        a, b = F.Subset(cp), F.Subset(cp)
        fm = F.MultiMatcher([], F.Config(pf_lanes=64))
        src, dst = None, a
        for q in ("dead", "dead be", "dead be !ad"):
            fm.set_patterns(q)
            fresh = O.MultiMatcher(O.parse_query(q), lanes=(64, 64, 32)).match_list(hs)
            assert_top(fm.match_list_top(cp, 100, subset=src, capture=dst), fresh, 100, (which, q))
            assert dst.info()["known"] == 1 and np.array_equal(dst.read(), np.sort(fresh["index"])), (which, q)
            same(fm.match_list(cp, subset=dst), fresh, (which, q, "over its own capture"))
            src, dst = dst, (b if dst is a else a)
        assert len(fresh) > 5, which


def test_refusals_launch_nothing():
    hs = Lists.get("uniform32")
    import torch

    with device_of(2):  # (launches are recorded only under the small-device switch)
        cp, other = F.Corpus(hs), F.Corpus(hs)
        s, t, foreign = F.Subset(cp), F.Subset(cp), F.Subset(other)
        s.set_indices([1, 5, 9])
        foreign.set_indices([1, 2])
        fm = pair(QUERIES["base_negated"])[0]
        fm.match_list(cp, subset=s, capture=t)
        buf, ends = torch.zeros(256, dtype=torch.uint8, device="cuda"), torch.tensor([16, 32, 48, 64], dtype=torch.int32, device="cuda")
        borrowed = F.Corpus.from_device(buf.data_ptr(), ends.data_ptr(), 4, 64, keep=(buf, ends))

        def forms(cp_, **kw):
            return (lambda: fm.match_list(cp_, **kw), lambda: fm.match_list_top(cp_, 3, **kw), lambda: fm.match_list_top_indices(cp_, 3, **kw),
                    lambda: device_top(fm, cp_, 3, **kw))

        def refused(calls, match):
            torch.cuda.synchronize()
            F.launch_grids()
            for call in calls:
                with pytest.raises(F.FrizbeeError, match=match) as e:
                    call()
                assert e.value.code == 1
            assert F.launch_grids() == {}, match

        refused(forms(cp, subset=foreign), "stale")
        refused(forms(cp, capture=foreign), "subset")
        refused(forms(cp, subset=s, capture=s), "capture")
        refused(forms(borrowed, subset=s), "borrows")
        refused(forms(borrowed, capture=t), "borrows")
        cp.append(["deadbeef"])
        refused(forms(cp, subset=s), "stale")
        fm.match_list(cp, capture=s)  # a capture takes the current generation
        assert s.info()["generation"] == cp.generation()
        fm.match_list(cp, subset=s, capture=t)


def test_no_device_allocation_after_reserve():
    hs = Lists.get("paths")
    n = len(hs)
    cp = F.Corpus(hs)
    cp.reserve(2 * n, 400 * n)
    cp.set_tags(np.zeros(n, np.uint16))
    fm = F.MultiMatcher(F.parse_query("dead be !ad"), F.Config(pf_lanes=64))
    fm.reserve(cp)
    fm.reserve_top_indices(cp, 100, 8)
    a, b = F.Subset(cp), F.Subset(cp)
    import torch

    out = torch.zeros(101 * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    fm.match_list(cp), fm.match_list_top(cp, 100), fm.match_list_top_indices(cp, 100)  # (the lazily made page-locked buffers)
    before = F.device_allocs()
    a.from_scope(0, 1)
    src, dst = a, b
    for q in ("dead be !ad", "de ad !x", "!de !ad", "deadbe", "d !e !a"):  # never more than three patterns
        fm.set_patterns(q)
        for call in (lambda: fm.match_list(cp, subset=src, capture=dst), lambda: fm.match_list_top(cp, 100, subset=src, capture=dst),
                     lambda: fm.match_list_top_indices(cp, 100, subset=src, capture=dst),
                     lambda: fm.match_list_top_device(cp, 100, out.data_ptr(), 100, cnt.data_ptr(), subset=src, capture=dst)):
            at = F.device_allocs()
            call()
            torch.cuda.synchronize()
            assert F.device_allocs() == at, (q, "a subset query allocated device memory after the reserves")
        cp.set_scope(0, 1 if q == "de ad !x" else 0)
        src, dst = (None if q == "!de !ad" else dst), (a if dst is b else b)
    assert F.device_allocs() == before


def test_without_a_subset_the_launches_are_those_of_the_plain_call():
    hs = Lists.get("uniform32")
    import torch

    with device_of(2):
        cp = F.Corpus(hs)
        for qname in ("two", "base_negated", "single", "all_negated", "none"):
            fm = pair(QUERIES[qname])[0]
            record = []
            for call in (lambda: fm.match_list_top(cp, 10), lambda: fm.match_list_top(cp, 10, subset=None, capture=None),
                         lambda: F._top(F.lib().fzb_multi_match_list_top, fm.h, cp.h, 10, True),
                         lambda: fm.match_list_top_indices(cp, 10), lambda: fm.match_list_top_indices(cp, 10, subset=None, capture=None)):
                torch.cuda.synchronize()
                F.launch_grids()
                call()
                record.append(F.launch_grids())
            assert record[0] == record[1] == record[2] and (record[0] or qname == "none"), (qname, record[:3])
            assert record[3] == record[4], (qname, record[3:])
            # and through the C entry point itself with in == NULL and no capture
            out, cnt, found = F.C.c_void_p(), F.C.c_size_t(), F.C.c_uint64()
            F.launch_grids()
            F._check(F.lib().fzb_multi_match_list_top_subset(fm.h, cp.h, None, None, 10, F.C.byref(out), F.C.byref(cnt), F.C.byref(found)))
            assert F.launch_grids() == record[0], qname
            F._take(out, cnt)


@pytest.mark.parametrize("cus", (1, 2))
def test_on_a_small_device(cus):
    """a device of 1 and 2 compute units: the same results, and the identity step over the items takes more than one trip of its loop"""
    hs = Lists.get("uniform32")
    with device_of(cus):
        cp = F.Corpus(hs)
        sub, cap = F.Subset(cp), F.Subset(cp)
        sub.set_indices(np.arange(N))
        for qname in ("all_negated", "base_negated"):
            fm = pair(QUERIES[qname])[0]
            want, items = oracle_over("uniform32", qname, "all", "ScoreThenIndexAsc")
            F.launch_grids()
            same(fm.match_list(cp, subset=sub, capture=cap), want, (cus, qname))
            grids = F.launch_grids()
            assert np.array_equal(cap.read(), np.sort(want["index"])), (cus, qname)
            assert_top(fm.match_list_top(cp, 50, subset=sub), want, 50, (cus, qname))
            recs, nfound = fm.match_list_top_indices(cp, 50, subset=sub)
            assert nfound == len(want) and top_indices_tuples(recs) == items[:50], (cus, qname)
            print("grids", cus, qname, grids)
            for k in ("k_items_records",) if qname == "all_negated" else ():
                assert k in grids and grids[k][1] * 256 < N, (cus, qname, k, grids.get(k))  # grid x 256 threads < items: a second trip
            k = "k_copy_capture_records"  # the composition's final copy and the capture, one launch
            assert k in grids and "k_subset_capture" not in grids and "k_copy_records" not in grids, (cus, qname, sorted(grids))
            assert grids[k][1] * 256 < N and (qname != "all_negated" or grids[k][1] * 256 < len(want)), (cus, qname, grids[k], len(want))


def test_narrowing_query():
    hs = Lists.get("uniform32")
    n = len(hs)
    cp = F.Corpus(hs)
    assert F.NarrowingQuery.DEFAULT_MAX_FRACTION == 0.0 or 0 < F.NarrowingQuery.DEFAULT_MAX_FRACTION <= 1
    folder = mask_of(subsets(n)["random_quarter"], n)
    within = F.Subset(cp)
    within.set_indices(np.flatnonzero(folder))
    cfg = F.Config(pf_lanes=64)
    nq, never, inside = F.NarrowingQuery(cp, cfg, max_fraction=1.0), F.NarrowingQuery(cp, cfg, max_fraction=0.0), F.NarrowingQuery(cp, cfg, max_fraction=1.0, within=within)
    steps = ("dead b", "dead be", "dead be !", "dead be !a", "dead be !ad")
    expect = [False, True, False, True, False]  # (`dead be !`: the empty needle is dropped, nothing changed; `!a` -> `!ad`: a changed negated atom)
    seen, seen_inside = [], []
    for q in steps:
        om = O.MultiMatcher(O.parse_query(q), lanes=(64, 64, 32))
        want = om.match_list(hs)
        assert_top(nq.query(q, 50), want, 50, q)
        seen.append(nq.last_narrowed)
        assert_top(never.query(q, 50), want, 50, q)
        assert never.last_narrowed is False
        want_in = mapped(om.match_list(sub_list(hs, folder)), folder)
        got = inside.query(q, 50)
        assert_top(got, want_in, 50, (q, "within"))
        assert folder[got[0]["index"]].all(), q  # never an index outside the folder, narrowed or not
        seen_inside.append(inside.last_narrowed)
    assert seen == expect and seen_inside == expect, (seen, seen_inside)
    # with positions, and a step that is no refinement after one that is
    for q, narrowed in (("de", False), ("dea", True), ("dea !x", True), ("de !x", False)):
        recs, found = inside.query(q, 5, indices=True)
        om = O.MultiMatcher(O.parse_query(q), lanes=(64, 64, 32))
        items = mapped_indices(om.match_list_indices_ordered(sub_list(hs, folder)), folder)
        assert found == len(items) and top_indices_tuples(recs) == items[:5] and inside.last_narrowed is narrowed, (q, inside.last_narrowed)
    # a change of `within` (identity) invalidates the previous capture
    inside.query("dead", 5)
    other = F.Subset(cp)
    other.set_indices(np.flatnonzero(folder)[::2])
    inside.within = other
    got = inside.query("deadb", 50)
    assert inside.last_narrowed is False and np.isin(got[0]["index"], np.flatnonzero(folder)[::2]).all()
