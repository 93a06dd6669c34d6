"""Candidate sets (fzb_subset): queries over a device-resident subset of a corpus and the capture of a query's match set.  The contract is
the scope's sentence restated for a set: a query over subset S returns what the same query returns over an upload of the haystacks of S
alone, in their order, with every index mapped back to the full list's.  So every expected value here is the ORACLE's result over the
sub-list plus the (monotone) index map - with the bias and the reference's ordering rule added in numpy where a bias is present - or plain
numpy; never this library's own unrestricted result.  Every 0-typo ASCII case runs through both item-list filter kernels (k1_items under
FZB_NO_ITEMS_DFA=1, k1_items_dfa through the fzb_debug_set_items_dfa_min hook)."""
import contextlib
import os
import sys

import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from test_gpu_parity import LANES
from test_gpu_scope import mapped, mapped_indices, sub_list, top_indices_tuples, visible
from test_gpu_score_bias import biased, same
from test_gpu_topk import SORTS, assert_top, limits_around, single

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
N = 3 * 1024 + 37


def unpack(data, ends):
    raw = np.asarray(data, np.uint8).tobytes()
    out, start = [], 0
    for e in np.asarray(ends).tolist():
        out.append(raw[start:e])
        start = e
    return out


class Lists:
    _made = {}

    @classmethod
    def get(cls, name):
        if name not in cls._made:
            cls._made[name] = getattr(cls, "_" + name)()
        return cls._made[name]

    @staticmethod
    def _uniform32():
        rows, ends = synth.fixed_corpus(b"deadbe", N, 32, seed=11)
        return unpack(rows.numpy().reshape(-1), ends)

    @staticmethod
    def _ragged32():
        return unpack(*synth.ragged_corpus(b"deadbe", N, 1, 32, seed=12))

    @staticmethod
    def _paths():
        hs = unpack(*synth.ragged_corpus(b"deadbe", N, 8, 250, seed=13))
        rng = np.random.default_rng(13)
        for i in rng.choice(N, 6, replace=False).tolist():  # a few beyond 256 bytes: the view's outliers
            hs[i] = (hs[i] * 40)[: int(rng.integers(257, 301))]
        return hs

    @staticmethod
    def _utf8():
        return unpack(*synth.utf8_corpus(N, 32, seed=14))

    @staticmethod
    def _long():
        return unpack(*synth.ragged_corpus(b"deadbeef" * 10, 512 + 5, 100, 200, seed=15, full=0.3))


def subsets(n):
    rng = np.random.default_rng(n)
    inside = 1024 + np.sort(rng.choice(1000, 50, replace=False))
    return {"empty": np.zeros(0, np.uint32), "first": np.array([0]), "last": np.array([n - 1]), "all": np.arange(n), "every_third": np.arange(0, n, 3),
            "run_1024": np.arange(100, 100 + min(1024, n - 100)), "run_1025": np.arange(7, 7 + min(1025, n - 7)), "clustered_50": inside[inside < n],
            "random_quarter": np.flatnonzero(rng.random(n) < 0.25)}


MATCHERS = {
    "ascii_0": ("deadbe", {}), "ascii_0_upper_smart": ("deaDbe", dict(casing="Smart")), "unicode_0": ("إن", {}), "typo_1": ("deadbe", dict(max_typos=1)),
    "typos_none": ("db", dict(max_typos=None)), "substring": ("de", dict(matching="Substring")), "prefix": ("d", dict(matching="Prefix")),
}
ZERO_TYPO_ASCII = ("ascii_0", "ascii_0_upper_smart")


@contextlib.contextmanager
def filter_kernel(which):
    """which item-list filter a candidate set's 0-typo ASCII query takes: 'items' = k1_items (FZB_NO_ITEMS_DFA=1), 'items_dfa' = k1_items_dfa
    from one item on (the test hook)"""
    old = os.environ.get("FZB_NO_ITEMS_DFA")
    try:
        if which == "items":
            os.environ["FZB_NO_ITEMS_DFA"] = "1"
        else:
            os.environ.pop("FZB_NO_ITEMS_DFA", None)
            F.lib().fzb_debug_set_items_dfa_min(1)
        F.lib().fzb_debug_reload_knobs()
        yield
    finally:
        if old is None:
            os.environ.pop("FZB_NO_ITEMS_DFA", None)
        else:
            os.environ["FZB_NO_ITEMS_DFA"] = old
        F.lib().fzb_debug_set_items_dfa_min(0)
        F.lib().fzb_debug_reload_knobs()


def mask_of(idx, n):
    m = np.zeros(n, bool)
    m[np.asarray(idx, np.int64)] = True
    return m


def device_top(fm, cp, limit, subset=None, capture=None):
    import torch

    cap = min(limit, len(cp))
    out = torch.zeros((cap + 1) * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    fm.match_list_top_device(cp, limit, out.data_ptr(), cap, cnt.data_ptr(), subset=subset, capture=capture)
    torch.cuda.synchronize()
    words = cnt.tolist()
    return out.cpu().numpy()[: words[0] * 8].view(F.MATCH_DTYPE), words


def check_subset(hs, cp, sub, cap, idx, needle, cfg, pf, name, sorts=SORTS):
    """every form over one subset of one list with one matcher configuration; returns the number of matches"""
    vis = mask_of(idx, len(hs))
    lst = sub_list(hs, vis)
    sub.set_indices(idx)
    found = 0
    for sort in sorts:
        fm, om = single(needle, sort=sort, pf=pf, **cfg)
        want = mapped(om.match_list(lst), vis) if lst else np.zeros(0, F.MATCH_DTYPE)
        found = len(want)
        captured = np.sort(want["index"]).astype(np.uint32)
        same(fm.match_list(cp, subset=sub, capture=cap), want, (name, sort))
        info = cap.info()
        assert info["known"] == 1 and info["count"] == found, (name, sort, info)
        assert np.array_equal(cap.read(), captured), (name, sort, "capture of match_list")
        items = mapped_indices(om.match_list_indices_ordered(lst), vis) if lst else []
        for limit in limits_around(found):
            assert_top(fm.match_list_top(cp, limit, subset=sub), want, limit, (name, sort))
            recs, nfound = fm.match_list_top_indices(cp, limit, subset=sub)
            assert nfound == found and top_indices_tuples(recs) == items[:limit], (name, sort, limit)
        limit = max(1, found // 2)
        got, words = device_top(fm, cp, limit, subset=sub, capture=cap)
        assert words[:2] == [min(limit, found), found] and words[2:] == [-1, -1], (name, sort, words)
        same(got, want[:limit], (name, sort, "device"))
        assert cap.info()["known"] == 0  # the _device form leaves the count on the device ...
        assert len(cap) == found and np.array_equal(cap.read(), captured), (name, sort, "capture of the _device form")  # ... until it is asked for
        recs, nfound = fm.match_list_top_indices(cp, 3, subset=sub, capture=cap)
        assert cap.info()["known"] == 1 and np.array_equal(cap.read(), captured), (name, sort, "capture of top_indices")
    return found


# (only fuzzy 0-typo ASCII queries choose between the two item-list filters: those cases run through both)
CASES = [(w, m, k) for w in ("uniform32", "ragged32", "paths", "utf8") for m in sorted(MATCHERS) for k in ("items", "items_dfa") if k == "items" or m in ZERO_TYPO_ASCII]


@pytest.mark.parametrize("which,matcher,kernel", CASES)
def test_queries_over_subsets_equal_the_oracle_over_the_sub_list(which, matcher, kernel):
    hs = Lists.get(which)
    needle, cfg = MATCHERS[matcher]
    cp = F.Corpus(hs)
    if which == "uniform32":
        assert cp.signature_info()[0]
    if which == "paths":
        assert cp.info()["has_view"] == 1
    sub, cap = F.Subset(cp), F.Subset(cp)
    total = 0
    with filter_kernel(kernel):
        for sname, idx in subsets(len(hs)).items():
            sorts = SORTS if sname in ("random_quarter", "every_third") else ("ScoreThenIndexAsc",)
            total += check_subset(hs, cp, sub, cap, idx, needle, cfg, 64, (which, matcher, kernel, sname), sorts)
    if matcher in ("ascii_0", "typo_1", "typos_none", "substring", "prefix") and which != "utf8":
        assert total > 20, (which, matcher, total)  # (the lists are planted with the ASCII needle)
    if (matcher, which) == ("unicode_0", "utf8"):
        assert total > 20


@pytest.mark.parametrize("kernel", ("items", "items_dfa"))
@pytest.mark.parametrize("pf", (32, 16))
def test_the_other_lane_pairs(pf, kernel):
    hs = Lists.get("uniform32")
    cp = F.Corpus(hs)
    sub, cap = F.Subset(cp), F.Subset(cp)
    idx = subsets(len(hs))["random_quarter"]
    with filter_kernel(kernel):
        for matcher in ("ascii_0", "typo_1", "typos_none"):
            needle, cfg = MATCHERS[matcher]
            assert check_subset(hs, cp, sub, cap, idx, needle, cfg, pf, (pf, matcher, kernel)) > 5


def test_a_long_needle_over_a_subset():
    hs = Lists.get("long")
    cp = F.Corpus(hs)
    sub, cap = F.Subset(cp), F.Subset(cp)
    needle = "deadbeef" * 10
    total = 0
    for sname in ("every_third", "random_quarter", "all", "empty"):
        total += check_subset(hs, cp, sub, cap, subsets(len(hs))[sname], needle, {}, 64, ("long", sname), ("ScoreThenIndexDesc",))
    assert total > 20


def test_both_filter_kernels_leave_the_same_records_counts_and_capture():
    for which in ("uniform32", "ragged32", "paths"):
        hs = Lists.get(which)
        cp = F.Corpus(hs)
        sub, cap = F.Subset(cp), F.Subset(cp)
        for sname, idx in subsets(len(hs)).items():
            sub.set_indices(idx)
            for needle in ("deadbe", "d", "eb"):
                got = {}
                for kernel in ("items", "items_dfa"):
                    with filter_kernel(kernel):
                        fm = F.Matcher(needle, F.Config(pf_lanes=64, sw_lanes=64, sort=F.SortStrategy.IndexAsc))
                        recs = fm.match_list(cp, subset=sub, capture=cap)
                        got[kernel] = (recs.tobytes(), fm.last_counters()["filter_survivors"], cap.read().tobytes(), fm.match_list_top(cp, 10, subset=sub)[1])
                assert got["items"] == got["items_dfa"], (which, sname, needle)


@pytest.mark.parametrize("sort", SORTS)
def test_bias_and_scope_on_top_of_a_subset(sort):
    """subset ∩ visible, a bias crossing 256; the capture is what the matcher accepted inside the subset, whatever the terms"""
    hs = Lists.get("uniform32")
    n = len(hs)
    rng = np.random.default_rng(31)
    tags = rng.integers(0, 4, n).astype(np.uint16)
    bias = rng.choice([0, 200, -32768, -5, 7], n).astype(np.int16)
    idx = np.flatnonzero(rng.random(n) < 0.5)
    in_sub, vis = mask_of(idx, n), visible(tags, 0, 1)
    both = in_sub & vis
    asc = mapped(O.Matcher("deadbe", sort="IndexAsc").match_list(sub_list(hs, both)), both)
    want = biased(asc, bias, sort)
    assert len(want) > 20 and int(want["score"].max()) >= 256
    accepted = np.sort(mapped(O.Matcher("deadbe", sort="IndexAsc").match_list(sub_list(hs, in_sub)), in_sub)["index"]).astype(np.uint32)
    cp = F.Corpus(hs)
    cp.set_bias(bias)
    cp.set_tags(tags)
    cp.set_scope(exclude=1)
    sub, cap = F.Subset(cp), F.Subset(cp)
    sub.set_indices(idx)
    fm = F.Matcher("deadbe", F.Config(sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=64))
    same(fm.match_list(cp, subset=sub, capture=cap), want, sort)
    assert np.array_equal(cap.read(), accepted) and len(accepted) > len(want)
    for limit in limits_around(len(want)):
        assert_top(fm.match_list_top(cp, limit, subset=sub, capture=cap), want, limit, sort)
        assert np.array_equal(cap.read(), accepted), (sort, limit)  # unchanged by limit, sort, bias and scope
    cp.set_scope(0, 0)
    cp.set_bias(None)
    fm.match_list_top(cp, 1, subset=sub, capture=cap)
    assert np.array_equal(cap.read(), accepted)


def test_capture_of_the_whole_list_and_a_narrowing_chain():
    hs = Lists.get("ragged32")
    n = len(hs)
    cp = F.Corpus(hs)
    a, b = F.Subset(cp), F.Subset(cp)
    for kernel in ("items", "items_dfa"):
        with filter_kernel(kernel):
            fm = F.Matcher("d", F.Config(pf_lanes=64, sw_lanes=64))
            src, dst, prev = None, a, np.ones(n, bool)
            for needle in ("d", "de", "dea", "dead", "deadb", "deadbe"):
                fm.set_pattern(needle)
                om = O.Matcher(needle)
                fresh = om.match_list(hs)
                want = mapped(om.match_list(sub_list(hs, prev)), prev)  # over the previous capture: the same records, by the premise
                assert want.tolist() == fresh.tolist()
                assert_top(fm.match_list_top(cp, 100, subset=src, capture=dst), fresh, 100, (kernel, needle))
                got = dst.read()
                assert dst.info()["known"] == 1 and np.array_equal(got, np.sort(fresh["index"])), (kernel, needle)
                prev = mask_of(got, n)
                src, dst = dst, (b if dst is a else a)
            assert prev.sum() > 10


def test_narrowing_matcher():
    hs = Lists.get("uniform32")
    cp = F.Corpus(hs)
    assert F.NarrowingMatcher.DEFAULT_MAX_FRACTION == 0.0 or 0 < F.NarrowingMatcher.DEFAULT_MAX_FRACTION <= 1
    nm = F.NarrowingMatcher(cp, F.Config(pf_lanes=64, sw_lanes=0), max_fraction=1.0)
    never = F.NarrowingMatcher(cp, F.Config(pf_lanes=64, sw_lanes=0), max_fraction=0.0)
    seen = []
    for needle in ("d", "de", "dea", "x", "dead", "deadb", "dea", "deaD", "deaDb", "deaDbé", "", "d"):
        want = O.Matcher(needle).match_list(hs)
        assert_top(nm.query(needle, 50), want, 50, needle)
        seen.append(nm.last_narrowed)
        assert_top(never.query(needle, 50), want, 50, needle)
        assert never.last_narrowed is False
        recs, found = nm.query(needle, 5, indices=True)  # the same needle again: not an extension, the whole list
        assert found == len(want) and nm.last_narrowed is False
        items = O.Matcher(needle).match_list_indices_ordered(hs)[:5]
        assert top_indices_tuples(recs) == items, needle
        assert_top(nm.query(needle, 50), want, 50, needle)
    # (every needle is queried three times; `seen` is the first of them: extensions narrow, anything else starts over)
    assert seen == [False, True, True, False, False, True, False, True, True, False, False, False], seen
    typo = F.NarrowingMatcher(cp, F.Config(pf_lanes=64, sw_lanes=0, max_typos=1), max_fraction=1.0)
    for needle in ("dead", "deadb"):
        assert_top(typo.query(needle, 50), O.Matcher(needle, max_typos=1).match_list(hs), 50, needle)
        assert typo.last_narrowed is False
    cp.append(["deadbeef"])
    want = O.Matcher("deadbe").match_list(hs + ["deadbeef"])
    nm.query("deadb", 10)
    assert_top(nm.query("deadbe", 50), want, 50, "after an append")
    assert nm.last_narrowed is True


@pytest.mark.parametrize("with_tags", (True, False))
def test_from_scope(with_tags):
    n = 5000
    hs = [b"a"] * n
    cp = F.Corpus(hs)
    tags = np.random.default_rng(12).integers(0, 16, n).astype(np.uint16) if with_tags else np.zeros(n, np.uint16)
    if with_tags:
        cp.set_tags(tags)
    s = F.Subset(cp)
    for require, exclude in ((1, 4), (8, 2), (0, 1), (0, 0), (6, 6)):
        s.from_scope(require, exclude)
        want = np.flatnonzero(visible(tags, require, exclude)).astype(np.uint32)
        info = s.info()
        assert info["known"] == 1 and info["count"] == len(want) and np.array_equal(s.read(), want), (require, exclude)
    if not with_tags:
        s.from_scope(0, 0)
        assert len(s) == n
        s.from_scope(1, 0)
        assert len(s) == 0
    # a query over the visible haystacks of a scope the corpus does NOT have set
    s.from_scope(0, 1)
    vis = visible(tags, 0, 1)
    fm, om = single("a")
    same(fm.match_list(cp, subset=s), mapped(om.match_list(sub_list(hs, vis)), vis), "from_scope")


def test_empty_needle_over_a_subset():
    hs = Lists.get("uniform32")
    n = len(hs)
    rng = np.random.default_rng(5)
    idx = np.flatnonzero(rng.random(n) < 0.3).astype(np.uint32)
    bias = rng.integers(-50, 300, n).astype(np.int16)
    tags = rng.integers(0, 2, n).astype(np.uint16)
    cp = F.Corpus(hs)
    sub, cap = F.Subset(cp), F.Subset(cp)
    sub.set_indices(idx)
    every = np.zeros(len(idx), F.MATCH_DTYPE)
    every["index"] = idx
    for sort in SORTS:
        fm = F.Matcher("", F.Config(sort=F.SortStrategy[sort], pf_lanes=64))
        cp.set_scope(0, 0)
        cp.set_bias(None)
        want = every[::-1].copy() if sort in ("IndexDesc", "ScoreThenIndexDesc") else every
        same(fm.match_list(cp, subset=sub, capture=cap), want, sort)
        assert np.array_equal(cap.read(), idx)
        assert_top(fm.match_list_top(cp, 10, subset=sub), want, 10, sort)
        cp.set_bias(bias)
        cp.set_tags(tags)
        cp.set_scope(exclude=1)
        shown = every[tags[idx] == 0]
        want = biased(shown, bias, sort)
        same(fm.match_list(cp, subset=sub), want, (sort, "terms"))
        for limit in (0, 7, len(want) + 1):
            assert_top(fm.match_list_top(cp, limit, subset=sub), want, limit, (sort, "terms"))
            recs, found = fm.match_list_top_indices(cp, limit, subset=sub)
            assert found == len(want) and top_indices_tuples(recs) == [(int(r["index"]), int(r["score"]), False, []) for r in want[:limit]]
    with pytest.raises(F.FrizbeeError, match="empty needle") as e:
        device_top(F.Matcher("", F.Config(pf_lanes=64)), cp, 5, subset=sub)
    assert e.value.code == 1


def test_refusals():
    hs = Lists.get("uniform32")
    n = len(hs)
    cp, other = F.Corpus(hs), F.Corpus(hs)
    s, t, foreign = F.Subset(cp), F.Subset(cp), F.Subset(other)
    s.set_indices([1, 5, 9])
    for bad, pos in (([3, 2, 7], 1), ([0, 4, 4], 2), ([0, n], 1), ([5, 6, 7, 6], 3)):
        with pytest.raises(F.FrizbeeError, match="position %d" % pos) as e:
            s.set_indices(bad)
        assert e.value.code == 1
        assert s.read().tolist() == [1, 5, 9]  # an error leaves the subset as it was
    fm = F.Matcher("deadbe", F.Config(pf_lanes=64, sw_lanes=64))
    foreign.set_indices([1, 2])
    for kw in (dict(subset=foreign), dict(capture=foreign)):
        with pytest.raises(F.FrizbeeError, match="subset") as e:
            fm.match_list_top(cp, 5, **kw)
        assert e.value.code == 1
    with pytest.raises(F.FrizbeeError, match="stale"):
        fm.match_list(cp, subset=foreign)
    for call in (lambda: fm.match_list(cp, subset=s, capture=s), lambda: fm.match_list_top(cp, 3, subset=s, capture=s), lambda: fm.match_list_top_indices(cp, 3, subset=s, capture=s)):
        with pytest.raises(F.FrizbeeError, match="capture") as e:
            call()
        assert e.value.code == 1
    import torch

    buf, ends = torch.zeros(256, dtype=torch.uint8, device="cuda"), torch.tensor([16, 32, 48, 64], dtype=torch.int32, device="cuda")
    borrowed = F.Corpus.from_device(buf.data_ptr(), ends.data_ptr(), 4, 64, keep=(buf, ends))
    with pytest.raises(F.FrizbeeError, match="borrows"):
        F.Subset(borrowed)
    # staleness: the calls that change the list bump the generation, the others do not
    g0 = cp.generation()
    cp.set_bias(np.zeros(n, np.int16))
    cp.set_tags(np.zeros(n, np.uint16))
    cp.set_scope(1, 0)
    cp.set_scope(0, 0)
    cp.set_bias(None)
    cp.reserve(2 * n, 64 * n)
    cp.truncate(n)      # changes nothing
    cp.remove([])       # changes nothing
    assert cp.generation() == g0
    assert len(fm.match_list(cp, subset=s)) >= 0  # still fresh
    edits = (lambda: cp.append(["deadbeef"]), lambda: cp.truncate(len(cp) - 1), lambda: cp.remove([3]), lambda: cp.replace([4], ["dead_be"]))
    for k, edit in enumerate(edits):
        s.set_indices([1, 5, 9])
        assert s.info()["generation"] == cp.generation()
        edit()
        assert cp.generation() == g0 + k + 1
        for call in (lambda: fm.match_list(cp, subset=s), lambda: fm.match_list_top(cp, 3, subset=s), lambda: fm.match_list_top_indices(cp, 3, subset=s),
                     lambda: device_top(fm, cp, 3, subset=s)):
            with pytest.raises(F.FrizbeeError, match="stale") as e:
                call()
            assert e.value.code == 1 and "subset" in str(e.value)
        fm.match_list(cp, capture=s)  # a capture takes the current generation
        assert s.info()["generation"] == cp.generation()
        fm.match_list(cp, subset=s, capture=t)


def test_no_device_allocation_after_reserve():
    hs = Lists.get("paths")
    n = len(hs)
    cp = F.Corpus(hs)
    cp.reserve(2 * n, 400 * n)
    cp.set_tags(np.zeros(n, np.uint16))
    fm = F.Matcher("deadbe", F.Config(pf_lanes=64, sw_lanes=64))
    fm.reserve(cp)
    fm.reserve_top_indices(cp, 100, 8)
    a, b = F.Subset(cp), F.Subset(cp)
    assert a.info()["capacity"] >= 2 * n
    import torch

    out = torch.zeros(101 * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    fm.match_list(cp), fm.match_list_top(cp, 100), fm.match_list_top_indices(cp, 100)  # (the lazily made page-locked buffers)
    with filter_kernel("items_dfa"):
        before = F.device_allocs()
        a.set_indices(np.arange(0, n, 2))
        a.from_scope(0, 1)
        src, dst = None, b
        for needle in ("d", "de", "dead", "deadbe"):
            fm.set_pattern(needle)
            fm.match_list(cp, subset=src, capture=dst)
            fm.match_list_top(cp, 100, subset=src, capture=dst)
            fm.match_list_top_indices(cp, 100, subset=src, capture=dst)
            fm.match_list_top_device(cp, 100, out.data_ptr(), 100, cnt.data_ptr(), subset=src, capture=dst)
            torch.cuda.synchronize()
            cp.set_scope(0, 1 if needle == "de" else 0)
            src, dst = dst, (a if dst is b else b)
        assert F.device_allocs() == before, "a subset query, fill or capture allocated device memory after the reserves"
