"""Top-`limit` queries (fzb_match_list_top / _top_device / fzb_multi_match_list_top): the first min(limit, found) records of `match_list`'s
result, selected and ordered on the device, and `found`.  The reference has no such call - its caller truncates the Vec `match_list`
returns (src/matcher/mod.rs:212-222) - so every expected value here is the ORACLE's full list cut on the host, never this library's own
`match_list`."""
import json
import os
import sys

import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from test_gpu_multi_requery import KEYS, hip_patterns
from test_gpu_parity import LANES, _expand
from test_oracle_multi import pats as oracle_pats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
MT = json.load(open(os.path.join(G, "matcher.json")))
MU = json.load(open(os.path.join(G, "multi.json")))
LT = json.load(open(os.path.join(G, "literal.json")))
SORTS = ("ScoreThenIndexAsc", "ScoreThenIndexDesc", "IndexAsc", "IndexDesc")


def limits_around(found):
    return sorted({x for x in (0, 1, 2, found - 1, found, found + 1, 10 * found) if x >= 0})


def assert_top(got, want, limit, ctx=""):
    recs, found = got
    assert found == len(want), (ctx, limit, found, len(want))
    if recs.tolist() != want[:limit].tolist():
        exp = want[:limit]
        n = min(len(recs), len(exp))
        bad = [i for i in range(n) if recs[i].tolist() != exp[i].tolist()][:5]
        raise AssertionError(f"{ctx} limit {limit}: len {len(recs)} vs {len(exp)}; first diffs {[(i, recs[i].tolist(), exp[i].tolist()) for i in bad]}")


def single(needle, sort="ScoreThenIndexAsc", pf=64, **kw):
    """(HIP matcher, oracle matcher) with the same configuration"""
    scoring = kw.pop("scoring", None) or O.DEFAULT_SCORING
    om = O.Matcher(needle, lanes=LANES[pf], scoring=scoring, sort=sort, **kw)
    oi = om.info()
    fc = F.Config(max_typos=kw.get("max_typos", 0), casing=F.CaseMatching[kw.get("casing", "Smart")], unicode=F.UnicodeMatching[kw.get("unicode", "Smart")],
                  matching=F.Matching[kw.get("matching", "Fuzzy")], sort=F.SortStrategy[sort], scoring=F.Scoring(*scoring), pf_lanes=oi["pf_lanes"], sw_lanes=oi["sw_lanes"])
    return F.Matcher(needle, fc), om


def opad(data):
    return np.concatenate([data, np.zeros(64, np.uint8)])


@pytest.mark.parametrize("sort", SORTS)
def test_reference_known_answers_cut_at_every_limit(sort):
    for case in MT["cases"]:
        hs = _expand(case["haystacks"])
        cfg = dict(case["config"])
        cfg["sort"] = sort
        fm, om = single(case["needle"], **cfg)
        want = om.match_list(hs)
        cp = F.Corpus(hs)
        for limit in limits_around(len(want)):
            assert_top(fm.match_list_top(cp, limit), want, limit, case["name"])


@pytest.mark.parametrize("sort", SORTS)
def test_multi_pattern_known_answers_cut_at_every_limit(sort):
    cases = [(hip_patterns(oracle_pats(c)), oracle_pats(c), c["haystacks"], c["config"], c["name"]) for c in MU["cases"]]
    cases += [(F.parse_query(q), O.parse_query(q), hs, cfg, q) for q, hs, cfg, _, _ in LT["multi_queries"]]
    for fpats, opats, hs, cfg, name in cases:
        cfg = dict(cfg)
        cfg["sort"] = sort
        want = O.MultiMatcher(opats, lanes=LANES[64], **cfg).match_list(hs)
        fc = F.Config(max_typos=cfg.get("max_typos", 0), casing=F.CaseMatching[cfg.get("casing", "Smart")], sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=0)
        mm = F.MultiMatcher(fpats, fc)
        cp = F.Corpus(hs)
        for limit in limits_around(len(want)):
            assert_top(mm.match_list_top(cp, limit), want, limit, name)


def test_random_parity_with_cuts_through_tie_groups():
    """336 (query, limit) pairs.  The condition that makes the test mean something is asserted: at least half of the pairs have
    found > limit and at least a quarter cut through a group of equal scores (the oracle's records limit-1 and limit tie)."""
    pairs = beyond = through_tie = 0
    for seed in range(6):
        data, ends = synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=seed)
        cp = F.Corpus(packed=(data, ends))
        odata = opad(data)
        for needle, typos in (("deadbeef", 0), ("dead", 0), ("deadbeef", 1), ("db", None)):
            for sort in ("ScoreThenIndexAsc", "ScoreThenIndexDesc"):
                fm, om = single(needle, sort=sort, max_typos=typos)
                want = om.match_packed(odata, ends)
                for limit in (0, 1, 2, 10, 100, 1000, 4096):
                    assert_top(fm.match_list_top(cp, limit), want, limit, (seed, needle, typos, sort))
                    pairs += 1
                    beyond += len(want) > limit
                    through_tie += 0 < limit < len(want) and want[limit - 1]["score"] == want[limit]["score"]
    print(f"pairs {pairs}, found > limit {beyond}, cut through a tie group {through_tie}")
    assert pairs == 336
    assert 2 * beyond >= pairs and 4 * through_tie >= pairs, (pairs, beyond, through_tie)


def test_both_selection_levels():
    """scores on both sides of 256: a cut above 255 (the high byte's level decides) and one below (the low byte's level inside bucket 0)"""
    needle = "deadbeefdeadbeefdead"
    data, ends = synth.ragged_corpus(needle.encode(), 30_000, 4, 96, seed=1)
    cp = F.Corpus(packed=(data, ends))
    for sort in ("ScoreThenIndexAsc", "ScoreThenIndexDesc"):
        fm, om = single(needle, sort=sort, max_typos=2)
        want = om.match_packed(opad(data), ends)
        assert int((want["score"] >= 256).sum()) > 100 and len(want) > 1000
        assert want[99]["score"] >= 256 > want[999]["score"]
        for limit in (100, 1000):
            assert_top(fm.match_list_top(cp, limit), want, limit, (needle, sort))
    data, ends = synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=1)
    cp = F.Corpus(packed=(data, ends))
    q = "deadbeef dead beef"
    for sort in ("ScoreThenIndexAsc", "ScoreThenIndexDesc"):
        want = O.MultiMatcher(O.parse_query(q), sort=sort).match_packed(opad(data), ends)
        assert want[19]["score"] >= 256 > want[499]["score"]
        mm = F.MultiMatcher(F.parse_query(q), F.Config(sort=F.SortStrategy[sort], pf_lanes=64))
        for limit in (20, 500):
            assert_top(mm.match_list_top(cp, limit), want, limit, (q, sort))


def test_unicode_literal_index_orders_empty_pattern_and_no_match():
    data, ends = synth.utf8_corpus(50_000, 32)
    cp = F.Corpus(packed=(data, ends))
    for sort in SORTS:
        fm, om = single("إنما", sort=sort)
        want = om.match_packed(opad(data), ends)
        assert len(want) > 200
        for limit in (0, 1, 100, len(want) - 1, len(want), len(want) + 1):
            assert_top(fm.match_list_top(cp, limit), want, limit, ("utf8", sort))
    data, ends = synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=2)
    cp = F.Corpus(packed=(data, ends))
    odata = opad(data)
    for sort in SORTS:
        for needle, kw in (("dead", {"matching": "Substring"}), ("de", {"matching": "Prefix"}), ("deadbeef", {}), ("deadbeef", {"max_typos": 1})):
            fm, om = single(needle, sort=sort, **kw)
            want = om.match_packed(odata, ends)
            for limit in (0, 1, 7, 100, 2049, len(want), len(want) + 5):
                assert_top(fm.match_list_top(cp, limit), want, limit, (needle, kw, sort))
        # CompiledPatterns::Empty: every haystack, score 0, the first `limit` indices or the last `limit` reversed
        want = O.Matcher("", sort=sort).match_packed(odata, ends)
        assert len(want) == 30_000
        for limit in (0, 1, 100, 30_000, 40_000):
            assert_top(F.Matcher("", F.Config(sort=F.SortStrategy[sort])).match_list_top(cp, limit), want, limit, ("empty needle", sort))
            assert_top(F.MultiMatcher([], F.Config(sort=F.SortStrategy[sort])).match_list_top(cp, limit), want, limit, ("no pattern", sort))
        # nothing matches at all
        for limit in (0, 1, 100):
            recs, found = F.Matcher("@@##", F.Config(sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=64)).match_list_top(cp, limit)
            assert found == 0 and len(recs) == 0
            recs, found = F.MultiMatcher(F.parse_query("@@## dead"), F.Config(sort=F.SortStrategy[sort], pf_lanes=64)).match_list_top(cp, limit)
            assert found == 0 and len(recs) == 0
    recs, found = F.Matcher("abc").match_list_top([], 5)
    assert found == 0 and len(recs) == 0


def test_device_form_into_torch_tensors():
    import torch

    data, ends = synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=4)
    cp = F.Corpus(packed=(data, ends))
    for sort in SORTS:
        fm, om = single("dead", sort=sort)
        want = om.match_packed(opad(data), ends)
        for limit in (0, 1, 100, 5000, len(want), 10 * len(want)):
            cap = min(limit, len(cp))
            out = torch.zeros((max(cap, 1), 2), dtype=torch.int32, device="cuda")
            cnt = torch.full((2,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            fm.match_list_top_device(cp, limit, out.data_ptr(), cap, cnt.data_ptr())
            torch.cuda.synchronize()
            words = cnt.cpu().numpy().view(np.uint32).tolist()
            assert words == [min(limit, len(want)), len(want)], (sort, limit, words)
            recs = out.cpu().numpy().reshape(-1).view(F.MATCH_DTYPE)[: words[0]]
            assert recs.tolist() == want[:limit].tolist(), (sort, limit)
        if len(want) > 10:  # room for fewer than min(limit, n) records: refused on the host, nothing launched
            out = torch.zeros((10, 2), dtype=torch.int32, device="cuda")
            cnt = torch.full((2,), -1, dtype=torch.int32, device="cuda")
            with pytest.raises(F.FrizbeeError) as e:
                fm.match_list_top_device(cp, 11, out.data_ptr(), 10, cnt.data_ptr())
            assert e.value.code == 5  # FZB_ERR_CAPACITY
            torch.cuda.synchronize()
            assert cnt.cpu().tolist() == [-1, -1]


def test_no_device_allocation_after_reserve():
    data, ends = synth.paths_corpus()
    ends = ends[:200_000]
    data = data[: int(ends[-1])]
    cp = F.Corpus(packed=(data, ends))
    # (fzb_matcher_reserve sizes the multi-chunk scorer's parked rows for the needle it is called with: the longest of the replay)
    fm = F.Matcher("srclinuxtest", F.Config(pf_lanes=64, sw_lanes=64))
    mm = F.MultiMatcher([], F.Config(pf_lanes=64))
    for key in KEYS:  # first pass, as in test_gpu_multi_requery: the multi matcher's slots grow to the query's three patterns
        mm.set_patterns(F.parse_query(key))
        mm.match_list_top(cp, 10)
    fm.reserve(cp)
    mm.reserve(cp)
    before = F.device_allocs()
    for key in KEYS:
        for limit in (1, 100, 100_000):
            fm.set_pattern(key.replace(" ", "").replace("!", ""))
            recs, found = fm.match_list_top(cp, limit)
            assert len(recs) == min(limit, found)
            mm.set_patterns(F.parse_query(key))
            recs, found = mm.match_list_top(cp, limit)
            assert len(recs) == min(limit, found)
    assert F.device_allocs() == before
    # and what the replay answered is right
    odata = opad(data)
    want = O.MultiMatcher(O.parse_query(KEYS[-1])).match_packed(odata, ends)
    assert_top(mm.match_list_top(cp, 100), want, 100, KEYS[-1])
    want = O.Matcher("srclinuxtest").match_packed(odata, ends)
    assert_top(fm.match_list_top(cp, 100), want, 100, "srclinuxtest")


def test_interleaving_with_every_other_call_on_one_matcher():
    data, ends = synth.ragged_corpus(b"deadbeef", 100_000, 4, 96, seed=5)  # (enough matches of "dead" for top(5000) to cut the list)
    cp = F.Corpus(packed=(data, ends))
    odata = opad(data)
    for sort in ("ScoreThenIndexAsc", "ScoreThenIndexDesc", "IndexDesc"):
        fm, om = single("dead", sort=sort)
        want = om.match_packed(odata, ends)
        into = O.Matcher("dead", sort="IndexAsc").match_packed(odata, ends)
        assert len(want) > 5000
        for rnd in range(2):
            assert_top(fm.match_list_top(cp, 10), want, 10, (sort, rnd))
            assert fm.match_list(cp).tolist() == want.tolist()
            top = fm.match_list_top(cp, 5000)
            assert_top(top, want, 5000, (sort, rnd))
            assert fm.match_list_into(cp).tolist() == into.tolist()
            sel = top[0]["index"][:50].astype(np.uint32)
            hs = [bytes(data[(int(ends[i - 1]) if i else 0) : int(ends[i])]) for i in sel.tolist()]
            got = [(m.index, m.score, m.exact, m.indices) for m in fm.match_list_indices(cp, selection=sel)]
            assert got == om.match_list_indices_ordered(hs)
            assert_top(fm.match_list_top(cp, 10), want, 10, (sort, rnd))
        fm.set_pattern("beef")
        want = O.Matcher("beef", sort=sort).match_packed(odata, ends)
        assert_top(fm.match_list_top(cp, 300), want, 300, ("after set_pattern", sort))
        fm.set_config(F.Config(max_typos=1, sort=F.SortStrategy.ScoreThenIndexDesc, pf_lanes=64, sw_lanes=64))
        want = O.Matcher("beef", max_typos=1, sort="ScoreThenIndexDesc").match_packed(odata, ends)
        assert_top(fm.match_list_top(cp, 300), want, 300, ("after set_config", sort))
        assert fm.match_list(cp).tolist() == want.tolist()
    mm = F.MultiMatcher(F.parse_query("dead be !x"), F.Config(pf_lanes=64))
    want = O.MultiMatcher(O.parse_query("dead be !x")).match_packed(odata, ends)
    for rnd in range(2):
        assert_top(mm.match_list_top(cp, 10), want, 10, ("multi", rnd))
        assert mm.match_list(cp).tolist() == want.tolist()
        assert_top(mm.match_list_top(cp, 5000), want, 5000, ("multi", rnd))


def test_c2_full_size():
    """the headline list: 10 M haystacks of 32 bytes, ~ 0.5 M matches"""
    rows, ends = synth.fixed_corpus(b"deadbe", 10_000_000, 32, device="cuda")
    data = rows.cpu().numpy().reshape(-1)
    fm, om = single("deadbe")
    want = om.match_packed(opad(data), ends, threads=os.cpu_count() or 1)
    assert len(want) > 100_000
    cp = F.Corpus(packed=(data, ends))
    for limit in (100, 100_000):
        assert_top(fm.match_list_top(cp, limit), want, limit, "C2")
    fm.set_config(F.Config(sort=F.SortStrategy.ScoreThenIndexDesc, pf_lanes=64, sw_lanes=64))
    recs, found = fm.match_list_top(cp, 100_000)
    s, i = recs["score"].astype(np.int64), recs["index"].astype(np.int64)
    assert found == len(want) and len(recs) == 100_000 and np.array_equal(s, want["score"][:100_000])
    assert np.all((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (i[:-1] > i[1:])))
