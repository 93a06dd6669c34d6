"""Multi-pattern top-`limit` with matched positions fused on the device (fzb_multi_match_list_top_indices_fused / _device /
fzb_multi_matcher_reserve_top_indices): the first min(limit, found) elements of what `Matcher::match_list_indices` returns over the whole list
for `Matcher::from_patterns` (src/matcher/mod.rs:234-275, `match_one_indices_multi` src/matcher/multi.rs:56-82), `index` = the corpus index,
and `found`.  Every expected value is the ORACLE's `MultiMatcher(...).match_list_indices_ordered(hs)` cut on the host, never this library's
own output; the facts about the inputs that make a case worth running (records beyond the pack's tile, mixed position counts, patterns
sharing characters, saturating sums) are asserted from the oracle's list before it is used."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from test_gpu_multi_requery import KEYS, hip_patterns
from test_gpu_parity import LANES
from test_gpu_top_indices import LT, MU, assert_top_indices, tuples, unpack
from test_gpu_topk import SORTS, limits_around
from test_oracle_multi import pats as oracle_pats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu

_corpus = {}


def ragged():
    """synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=1): (Corpus, haystacks), made once"""
    if "ragged" not in _corpus:
        data, ends = synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=1)
        _corpus["ragged"] = (F.Corpus(packed=(data, ends)), unpack(data, ends))
    return _corpus["ragged"]


_wanted = {}


def oracle_list(query, sort, **cfg):
    """the oracle's full ordered list for a parsed query over the ragged corpus, computed once per (query, sort, config)"""
    key = (query, sort, tuple(sorted(cfg.items())))
    if key not in _wanted:
        _wanted[key] = O.MultiMatcher(O.parse_query(query), sort=sort, **cfg).match_list_indices_ordered(ragged()[1])
    return _wanted[key]


def fused(query, sort, **cfg):
    return F.MultiMatcher(F.parse_query(query), F.Config(sort=F.SortStrategy[sort], pf_lanes=64, **cfg))


def composed(mm, cp, limit):
    """the untouched host composition fzb_multi_match_list_top_indices, called through lib() directly"""
    return F._top_indices(F.lib().fzb_multi_match_list_top_indices, mm.h, cp, limit)


@pytest.mark.parametrize("sort", SORTS)
def test_across_the_packs_tile(sort):
    cp, hs = ragged()
    want = oracle_list("de ad", sort)
    assert len(want) == 2803 and len(want) > 2049
    if sort == "ScoreThenIndexAsc":
        lens = [len(w[3]) for w in want[:2049]]
        assert set(lens) == {1, 2, 3, 4} and sum(x < 4 for x in lens) == 626  # shorter than the 4 needle bytes: the patterns share characters
    assert len({len(w[3]) for w in want[:2049]}) >= 3
    mm = fused("de ad", sort)
    for limit in (0, 1, 2, 100, 2048, 2049, 2803, 4000):
        got = mm.match_list_top_indices(cp, limit)
        assert_top_indices(got, want, limit, ("de ad", sort))
        if limit in (100, 2049):
            assert tuples(composed(mm, cp, limit)[0]) == tuples(got[0])


def test_typos():
    cp, hs = ragged()
    q = "deadbeef dea"
    want = oracle_list(q, "ScoreThenIndexAsc", max_typos=1)
    assert len(want) == 2151
    assert {len(w[3]) for w in want[:2049]} == set(range(2, 12)) and {len(w[3]) for w in want[:100]} == {7, 8, 9}
    mm = fused(q, "ScoreThenIndexAsc", max_typos=1)
    for limit in (100, 2049):
        got = mm.match_list_top_indices(cp, limit)
        assert_top_indices(got, want, limit, q)
        assert tuples(composed(mm, cp, limit)[0]) == tuples(got[0])


def test_fuzzy_literal_and_negated_mixed():
    cp, hs = ragged()
    q = "dead 'ea ^d !zz"
    for sort in ("ScoreThenIndexDesc", "IndexAsc"):
        want = oracle_list(q, sort)
        assert len(want) == 254 and {len(w[3]) for w in want} == set(range(3, 8))
        mm = fused(q, sort)
        for limit in limits_around(len(want)):
            got = mm.match_list_top_indices(cp, limit)
            assert_top_indices(got, want, limit, (q, sort))
            assert tuples(composed(mm, cp, limit)[0]) == tuples(got[0])


@pytest.mark.parametrize("sort", SORTS)
def test_known_answers_at_every_limit(sort):
    cases = [(hip_patterns(oracle_pats(c)), oracle_pats(c), c["haystacks"], c["config"], c["name"]) for c in MU["cases"]]
    cases += [(F.parse_query(q), O.parse_query(q), hs, cfg, q) for q, hs, cfg, _, _ in LT["multi_queries"]]
    for fpats, opats, hs, cfg, name in cases:
        cfg = dict(cfg)
        cfg["sort"] = sort
        want = O.MultiMatcher(opats, lanes=LANES[64], **cfg).match_list_indices_ordered(hs)
        fc = F.Config(max_typos=cfg.get("max_typos", 0), casing=F.CaseMatching[cfg.get("casing", "Smart")], sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=0)
        mm = F.MultiMatcher(fpats, fc)
        cp = F.Corpus(hs)
        for limit in limits_around(len(want)):
            assert_top_indices(mm.match_list_top_indices(cp, limit), want, limit, name)


def test_only_negated_patterns():
    hs = ["foo", "bar", "baz"]
    for sort in SORTS:
        want = O.MultiMatcher(O.parse_query("!foo"), sort=sort).match_list_indices_ordered(hs)
        assert sorted(w[0] for w in want) == [1, 2] and all(w[1] == 0 and w[3] == [] for w in want)
        mm = F.MultiMatcher(F.parse_query("!foo"), F.Config(sort=F.SortStrategy[sort], pf_lanes=64))
        for limit in (0, 1, 2, 3, 10):
            assert_top_indices(mm.match_list_top_indices(hs, limit), want, limit, ("!foo", sort))


def test_shared_characters_are_reported_once():
    hs = ["foo", "xfoo", "fo_foo", "f"]
    want = O.MultiMatcher(O.parse_query("foo fo")).match_list_indices_ordered(hs)
    assert want == [(0, 112, True, [2, 1, 0]), (2, 98, False, [4, 1, 0]), (1, 80, False, [3, 2, 1])]
    mm = F.MultiMatcher(F.parse_query("foo fo"), F.Config(pf_lanes=64))
    for limit in (1, 2, 3, 4):
        assert_top_indices(mm.match_list_top_indices(hs, limit), want, limit, "foo fo")


def test_sums_saturate_as_the_heads_do():
    """four patterns of 20000 and more each: the multi stage's sum and the union kernel's sum both stop at 65535 (else the pack's check fires)"""
    scoring = [20000, 6, 5, 1, 12, 4, 4, 8, 4]
    hs = ["abcd", "xaxbxcxd", "abc", "dcba"]
    opats = [O.P(x) for x in "abcd"]
    want = O.MultiMatcher(opats, scoring=scoring).match_list_indices_ordered(hs)
    assert len(want) == 3 and all(w[1] == 65535 for w in want)
    mm = F.MultiMatcher([F.Pattern(x) for x in "abcd"], F.Config(scoring=F.Scoring(*scoring), pf_lanes=64))
    for limit in (1, 3, 5):
        assert_top_indices(mm.match_list_top_indices(hs, limit), want, limit, "abcd, match_score 20000")


def test_more_patterns_than_the_argument_block_holds():
    """beyond the sources a launch carries by value, the union kernel reads them (and keeps its cursors) in device memory"""
    cp, hs = ragged()
    q = "d e a d b e e f de ad"
    want = oracle_list(q, "ScoreThenIndexAsc")
    assert len(F.parse_query(q)) == 10 and len(want) > 1500
    assert min(len(w[3]) for w in want[:2049]) < 12  # patterns share characters here too
    mm = fused(q, "ScoreThenIndexAsc")
    for limit in (100, 1500, 2049):
        assert_top_indices(mm.match_list_top_indices(cp, limit), want, limit, q)
    mm.set_patterns(F.parse_query("de ad"))  # and back under the bound on the same matcher
    assert_top_indices(mm.match_list_top_indices(cp, 100), oracle_list("de ad", "ScoreThenIndexAsc"), 100, "de ad")


def test_device_form_into_torch_tensors_on_a_side_stream():
    import torch

    cp, hs = ragged()
    q = "deadbeef dea"
    U = 11  # needle bytes of the two non-negated patterns together
    stream = torch.cuda.Stream()
    for sort in SORTS:
        want = oracle_list(q, sort, max_typos=1)
        mm = fused(q, sort, max_typos=1)
        for limit in (0, 1, 100, 2049, len(want), 10 * len(want)):
            cap = min(limit, len(cp))
            out = torch.zeros((max(cap, 1), 4), dtype=torch.int32, device="cuda")
            pos = torch.full((max(cap * U, 1),), -1, dtype=torch.int32, device="cuda")
            cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            mm.match_list_top_indices_device(cp, limit, out.data_ptr(), cap, pos.data_ptr(), cap * U, cnt.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()  # the call itself waits for nothing: the result is there once the stream has drained
            words = cnt.cpu().numpy().view(np.uint32).tolist()
            exp = want[:limit]
            total = sum(len(w[3]) for w in exp)
            assert words == [min(limit, len(want)), len(want), total, 0], (sort, limit, words)
            recs = out.cpu().numpy().reshape(-1).view(F.MATCH_INDICES_DTYPE)[: words[0]]
            flat = pos.cpu().numpy().view(np.uint32)
            begins = np.cumsum([0] + [len(w[3]) for w in exp])[:-1].tolist()
            assert recs["positions_begin"].tolist() == begins  # dense
            assert (flat[total:] == 0xFFFFFFFF).all()          # nothing is written behind the total
            got = [(int(r["index"]), int(r["score"]), bool(r["exact"]), flat[int(r["positions_begin"]) : int(r["positions_begin"]) + int(r["positions_len"])].tolist()) for r in recs]
            assert got == exp, (sort, limit)
        # room for fewer than min(limit, n) records, or for fewer than min(limit, n) x U positions: refused on the host, nothing launched
        for cap, pcap in ((10, 11 * U), (11, 11 * U - 1)):
            out = torch.zeros((11, 4), dtype=torch.int32, device="cuda")
            pos = torch.zeros((11 * U,), dtype=torch.int32, device="cuda")
            cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
            with pytest.raises(F.FrizbeeError) as e:
                mm.match_list_top_indices_device(cp, 11, out.data_ptr(), cap, pos.data_ptr(), pcap, cnt.data_ptr())
            assert e.value.code == 5  # FZB_ERR_CAPACITY
            torch.cuda.synchronize()
            assert cnt.cpu().tolist() == [-1, -1, -1, -1]
    with pytest.raises(F.FrizbeeError) as e:  # CompiledPatterns::Empty is the host form's
        F.MultiMatcher([]).match_list_top_indices_device(cp, 1, out.data_ptr(), 11, pos.data_ptr(), 11 * U, cnt.data_ptr())
    assert e.value.code == 1
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [-1, -1, -1, -1]
    # an empty corpus zeroes the four words
    F.MultiMatcher(F.parse_query("abc !d")).match_list_top_indices_device(F.Corpus([]), 5, out.data_ptr(), 11, pos.data_ptr(), 11 * U, cnt.data_ptr())
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [0, 0, 0, 0]


def test_no_device_allocation_after_reserve():
    data, ends = synth.paths_corpus()
    ends = ends[:200_000]
    data = data[: int(ends[-1])]
    cp = F.Corpus(packed=(data, ends))
    mm = F.MultiMatcher(F.parse_query(KEYS[-1]), F.Config(pf_lanes=64))  # three patterns: the slots the sequence needs
    mm.reserve(cp)
    mm.reserve_top_indices(cp, 1000, 8)
    before = F.device_allocs()
    last = {}
    for key in KEYS:
        mm.set_patterns(F.parse_query(key))
        for limit in (1, 100, 1000):
            recs, found = mm.match_list_top_indices(cp, limit)
            assert len(recs) == min(limit, found)
            last[key] = (recs, found)
    mm.set_config(F.Config(pf_lanes=64, sort=F.SortStrategy.ScoreThenIndexDesc))
    mm.set_patterns(F.parse_query("src linux"))
    got = mm.match_list_top_indices(cp, 100)
    assert F.device_allocs() == before
    # and what the replay answered is right
    hs = unpack(data, ends)
    for key in ("src linux !test", "src l"):
        want = O.MultiMatcher(O.parse_query(key)).match_list_indices_ordered(hs)
        assert len(want) > 1000
        assert_top_indices(last[key], want, 1000, key)
    want = O.MultiMatcher(O.parse_query("src linux"), sort="ScoreThenIndexDesc").match_list_indices_ordered(hs)
    assert_top_indices(got, want, 100, "src linux, Desc")


def test_interleaving_on_one_matcher():
    """the fused query shares the composition's buffers, the sort's and every sub-matcher's trace scratch with the other entry points"""
    data, ends = synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=5)
    cp = F.Corpus(packed=(data, ends))
    hs = unpack(data, ends)
    odata = np.concatenate([data, np.zeros(64, np.uint8)])
    sort = "ScoreThenIndexDesc"
    mm = F.MultiMatcher(F.parse_query("dead be"), F.Config(sort=F.SortStrategy[sort], pf_lanes=64))

    def rounds(m, q, n):
        om = O.MultiMatcher(O.parse_query(q), sort=sort)
        full = om.match_packed(odata, ends)
        full_ix = om.match_list_indices_ordered(hs)
        assert len(full_ix) > 300
        for _ in range(n):
            recs, found = m.match_list_top(cp, 50)
            assert recs.tolist() == full[:50].tolist() and found == len(full)
            assert_top_indices(m.match_list_top_indices(cp, 300), full_ix, 300, q)
            assert m.match_list(cp).tolist() == full.tolist()
            sel = full["index"][:40]
            sub = O.MultiMatcher(O.parse_query(q), sort=sort).match_list_indices_ordered([hs[i] for i in sel])
            assert tuples(m.match_list_indices(cp, selection=sel)) == sub
            assert_top_indices(m.match_list_top_indices(cp, 3000), full_ix, 3000, q)

    rounds(mm, "dead be", 2)
    mm.set_patterns(F.parse_query("dead"))          # fewer patterns (CompiledPatterns::Single)
    rounds(mm, "dead", 1)
    mm.set_patterns(F.parse_query("de ad be !x"))   # and more than before
    rounds(mm, "de ad be !x", 1)
    other = mm.clone()
    rounds(other, "de ad be !x", 1)
    rounds(mm, "de ad be !x", 1)
