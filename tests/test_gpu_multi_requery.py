"""The multi-pattern matcher's lifecycle on the device (fzb_multi_matcher_set_patterns / _set_config / _reserve / _clone): a re-queried
matcher answers exactly as a fresh `from_patterns` matcher would (src/matcher/mod.rs:154-190), an identical re-query is a no-op, and after
`reserve` the keystroke replay of an interactive picker allocates no device memory."""
import json
import os
import sys

import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from ref_generators import multi_cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import synth  # noqa: E402
from test_oracle_multi import pats as oracle_pats  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MU = json.load(open(os.path.join(GOLDEN, "multi.json")))
LT = json.load(open(os.path.join(GOLDEN, "literal.json")))
SORTS = ("ScoreThenIndexAsc", "ScoreThenIndexDesc", "IndexAsc", "IndexDesc")
KEYS = ["s", "sr", "src", "src l", "src li", "src lin", "src linux", "src linux !", "src linux !t", "src linux !test"]


def hip_patterns(opats):
    return [F.Pattern(p["needle"], negated=p["negated"], max_typos=None if p["max_typos"] == O.INHERIT else p["max_typos"],
                      casing=None if p["casing"] is None else F.CaseMatching[p["casing"]],
                      matching=None if p.get("matching") is None else F.Matching[p["matching"]]) for p in opats]


def cfg_of(sort="ScoreThenIndexAsc", max_typos=0, casing="Smart", matching="Fuzzy"):
    return F.Config(max_typos=max_typos, casing=F.CaseMatching[casing], matching=F.Matching[matching], sort=F.SortStrategy[sort], pf_lanes=64)


def test_set_patterns_equals_a_fresh_matcher_on_the_known_answers():
    """golden multi.json cases and literal.json's parsed queries, one re-queried matcher per sort strategy"""
    cases = [(hip_patterns(oracle_pats(c)), c["haystacks"], c["config"]) for c in MU["cases"]]
    cases += [(F.parse_query(q), hs, cfg) for q, hs, cfg, _, _ in LT["multi_queries"]]
    for sort in SORTS:
        rq = F.MultiMatcher(F.parse_query("seed pattern !x"), cfg_of(sort))
        for pats, hs, cfg in cases:
            c = cfg_of(sort, max_typos=cfg.get("max_typos", 0), casing=cfg.get("casing", "Smart"))
            cp = F.Corpus(hs)
            rq.set_config(c)
            rq.set_patterns(pats)
            assert rq.match_list(cp).tolist() == F.MultiMatcher(pats, c).match_list(cp).tolist(), (pats, cfg, sort)


def test_set_patterns_equals_a_fresh_matcher_on_generated_cases():
    rq = {s: F.MultiMatcher([], cfg_of(s)) for s in SORTS}
    for it, (patterns, haystacks, cfg) in enumerate(multi_cases(200, 4242)):
        fpats = [F.Pattern(p["needle"], negated=p["negated"], matching=None if p["matching"] is None else F.Matching[p["matching"]]) for p in patterns]
        opats = [O.P(p["needle"], negated=p["negated"], matching=p["matching"]) for p in patterns]
        cp = F.Corpus(haystacks)
        for sort in SORTS:
            c = cfg_of(sort, **cfg)
            rq[sort].set_config(c)
            rq[sort].set_patterns(fpats)
            got = rq[sort].match_list(cp)
            assert got.tolist() == F.MultiMatcher(fpats, c).match_list(cp).tolist(), (it, patterns, cfg, sort)
            assert got.tolist() == O.MultiMatcher(opats, lanes=(64, 64, 32), sort=sort, **cfg).match_list(haystacks).tolist(), (it, patterns, cfg, sort)


def test_transitions_between_empty_single_and_multi():
    """Empty -> Single -> Multi -> lone negated (Multi) -> Empty, the pattern count growing and shrinking (src/matcher/mod.rs:178-190)"""
    rows, ends = synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=11)
    cp = F.Corpus(packed=(rows, ends))
    odata = np.concatenate([rows, np.zeros(64, np.uint8)])
    steps = ["", "dead", "dead be !x", "de ad be ef !q", "!x", "dead", "", "a b c d e", "!deadbeef", ""]
    for sort in SORTS:
        rq = F.MultiMatcher([], cfg_of(sort))
        for q in steps:
            rq.set_patterns(F.parse_query(q))
            got = rq.match_list(cp)
            assert len(rq) == len(F.parse_query(q))
            assert got.tolist() == F.MultiMatcher(F.parse_query(q), cfg_of(sort)).match_list(cp).tolist(), (q, sort)
            assert got.tolist() == O.MultiMatcher(O.parse_query(q), sort=sort).match_packed(odata, ends).tolist(), (q, sort)


def test_set_config_equals_a_fresh_matcher_including_a_sort_only_change():
    """every config change answers as a fresh matcher; a reserved matcher allocates nothing for any of them (its slots hold the buffers of
    every form), and a change of `sort` alone rebuilds no sub-matcher"""
    rows, ends = synth.ragged_corpus(b"deadbeef", 20_000, 4, 96, seed=3)
    cp = F.Corpus(packed=(rows, ends))
    pats = F.parse_query("dead bf !x")
    rq = F.MultiMatcher(pats, cfg_of())
    rq.reserve(cp)
    rq.match_list(cp)
    for c in (cfg_of("IndexDesc"), cfg_of("ScoreThenIndexDesc"), cfg_of(max_typos=1), cfg_of(max_typos=None, casing="Respect"), cfg_of("IndexAsc", max_typos=2),
              cfg_of("IndexDesc", matching="Substring"), cfg_of("ScoreThenIndexAsc", matching="Substring")):
        before = F.device_allocs()
        rq.set_config(c)
        got = rq.match_list(cp)
        grew = F.device_allocs() - before  # (before the fresh matcher below allocates its own buffers)
        assert got.tolist() == F.MultiMatcher(pats, c).match_list(cp).tolist(), c
        assert grew == 0, c
    c = cfg_of("IndexDesc", max_typos=2)
    rq.set_config(c)
    before = F.device_allocs()
    rq.set_config(c)  # equal config: no-op
    assert F.device_allocs() == before


def test_reserve_on_a_short_query_covers_longer_fuzzy_and_unicode_needles():
    """reserve sizes every slot for ANY needle of up to 64 bytes in any form: reserved on a one-letter query with a literal (negated) pattern,
    re-queries with longer needles, a literal slot turned fuzzy, a wider score class and a unicode needle allocate nothing"""
    data, ends = synth.paths_corpus()
    ends = ends[:200_000]
    data = data[: int(ends[-1])]
    cp = F.Corpus(packed=(data, ends))
    odata = np.concatenate([data, np.zeros(64, np.uint8)])
    m = F.MultiMatcher(F.parse_query("s !t"), F.Config(pf_lanes=64))
    m.reserve(cp)
    before = F.device_allocs()
    queries = ["s !t", "src l", "src linux", "src t", "src linux", "linuxsrclinuxsrcab t", "src linuxlinuxlinuxlinuxlinuxlinuxlinuxlinuxlinux12",
               "münchen src", "ü !ü", "src !linux", "s"]
    results = []
    for q in queries:
        m.set_patterns(q)
        results.append(m.match_list(cp))
    assert F.device_allocs() - before == 0
    for q, got in zip(queries, results):
        want = O.MultiMatcher(O.parse_query(q)).match_packed(odata, ends)
        assert np.array_equal(got, want), (q, len(got), len(want))


def test_identical_set_patterns_is_a_no_op():
    rows, ends = synth.ragged_corpus(b"deadbeef", 20_000, 4, 96, seed=5)
    cp = F.Corpus(packed=(rows, ends))
    pats = F.parse_query("dead ^de !x")
    m = F.MultiMatcher(pats, cfg_of())
    want = m.match_list(cp)
    before = F.device_allocs()
    m.set_patterns(F.parse_query("dead ^de !x"))
    got = m.match_list(cp)
    assert F.device_allocs() - before == 0 and got.tolist() == want.tolist()


def test_keystroke_replay_after_reserve_allocates_nothing_on_the_paths_list():
    data, ends = synth.paths_corpus()
    cp = F.Corpus(packed=(data, ends))
    odata = np.concatenate([data, np.zeros(64, np.uint8)])
    m = F.MultiMatcher([], F.Config(pf_lanes=64))
    for q in KEYS:  # first pass: the slots grow to the query's three patterns
        m.set_patterns(F.parse_query(q))
        m.match_list(cp)
    m.reserve(cp)
    before = F.device_allocs()
    results = []
    for q in KEYS:
        m.set_patterns(F.parse_query(q))
        results.append(m.match_list(cp))
    assert F.device_allocs() - before == 0
    for q, got in zip(KEYS, results):
        want = O.MultiMatcher(O.parse_query(q)).match_packed(odata, ends)
        assert len(got) == len(want) and np.array_equal(got, want), (q, len(got), len(want))


def test_clone_is_independent():
    rows, ends = synth.ragged_corpus(b"deadbeef", 20_000, 4, 96, seed=9)
    cp = F.Corpus(packed=(rows, ends))
    m = F.MultiMatcher(F.parse_query("dead be !x"), cfg_of("ScoreThenIndexDesc"))
    want = m.match_list(cp)
    c = m.clone()
    assert c.match_list(cp).tolist() == want.tolist()
    c.set_patterns(F.parse_query("ef !d"))
    assert c.match_list(cp).tolist() == F.MultiMatcher(F.parse_query("ef !d"), cfg_of("ScoreThenIndexDesc")).match_list(cp).tolist()
    assert m.match_list(cp).tolist() == want.tolist()
    del c
    assert m.match_list(cp).tolist() == want.tolist()
