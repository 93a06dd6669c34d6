"""Any-of groups (`a | b`) composed on the device: every records form of a grouped `MultiMatcher` against the model of tests/anyof_model.py -
the oracle per alternative over the full list, unioned per group under the max rule, composed in numpy (held to the reference's composition
by tests/test_oracle_anyof_premise.py) - compared on index, score and exact.  Terms around the composition (bias, scope, subset, capture,
facets, sections, top-`limit`) are applied to the model in numpy, as the tests of those features do."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import anyof_model as M
import frizbee_amd as F
import oracle_lib as O
from facets_model import facet_words
from test_gpu_facets import check as check_facets
from test_gpu_scope import visible
from test_gpu_score_bias import biased, same
from test_gpu_subset import device_top, mask_of
from test_gpu_topk import SORTS, assert_top

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = (1, 1023, 1024, 1025, 2049)  # the compaction's tile is 1024
TIE = [12, 6, 5, 1, 36, 4, 4, 8, 4]  # the needle without its last byte under this scoring ties the whole needle on the haystack that IS the needle
TOKENS = [b"dead", b"deadbe", b"beef", b"cafe", b"src/", b"test", b"x", b"_", b"Qz", b"daed", b"cfe", b"e"]
EXTS = [b".rs", b".py", b".go", b".md", b".c"]
_LISTS = {}


def tie_haystack(kind):
    return b"dead" if kind == "ragged" else b"dead" + b"ghij" * 7


def make_list(kind, n):
    """seeded haystacks of tokens with an extension at the end; uniform32: every one padded in the middle to 32 bytes.  The first holds the
    tie haystack, the next few one of every class by construction (the tests assert the classes on the model anyway)."""
    if (kind, n) not in _LISTS:
        if kind == "utf8":
            data, ends = synth.utf8_corpus(n, 32, seed=n)
            raw, hs, start = data.tobytes(), [], 0
            for e in ends.tolist():
                hs.append(raw[start:e])
                start = e
        else:
            rng = np.random.default_rng(n * 2 + (kind == "ragged"))
            hs = [tie_haystack(kind), b"zzz.md", b"dead.rs", b"deadbeefcafe.py", b"src/test_cafe.go"]
            while len(hs) < n:
                body = b"".join(TOKENS[int(t)] for t in rng.integers(0, len(TOKENS), int(rng.integers(1, 5))))
                hs.append(body[:24] + EXTS[int(rng.integers(0, len(EXTS)))])
            hs = hs[:n]
            if kind == "uniform32":
                hs = [h if len(h) == 32 else h[:-3][:29] + b"g" * (32 - len(h[:-3][:29]) - 3) + h[-3:] for h in hs]
                assert all(len(h) == 32 for h in hs)
        _LISTS[(kind, n)] = hs
    return _LISTS[(kind, n)]


def alternatives(name, kind):
    t = tie_haystack(kind).decode()
    return {
        "fuzzy0": [O.P("dead"), O.P("beef"), O.P("cafe")],
        "fuzzy1": [O.P("deadbe", max_typos=1), O.P("cafe", max_typos=1)],
        "suffix": [O.P("rs", matching="Suffix"), O.P("py", matching="Suffix"), O.P("go", matching="Suffix")],
        "tie": [O.P(t), O.P(t[:-1], scoring=TIE)],
        "unicode": [O.P("إن"), O.P("ما"), O.P("إنما")],
    }[name]


def positions(alts, kind):
    """name -> (patterns, group_of): where the group stands in the query"""
    k = len(alts)
    if kind == "utf8":
        base, other, neg = O.P("ن"), [O.P("إ"), O.P("م")], O.P("ا", negated=True, matching="Substring")
    else:
        base, other, neg = O.P("a"), [O.P("s"), O.P("t")], O.P("test", negated=True, matching="Substring")
    neg2 = dict(neg, needle="x" if kind != "utf8" else "،")
    return {
        "base": (alts, [0] * k),
        "later": ([base] + alts, [0] + [1] * k),
        "then_negated": (alts + [neg], [0] * k + [1]),
        "two_groups": (alts + other, [0] * k + [1, 1]),
        "others_negated": ([neg2] + alts + [neg], [0] + [1] * k + [2]),
    }


def hip_patterns(opats):
    return [F.Pattern(p["needle"], negated=p["negated"], max_typos=None if p["max_typos"] == O.INHERIT else p["max_typos"],
                      matching=None if p.get("matching") is None else F.Matching[p["matching"]], scoring=None if p["scoring"] is None else F.Scoring(*p["scoring"]))
            for p in opats]


def matcher(pats, groups, sort="ScoreThenIndexAsc", **kw):
    return F.MultiMatcher(hip_patterns(pats), F.Config(sort=F.SortStrategy[sort], pf_lanes=64, **kw), groups=groups)


def classes(alts, hs):
    """how many haystacks are matched by no, exactly one, several alternatives, and how many hold a tie at the maximum with different exact flags"""
    hits = [M.pattern_hits(p, hs, {}) for p in alts]
    per = [[h[i] for h in hits if i in h] for i in range(len(hs))]
    ties = sum(1 for v in per if v and len({e for s, e in v if s == max(x[0] for x in v)}) == 2)
    return dict(none=sum(not v for v in per), one=sum(len(v) == 1 for v in per), several=sum(len(v) > 1 for v in per), tie=ties)


def check_all_sorts(pats, groups, hs, cp, ctx):
    fm = matcher(pats, groups)
    for sort in SORTS:
        fm.set_config(F.Config(sort=F.SortStrategy[sort], pf_lanes=64))
        want = M.match_list(pats, groups, hs, sort=sort)
        same(fm.match_list(cp), want, (ctx, sort))
        recs, found = fm.match_list_top(cp, 10)
        assert found == len(want) and recs.tolist() == want[:10].tolist(), (ctx, sort, found, len(want))
    return len(want)


CASES = [(kind, n) for kind in ("uniform32", "ragged") for n in SIZES] + [("utf8", 1025)]


@pytest.mark.parametrize("kind,n", CASES)
def test_match_list_in_every_sort_order_equals_the_model(kind, n):
    hs = make_list(kind, n)
    cp = F.Corpus(hs)
    kinds = ("unicode",) if kind == "utf8" else ("fuzzy0", "fuzzy1", "suffix", "tie")
    sizes = {}
    for aname in kinds:
        alts = alternatives(aname, kind)
        if n >= 1023:  # the list says something about the union: every class of haystack is there
            c = classes(alts, hs)
            if aname == "tie":  # (on the uniform list only the planted haystack holds the 32-byte needle)
                assert c["none"] and c["several"] and c["tie"] >= 1, c
            else:
                assert c["none"] and c["one"] and (c["several"] or aname == "suffix"), (aname, c)  # (a haystack has one suffix)
        for pname, (pats, groups) in positions(alts, kind).items():
            sizes[(aname, pname)] = check_all_sorts(pats, groups, hs, cp, (kind, n, aname, pname))
    if n >= 1023:
        assert all(0 < v < n for k, v in sizes.items() if k[1] in ("base", "later")), sizes
        assert all(sizes[(a, "later")] < sizes[(a, "base")] for a in kinds if a != "tie"), sizes  # (the base pattern narrows what the group sees)
        assert sum(v > 0 for v in sizes.values()) > len(sizes) // 2, sizes


def test_the_tie_takes_the_exact_flag_of_the_alternative_that_has_it():
    for kind in ("ragged", "uniform32"):
        hs = make_list(kind, 1025)
        alts = alternatives("tie", kind)
        for order in (alts, alts[::-1]):
            got = matcher(order, [0, 0], sort="IndexAsc").match_list(F.Corpus(hs))
            want = M.match_list(order, [0, 0], hs, sort="IndexAsc")
            same(got, want, kind)
            solo = [M.pattern_hits(p, hs, {})[0] for p in alts]
            assert solo[0][0] == solo[1][0] and {solo[0][1], solo[1][1]} == {0, 1}, solo  # haystack 0: equal scores, different flags
            assert int(got[0]["index"]) == 0 and int(got[0]["exact"]) == 1 and int(got[0]["score"]) == solo[0][0]


def test_an_empty_corpus_and_a_query_no_alternative_matches():
    alts = alternatives("fuzzy0", "ragged")
    fm = matcher(alts, [0, 0, 0])
    assert len(fm.match_list(F.Corpus([]))) == 0
    assert fm.match_list_top(F.Corpus([]), 5)[1] == 0
    hs = make_list("ragged", 1025)
    cp = F.Corpus(hs)
    none = [O.P("zqjzqj"), O.P("wvwvwv")]
    for pats, groups in (([O.P("e")] + none, [0, 1, 1]), (none, [0, 0]), (none + [O.P("e")], [0, 0, 1])):
        assert len(M.compose(pats, groups, hs)) == 0
        assert len(matcher(pats, groups).match_list(cp)) == 0
        assert matcher(pats, groups).match_list_top(cp, 3)[1] == 0


def test_candidate_plus_group_saturates_at_65535():
    big = [5000, 6, 5, 1, 12, 4, 4, 8, 4]  # "dead" scores about 20 000, "deadbe" about 30 000, "e" about 5 000
    hs = make_list("ragged", 1025)
    pats = [O.P("dead", scoring=big), O.P("dead", scoring=big), O.P("beef", scoring=big), O.P("deadbe", scoring=big), O.P("e", scoring=big)]
    groups = [0, 1, 1, 2, 2]
    want = M.match_list(pats, groups, hs, sort="IndexAsc")
    assert (want["score"] == 65535).any() and (want["score"] < 65535).any(), np.unique(want["score"])
    same(matcher(pats, groups, sort="IndexAsc").match_list(F.Corpus(hs)), want, "saturation")


def corpus_with_terms(hs, seed=5):
    rng = np.random.default_rng(seed)
    bias = rng.integers(-40, 300, len(hs)).astype(np.int16)
    tags = rng.integers(0, 16, len(hs)).astype(np.uint16)
    cp = F.Corpus(hs)
    cp.set_bias(bias)
    cp.set_tags(tags)
    return cp, bias, tags


def with_terms(index_asc, bias, tags, scope, sort):
    vis = visible(tags, *scope)
    return biased(index_asc[vis[index_asc["index"]]], bias, sort)


@pytest.mark.parametrize("pname", ("base", "later", "then_negated"))
def test_top_limit_subset_capture_bias_scope_facets_and_sections(pname):
    hs = make_list("ragged", 2049)
    pats, groups = positions(alternatives("fuzzy0", "ragged"), "ragged")[pname]
    index_asc = M.compose(pats, groups, hs)
    found = len(index_asc)
    assert found > 150
    plain = F.Corpus(hs)
    for sort in SORTS:
        fm = matcher(pats, groups, sort=sort)
        want = M.ordered(index_asc, sort)
        for limit in (1, 100, found + 7):
            assert_top(fm.match_list_top(plain, limit), want, limit, (pname, sort))
            recs, words = device_top(fm, plain, limit)
            assert words[:2] == [min(limit, found), found] and recs.tolist() == want[:limit].tolist(), (pname, sort, limit, words)
    # subset= with capture=: the composition over the sub-list, and what it accepted
    rng = np.random.default_rng(9)
    idx = np.flatnonzero(rng.random(len(hs)) < 0.4).astype(np.uint32)
    inside = mask_of(idx, len(hs))
    sub_asc = index_asc[inside[index_asc["index"]]]  # (every term is decided per haystack: the composition over S is the composition, restricted)
    assert 50 < len(sub_asc) < found
    sub, cap = F.Subset(plain), F.Subset(plain)
    sub.set_indices(idx)
    fm = matcher(pats, groups)
    same(fm.match_list(plain, subset=sub, capture=cap), M.ordered(sub_asc, "ScoreThenIndexAsc"), (pname, "subset"))
    assert cap.read().tolist() == sub_asc["index"].tolist()
    assert_top(fm.match_list_top(plain, 100, subset=sub, capture=cap), M.ordered(sub_asc, "ScoreThenIndexAsc"), 100, (pname, "top subset"))
    assert cap.read().tolist() == sub_asc["index"].tolist()
    same(fm.match_list(plain, subset=cap), M.ordered(sub_asc, "ScoreThenIndexAsc"), (pname, "over the capture"))
    # bias, tags and a scope; a facet sink; two overlapping sections
    cp, bias, tags = corpus_with_terms(hs)
    scope = (2, 1)
    sections = [(8, 0), (0, 4)]
    for sort in ("ScoreThenIndexAsc", "IndexDesc"):
        fm = matcher(pats, groups, sort=sort)
        cp.set_scope(0, 0)
        same(fm.match_list(cp), with_terms(index_asc, bias, tags, (0, 0), sort), (pname, sort, "bias"))
        cp.set_scope(*scope)
        want = with_terms(index_asc, bias, tags, scope, sort)
        assert 20 < len(want) < found
        same(fm.match_list(cp), want, (pname, sort, "bias + scope"))
        assert_top(fm.match_list_top(cp, 100), want, 100, (pname, sort, "bias + scope"))
        sink = F.Facets(cp)
        fm.set_facets(sink)
        same(fm.match_list(cp), want, (pname, sort, "sink"))
        check_facets(sink, facet_words(tags[index_asc["index"]], *scope), (pname, sort), found=len(want))
        fm.match_list_top(cp, 5)
        check_facets(sink, facet_words(tags[index_asc["index"]], *scope), (pname, sort, "top"), found=len(want))
        fm.set_facets(None)
        got = fm.match_list_top_sections(cp, sections, 100)
        both = 0
        for (req, exc), (recs, sfound) in zip(sections, got):
            w = want[visible(tags, req, exc)[want["index"]]]
            assert_top((recs, sfound), w, 100, (pname, sort, "section", req, exc))
            both += len(w)
        assert all(f for _, f in got) and both > len(want) // 2  # (neither section is empty; about a quarter of the records are in both)
        cp.set_scope(0, 0)


def test_requery_clone_and_reserve():
    hs = make_list("ragged", 2049)
    cp = F.Corpus(hs)
    a, b = alternatives("fuzzy0", "ragged"), alternatives("suffix", "ragged")
    steps = [(a + [O.P("e")], [0, 0, 0, 1]), (a + [O.P("e")], [0, 1, 1, 2]), (a + b, [0] * 3 + [1] * 3), (a + [O.P("e")], None), (b, [0, 0, 0]), (a[:1] + b, [0, 1, 1, 1])]
    fm = matcher(*steps[0])
    fm.reserve(cp)
    fm.match_list(cp)
    before = F.device_allocs()
    for pats, groups in steps + steps[::-1]:
        fm.set_patterns(hip_patterns(pats), groups=groups)
        same(fm.match_list(cp), M.match_list(pats, groups, hs), ("requery", groups))
        twin = fm.clone()
        assert twin.groups == fm.groups
        same(twin.match_list(cp), M.match_list(pats, groups, hs), ("clone", groups))
    # reserve covers the group's buffers: a matcher that had no group when it was made, reserved once it has one
    fresh = matcher(a + b + [O.P("e")], [0, 0, 0, 1, 1, 1, 2])
    fresh.reserve(cp)
    before = F.device_allocs()
    for pats, groups in ((a + b + [O.P("s")], [0, 0, 0, 1, 1, 1, 2]), (b + a + [O.P("s")], [0, 0, 0, 1, 1, 1, 2]), (a + b + [O.P("s")], [0, 0, 1, 1, 1, 1, 2])):
        fresh.set_patterns(hip_patterns(pats), groups=groups)
        same(fresh.match_list(cp), M.match_list(pats, groups, hs), ("reserved", groups))
        fresh.match_list_top(cp, 10)
    assert F.device_allocs() == before, (F.device_allocs(), before)


def test_a_group_of_one_and_no_grouping_take_the_paths_they_took():
    from test_gpu_small_device import device_of

    hs = make_list("ragged", 2049)
    pats = [O.P("dead"), O.P("e"), O.P("test", negated=True, matching="Substring")]
    with device_of(5):
        cp = F.Corpus(hs)
        F.MultiMatcher(hip_patterns(pats), F.Config(pf_lanes=64)).match_list(cp)  # (what the corpus builds on its first query is built)
        seen = []
        for make in (lambda: F.MultiMatcher(hip_patterns(pats), F.Config(pf_lanes=64)), lambda: matcher(pats, None), lambda: matcher(pats, [4, 9, 2]),
                     lambda: matcher(pats[:1] + [O.P("")] + pats[1:], [0, 0, 1, 2])):  # (the last: a group left with one alternative)
            fm = make()
            before = F.device_allocs()
            F.launch_grids()
            recs = fm.match_list(cp)
            seen.append((recs.tolist(), F.launch_grids(), F.device_allocs() - before))
        assert len(seen[0][0]) > 100 and not any(k.startswith("k_anyof") for k in seen[0][1])
        for other in seen[1:]:
            assert other == seen[0]
        fm = matcher(pats[:2] + [O.P("beef")] + pats[2:], [0, 1, 1, 2])
        fm.match_list(cp)
        grids = F.launch_grids()
        assert {k: v[2] for k, v in grids.items() if k.startswith("k_anyof")} == {"k_anyof_clear": 1, "k_anyof_accumulate": 2, "k_anyof_flag": 1, "k_anyof_compact": 1}, grids


def test_forms_that_do_not_compose_a_group_refuse_it():
    hs = make_list("ragged", 1025)
    cp = F.Corpus(hs)
    pats, groups = positions(alternatives("fuzzy0", "ragged"), "ragged")["later"]
    fm = matcher(pats, groups)
    want = M.match_list(pats, groups, hs)
    calls = {
        "fzb_multi_match_list_indices": lambda: fm.match_list_indices(cp),
        "fzb_multi_match_list_indices_into": lambda: fm._indices_into(cp, 0),
        "fzb_multi_match_list_top_indices": lambda: F._top_indices(F.lib().fzb_multi_match_list_top_indices, fm.h, cp, 5),
        "fzb_multi_match_list_top_indices_fused": lambda: fm.match_list_top_indices(cp, 5),
        "fzb_multi_match_list_top_indices_device": lambda: fm.match_list_top_indices_device(cp, 5, 64, 5, 64, 400, 64),
        "fzb_multi_match_list_top_sections_indices": lambda: fm.match_list_top_sections_indices(cp, [(0, 0)], 5),
        "fzb_multi_match_list_top_sections_indices_device": lambda: fm.match_list_top_sections_indices_device(cp, [(0, 0)], 5, 64, 5, 64, 400, 64),
    }
    sub = F.Subset(cp)
    sub.set_indices(np.arange(10, dtype=np.uint32))
    calls["fzb_multi_match_list_top_indices_subset"] = lambda: fm.match_list_top_indices(cp, 5, subset=sub)
    sharded = F.ShardedCorpus(hs, ndev=1)
    calls["fzb_multi_match_list_parallel_sharded"] = lambda: fm.match_list_parallel_sharded(sharded)
    calls["fzb_multi_match_list_top_sharded"] = lambda: fm.match_list_top_sharded(sharded, 5)
    for name, call in calls.items():
        with pytest.raises(F.FrizbeeError) as e:
            call()
        assert e.value.code == 1 and name in str(e.value) and "any-of group" in str(e.value), (name, str(e.value))
    # the RCCL form: refused ahead of the library's load and of the communicator (a handle it never reads)
    out, n = C.c_void_p(), C.c_size_t()
    fake = C.c_void_p(64)
    assert F.lib().fzb_multi_match_list_parallel_rccl(fm.h, cp.h, 0, fake, 0, C.byref(out), C.byref(n)) == 1
    assert b"fzb_multi_match_list_parallel_rccl" in F.lib().fzb_last_error() and b"any-of group" in F.lib().fzb_last_error()
    same(fm.match_list(cp), want, "after the refusals")
    fm.set_patterns(hip_patterns(pats))  # every pattern a single term again: served
    assert fm.match_list_top_indices(cp, 5)[1] == len(O.MultiMatcher(pats, lanes=M.LANES).match_list(hs))
