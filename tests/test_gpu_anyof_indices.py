"""Matched positions of the top-`limit` for a matcher with any-of groups (`MultiMatcher.match_list_top_indices_groups` and its device
form) against the model of tests/anyof_indices_model.py: the head of tests/anyof_model.py, every pattern's positions from the oracle on its
own, the carrier rule and the descending unique union stated once in Python (held to the reference by
tests/test_oracle_anyof_indices_premise.py).  Compared on index, score, exact, `found` and the positions of every record.  Terms around the
composition (bias, scope, subset, capture, facets) are applied to the model's head in numpy, as tests/test_gpu_anyof.py does."""
import numpy as np
import pytest

import anyof_indices_model as MI
import anyof_model as M
import frizbee_amd as F
import oracle_lib as O
from test_gpu_anyof import alternatives, classes, corpus_with_terms, hip_patterns, make_list, matcher, positions, with_terms
from test_gpu_small_device import device_of
from test_gpu_subset import mask_of
from test_gpu_topk import SORTS

pytestmark = pytest.mark.gpu
IPACK_TILE = 2048


def tuples(res):
    recs, found = res
    return [(r.index, r.score, bool(r.exact), list(r.indices)) for r in recs], found


def assert_same(got, want, ctx):
    (grecs, gfound), (wrecs, wfound) = got, want
    assert gfound == wfound, (ctx, gfound, wfound)
    if grecs != wrecs:
        bad = [(k, g, w) for k, (g, w) in enumerate(zip(grecs, wrecs)) if g != w][:4]
        raise AssertionError(f"{ctx}: len {len(grecs)} vs {len(wrecs)}; first diffs (at, got, want) {bad}")


def head_classes(alts, head, hs):
    """of the head's records: matched by exactly one alternative, by several, and with max-scoring alternatives that differ in the exact flag"""
    hits = [M.pattern_hits(p, hs, {}) for p in alts]
    one = several = tie = 0
    for i, *_ in head:
        v = [h[i] for h in hits if i in h]
        one += len(v) == 1
        several += len(v) > 1
        tie += len({e for s, e in v if s == max(x[0] for x in v)}) == 2
    return dict(one=one, several=several, tie=tie)


CASES = [(kind, n, a) for kind in ("ragged", "uniform32") for n in (1025, 2049) for a in ("fuzzy0", "fuzzy1", "suffix", "tie")] + [("utf8", 1025, "unicode")]


@pytest.mark.parametrize("kind,n,aname", CASES)
def test_parity_with_the_model(kind, n, aname):
    hs = make_list(kind, n)
    cp = F.Corpus(hs)
    alts = alternatives(aname, kind)
    largest = 0
    for pname, (pats, groups) in positions(alts, kind).items():
        fm = matcher(pats, groups)
        assert fm.groups_positions_stride() == MI.stride(pats, groups)
        for sort in SORTS:
            fm.set_config(F.Config(sort=F.SortStrategy[sort], pf_lanes=64))
            every, found = MI.match_list_top_indices(pats, groups, hs, len(hs), sort=sort)
            largest = max(largest, found)
            if pname == "base" and sort == "IndexAsc":  # the head says something about the carrier rule: every class of record is in it
                c = head_classes(alts, every, hs)
                if aname == "tie":  # (only the planted haystack holds the whole needle of the uniform list)
                    assert c["several"] and c["tie"] >= 1, (pname, c)
                else:
                    assert c["one"] and (c["several"] or aname == "suffix"), (pname, c)  # (a haystack has one suffix)
            for limit in (1, 5, 257, len(hs)):  # 257: one more than the merge kernel's 256-thread block; len(hs): the head is every match
                assert_same(tuples(fm.match_list_top_indices_groups(cp, limit)), (every[:limit], found), (kind, n, aname, pname, sort, limit))
    # the pack's single-launch form takes heads of up to IPACK_TILE records.  No alternative matches every haystack of these lists, so the
    # largest head reached here stays within one tile; the longer head is test_a_head_beyond_one_pack_tile's
    print("largest head", kind, n, aname, largest)
    assert 0 < largest <= IPACK_TILE, largest


def test_a_head_beyond_one_pack_tile():
    hs = make_list("ragged", 8193)
    cp = F.Corpus(hs)
    pats, groups = positions(alternatives("fuzzy0", "ragged"), "ragged")["base"]
    for sort in ("ScoreThenIndexAsc", "IndexDesc"):
        every, found = MI.match_list_top_indices(pats, groups, hs, len(hs), sort=sort)
        assert found > IPACK_TILE + 256, found
        c = head_classes(alternatives("fuzzy0", "ragged"), every, hs)
        assert c["one"] > 100 and c["several"] > 100, c
        fm = matcher(pats, groups, sort=sort)
        for limit in (IPACK_TILE, IPACK_TILE + 1, len(hs)):
            assert_same(tuples(fm.match_list_top_indices_groups(cp, limit)), (every[:limit], found), (sort, limit))


# `ab` and `cd` on the haystack `_ab_cd`: both follow a delimiter, both score 36 without the exact flag, at positions [2, 1] and [5, 4].  Found on
# the CPU by running the oracle over every ordered pair of the needles ab, cd, ba, dc, ac, bd on a handful of short haystacks and keeping the
# pairs with equal (score, exact) and different positions.
EQUAL_KEYS = ("_ab_cd", "ab", "cd", [2, 1], [5, 4])


def test_query_order_decides_only_on_equal_keys():
    h, a, b, pa, pb = EQUAL_KEYS
    hs = make_list("ragged", 1025)[:300] + [h.encode()]
    at = len(hs) - 1
    cp = F.Corpus(hs)
    ra, rb = MI.pattern_indices(O.P(a), hs, {})[at], MI.pattern_indices(O.P(b), hs, {})[at]
    assert ra[:2] == rb[:2] and ra[2] == pa and rb[2] == pb  # the premise: equal keys, different positions
    for order, first in (([O.P(a), O.P(b)], pa), ([O.P(b), O.P(a)], pb)):
        want = MI.match_list_top_indices(order, [0, 0], hs, len(hs), sort="IndexAsc")
        got = tuples(matcher(order, [0, 0], sort="IndexAsc").match_list_top_indices_groups(cp, len(hs)))
        assert_same(got, want, order)
        rec = [g for g in got[0] if g[0] == at]
        assert rec == [(at, ra[0], bool(ra[1]), first)], rec  # the positions follow the first alternative
    # the tie alternatives: equal scores, different exact flags - the positions follow the exact one in either order
    for kind in ("ragged", "uniform32"):
        hs = make_list(kind, 1025)
        cp = F.Corpus(hs)
        alts = alternatives("tie", kind)
        solo = [MI.pattern_indices(p, hs, {})[0] for p in alts]
        assert solo[0][0] == solo[1][0] and (solo[0][1], solo[1][1]) == (1, 0) and solo[0][2] != solo[1][2], solo  # the premise, on haystack 0
        for order in (alts, alts[::-1]):
            want = MI.match_list_top_indices(order, [0, 0], hs, len(hs), sort="IndexAsc")
            got = tuples(matcher(order, [0, 0], sort="IndexAsc").match_list_top_indices_groups(cp, len(hs)))
            assert_same(got, want, (kind, "tie"))
            assert got[0][0] == (0, solo[0][0], True, solo[0][2])


def test_more_than_eight_sources_take_the_device_memory_path():
    hs = make_list("ragged", 2049)
    five_a = [O.P("dead"), O.P("beef"), O.P("cafe"), O.P("daed"), O.P("cfe")]
    five_b = [O.P("rs", matching="Suffix"), O.P("py", matching="Suffix"), O.P("go", matching="Suffix"), O.P("src/"), O.P("e")]
    pats, groups = five_a + five_b, [0] * 5 + [1] * 5
    with device_of(5):
        cp = F.Corpus(hs)
        fm = matcher(pats, groups)
        for limit in (5, 600):
            want = MI.match_list_top_indices(pats, groups, hs, limit)
            assert want[1] > 600
            F.launch_grids()
            got = tuples(fm.match_list_top_indices_groups(cp, limit))
            grids = F.launch_grids()
            assert grids["k_gunion_merge"][2] == 1 and "k_multi_union" not in grids, grids
            assert_same(got, want, limit)
        c = head_classes(five_a, want[0], hs)
        assert c["one"] and c["several"], c
        fm.set_patterns(hip_patterns(pats[:6]), groups=[0] * 5 + [1])  # and back under the bound on the same matcher
        assert_same(tuples(fm.match_list_top_indices_groups(cp, 100)), MI.match_list_top_indices(pats[:6], [0] * 5 + [1], hs, 100), "six sources")


def test_an_ungrouped_matcher_takes_the_path_it_took():
    hs = make_list("ragged", 2049)
    pats = [O.P("dead"), O.P("e"), O.P("test", negated=True, matching="Substring")]
    with device_of(5):
        cp = F.Corpus(hs)
        sub = F.Subset(cp)
        sub.set_indices(np.arange(0, 2049, 2, dtype=np.uint32))
        matcher(pats, None).match_list_top_indices(cp, 50)  # (what the corpus builds on its first query is built)
        seen = []
        for call in (lambda fm: fm.match_list_top_indices(cp, 50), lambda fm: fm.match_list_top_indices_groups(cp, 50),
                     lambda fm: fm.match_list_top_indices(cp, 50, subset=sub), lambda fm: fm.match_list_top_indices_groups(cp, 50, subset=sub)):
            fm = matcher(pats[:1] + [O.P("")] + pats[1:], [0, 0, 1, 2])  # (a group left with one alternative is that plain pattern)
            before = F.device_allocs()
            F.launch_grids()
            got = tuples(call(fm))
            seen.append((got, F.launch_grids(), F.device_allocs() - before))
        assert seen[0] == seen[1] and seen[2] == seen[3] and seen[0][0] != seen[2][0]
        assert len(seen[0][0][0]) == 50 and "k_multi_union" in seen[1][1] and not any(k.startswith("k_gunion") for s in seen for k in s[1])
        want = O.MultiMatcher(pats, lanes=M.LANES).match_list_indices_ordered(hs)
        assert seen[1][0] == ([(i, s, e, list(ix)) for i, s, e, ix in want[:50]], len(want))


def test_launches_of_a_grouped_call_and_no_allocation_on_a_second_one():
    hs = make_list("ragged", 2049)
    a, b = alternatives("fuzzy0", "ragged"), alternatives("suffix", "ragged")
    steps = [(a + b + [O.P("e")], [0, 0, 0, 1, 1, 1, 2]), (b + a + [O.P("s")], [0, 0, 0, 1, 1, 1, 2]), (a + b + [O.P("s")], [0, 0, 1, 1, 1, 1, 2]), (a + b + [O.P("e")], [0, 1, 2, 3, 3, 4, 5])]
    with device_of(5):
        cp = F.Corpus(hs)
        fm = matcher(*steps[0])
        fm.reserve(cp)
        fm.reserve_top_indices_groups(cp, 300, 8)
        F.launch_grids()
        assert_same(tuples(fm.match_list_top_indices_groups(cp, 300)), MI.match_list_top_indices(*steps[0], hs, 300), "first")
        grids = F.launch_grids()
        assert {k: v[2] for k, v in grids.items() if k.startswith("k_gunion")} == {"k_gunion_slots": 1, "k_gunion_clear": 1, "k_gunion_where": 1, "k_gunion_merge": 1}, grids
        assert "k_multi_union" not in grids
        before = F.device_allocs()
        for pats, groups in steps + steps[::-1]:
            fm.set_patterns(hip_patterns(pats), groups=groups)
            for limit in (300, 7):
                assert_same(tuples(fm.match_list_top_indices_groups(cp, limit)), MI.match_list_top_indices(pats, groups, hs, limit), (groups, limit))
        assert F.device_allocs() == before, (F.device_allocs(), before)


def test_around_the_composition_bias_scope_facets_subset_and_capture():
    hs = make_list("ragged", 2049)
    pats, groups = positions(alternatives("fuzzy0", "ragged"), "ragged")["later"]
    index_asc = M.compose(pats, groups, hs)
    found = len(index_asc)
    assert found > 150
    plain = F.Corpus(hs)
    # subset= with capture=: only the top stage sees the set; the capture is match_list_top's
    idx = np.flatnonzero(np.random.default_rng(9).random(len(hs)) < 0.4).astype(np.uint32)
    sub_asc = index_asc[mask_of(idx, len(hs))[index_asc["index"]]]
    assert 50 < len(sub_asc) < found
    sub, cap, cap2 = F.Subset(plain), F.Subset(plain), F.Subset(plain)
    sub.set_indices(idx)
    fm = matcher(pats, groups)
    want = M.ordered(sub_asc, "ScoreThenIndexAsc")
    got = tuples(fm.match_list_top_indices_groups(plain, 100, subset=sub, capture=cap))
    assert_same(got, (MI.with_positions(want[:100], pats, groups, hs), len(want)), "subset + capture")
    fm.match_list_top(plain, 100, subset=sub, capture=cap2)
    assert cap.read().tolist() == cap2.read().tolist() == sub_asc["index"].tolist()
    # bias, then a scope, then a facet sink
    cp, bias, tags = corpus_with_terms(hs)
    scope = (2, 1)
    for sort in ("ScoreThenIndexAsc", "IndexDesc"):
        fm = matcher(pats, groups, sort=sort)
        cp.set_scope(0, 0)
        want = with_terms(index_asc, bias, tags, (0, 0), sort)
        assert_same(tuples(fm.match_list_top_indices_groups(cp, 100)), (MI.with_positions(want[:100], pats, groups, hs), len(want)), (sort, "bias"))
        cp.set_scope(*scope)
        want = with_terms(index_asc, bias, tags, scope, sort)
        assert 20 < len(want) < found
        assert_same(tuples(fm.match_list_top_indices_groups(cp, 100)), (MI.with_positions(want[:100], pats, groups, hs), len(want)), (sort, "bias + scope"))
        sink = F.Facets(cp)
        fm.set_facets(sink)
        fm.match_list_top(cp, 100)
        records_form = sink.read_words().tolist()
        assert records_form[0] == found and records_form[1] == len(want)
        other = F.Facets(cp)
        fm.set_facets(other)
        assert_same(tuples(fm.match_list_top_indices_groups(cp, 100)), (MI.with_positions(want[:100], pats, groups, hs), len(want)), (sort, "sink"))
        assert other.read_words().tolist() == records_form
        fm.set_facets(None)
        cp.set_scope(0, 0)


def test_the_device_form():
    import torch

    hs = make_list("ragged", 2049)
    cp = F.Corpus(hs)
    pats, groups = positions(alternatives("fuzzy0", "ragged"), "ragged")["two_groups"]
    fm = matcher(pats, groups)
    U = fm.groups_positions_stride()
    assert U == MI.stride(pats, groups) == 4 + 1
    for limit in (1, 300, len(hs)):
        host, found = tuples(fm.match_list_top_indices_groups(cp, limit))
        cap = min(limit, len(cp))
        out = torch.zeros((cap, 4), dtype=torch.int32, device="cuda")
        pos = torch.full((cap * U,), -1, dtype=torch.int32, device="cuda")
        cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        fm.match_list_top_indices_groups_device(cp, limit, out.data_ptr(), cap, pos.data_ptr(), cap * U, cnt.data_ptr())
        torch.cuda.synchronize()
        words = cnt.cpu().numpy().view(np.uint32).tolist()
        total = sum(len(h[3]) for h in host)
        assert words == [len(host), found, total, 0], (limit, words)
        recs = out.cpu().numpy().reshape(-1).view(F.MATCH_INDICES_DTYPE)[: words[0]]
        flat = pos.cpu().numpy().view(np.uint32)
        assert recs["positions_begin"].tolist() == np.cumsum([0] + [len(h[3]) for h in host])[:-1].tolist()  # dense
        assert (flat[total:] == 0xFFFFFFFF).all()  # nothing is written behind the total
        got = [(int(r["index"]), int(r["score"]), bool(r["exact"]), flat[int(r["positions_begin"]): int(r["positions_begin"]) + int(r["positions_len"])].tolist()) for r in recs]
        assert got == host, limit
    assert_same((host, found), MI.match_list_top_indices(pats, groups, hs, len(hs)), "host form")
    # a positions buffer one word short of want x U_g, or room for one record too few: refused on the host, nothing launched
    for cap, pcap in ((11, 11 * U - 1), (10, 11 * U)):
        out = torch.zeros((11, 4), dtype=torch.int32, device="cuda")
        pos = torch.zeros((11 * U,), dtype=torch.int32, device="cuda")
        cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        with pytest.raises(F.FrizbeeError) as e:
            fm.match_list_top_indices_groups_device(cp, 11, out.data_ptr(), cap, pos.data_ptr(), pcap, cnt.data_ptr())
        assert e.value.code == 5  # FZB_ERR_CAPACITY
        torch.cuda.synchronize()
        assert cnt.cpu().tolist() == [-1, -1, -1, -1]
    # an empty corpus zeroes the four words; limit 0 returns nothing
    fm.match_list_top_indices_groups_device(F.Corpus([]), 5, out.data_ptr(), 11, pos.data_ptr(), 11 * U, cnt.data_ptr())
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [0, 0, 0, 0]
    assert tuples(fm.match_list_top_indices_groups(F.Corpus([]), 5)) == ([], 0)
    recs, found = tuples(fm.match_list_top_indices_groups(cp, 0))
    assert recs == [] and found == MI.match_list_top_indices(pats, groups, hs, 0)[1]
    # the existing form keeps refusing a grouped matcher
    with pytest.raises(F.FrizbeeError) as e:
        fm.match_list_top_indices(cp, 5)
    assert e.value.code == 1 and "any-of group" in str(e.value)
