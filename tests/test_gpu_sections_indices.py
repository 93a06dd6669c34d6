"""Sectioned top-`limit` WITH matched positions (fzb_match_list_top_sections_indices and its siblings; k_sec_items in kernels_sections.hip):
element s is what `match_list_top_indices(corpus, limit)` returns over a corpus whose scope is the corpus' own scope AND section s's
predicate.  Every expected value is the ORACLE's: the records and their order are tests/test_gpu_sections.py's `want_list` (the oracle's
`match_list` over the sub-list of the haystacks visible under the corpus scope and the section, mapped back, bias and ordering rule added in
numpy), and the positions of a record are the oracle's `match_list_indices` over the WHOLE list, looked up by full-list index - the positions
of a haystack do not depend on the list around it (tests/test_gpu_scope.py::test_scope_and_bias_together_with_ties_at_the_cut does the same).
Never this library's own output.  The list is test_gpu_facets' (20 517 haystacks of 16 bytes, random 16-bit tags, bias +-300, a one-in-three
subset).

A note on position counts.  On that list every match of `deadbe` with max_typos=1 carries six positions (by the oracle: the rows hold the
letters g-v and x, so only the planted rows match, and they match every needle byte), `g` carries one and `dead !x` four: no head of it has
records with different position counts, whatever is under test.  The pack's scan is only exercised by such heads, so
test_heads_with_different_position_counts runs on the SAME list with one needle byte of every third planted row overwritten (tags, bias and
subset unchanged), where the oracle reports five and six positions, and asserts that from the oracle's data first."""
import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from facets_model import facet_words
from test_gpu_facets import Data, N
from test_gpu_parity import LANES
from test_gpu_scope import mapped, sub_list, visible
from test_gpu_score_bias import biased
from test_gpu_sections import QUERY, SCOPES, SECTIONS, corpus, limits_for, multi_of, oracle_of, relies_on, want_list
from test_gpu_topk import SORTS, single

pytestmark = pytest.mark.gpu
S = len(SECTIONS)
FZB_ERR_INVALID, FZB_ERR_CAPACITY = 1, 5
_POS = {}


def positions_of(query):
    """full-list index -> the oracle's matched positions (descending), from ONE `match_list_indices` over the whole list per query"""
    if query not in _POS:
        recs, idx = oracle_of(query, "IndexAsc").match_list_indices(Data.get()["hs"])
        _POS[query] = {int(r["index"]): ix for r, ix in zip(recs, idx)}
    return _POS[query]


def tuples(ms):
    return [(m.index, m.score, m.exact, m.indices) for m in ms]


def expected(w, pos, limit):
    return [(int(r["index"]), int(r["score"]), bool(r["exact"]), pos[int(r["index"])]) for r in w[:limit]]


def assert_sections_indices(got, wants, pos, limit, ctx):
    assert len(got) == len(wants), (ctx, len(got))
    for s, ((recs, found), w) in enumerate(zip(got, wants)):
        assert found == len(w), (ctx, "section", s, found, len(w))
        got_t, exp = tuples(recs), expected(w, pos, limit)
        if got_t != exp:
            bad = [(i, g, e) for i, (g, e) in enumerate(zip(got_t, exp)) if g != e][:4]
            raise AssertionError(f"{ctx} section {s} limit {limit}: len {len(got_t)} vs {len(exp)}; first diffs (at, got, want) {bad}")


def totals(wants, limit):
    return sum(min(limit, len(w)) for w in wants)


@pytest.mark.parametrize("scope", sorted(SCOPES))
@pytest.mark.parametrize("use_bias", (False, True), ids=("plain", "bias"))
@pytest.mark.parametrize("sort", SORTS)
def test_eight_sections_with_positions_against_the_oracle(sort, use_bias, scope):
    cp = corpus(SCOPES[scope], use_bias)
    for needle in ("deadbe", "g"):
        pos = positions_of(needle)
        wants = [want_list(needle, sort, SCOPES[scope], sec, use_bias) for sec in SECTIONS]
        limits = limits_for(wants)
        assert {0, 1, 5, 100, 1024} <= set(limits)
        assert {"ties", "keep_all", "empty"} <= relies_on(wants, limits, sort), (needle, [len(w) for w in wants])
        assert any(len(w) == 0 for w in wants) and any(0 < len(w) <= max(limits) for w in wants)  # an empty section and a keep-all one
        # both pack forms run: the one-launch pack takes heads of up to 2048 records, the tiled one longer heads
        assert S * 1024 > 2048 >= S * 100 and totals(wants, 100) < 2048
        if needle == "g":
            assert totals(wants, 1024) > 2048
        fm, _ = single(needle, sort=sort)
        for limit in limits:
            assert_sections_indices(fm.match_list_top_sections_indices(cp, SECTIONS, limit), wants, pos, limit, (needle, sort, use_bias, scope, limit))


def test_overlapping_sections_share_records_with_their_positions():
    """a haystack that sits in several sections appears in each head, with its positions: asserted from the oracle's lists first"""
    cp = corpus((0, 0), True)
    for sort in ("ScoreThenIndexAsc", "IndexDesc"):
        for matcher, query in ((single("deadbe", sort=sort)[0], "deadbe"), (multi_of(sort), QUERY)):
            wants = [want_list(query, sort, (0, 0), sec, True) for sec in SECTIONS]
            for limit in (20, 1024):
                heads = [set(w["index"][:limit].tolist()) for w in wants]
                assert heads[0] & heads[2] and heads[0] == heads[5] and heads[1] & heads[2], "sections (1, 0), (0, 0), (1, 0) again and (2, 1) share records"
                assert_sections_indices(matcher.match_list_top_sections_indices(cp, SECTIONS, limit), wants, positions_of(query), limit, (query, sort, limit))


def test_everything_is_the_oracles_match_list_indices_cut_at_limit():
    """(0, 0) alone over an unscoped, unbiased corpus: the oracle's `match_list_indices_ordered` over the whole list, cut at `limit`"""
    d = Data.get()
    cp = corpus()
    for sort in SORTS:
        for query, matcher in (("deadbe", single("deadbe", sort=sort)[0]), ("g", single("g", sort=sort)[0]), (QUERY, multi_of(sort))):
            want = oracle_of(query, sort).match_list_indices_ordered(d["hs"])
            assert len(want) > 1024
            for limit in (0, 1, 20, 1024):
                (recs, found), = matcher.match_list_top_sections_indices(cp, [(0, 0)], limit)
                assert found == len(want) and tuples(recs) == want[:limit], (query, sort, limit)
    assert single("g")[0].match_list_top_sections_indices(cp, [], 5) == []
    for matcher in (single("g")[0], multi_of("IndexAsc")):  # an empty corpus: S empty heads
        assert [(r, f) for r, f in matcher.match_list_top_sections_indices(F.Corpus([]), SECTIONS[:3], 5)] == [([], 0)] * 3


@pytest.mark.parametrize("use_bias", (False, True), ids=("plain", "bias"))
def test_query_syntax_with_positions(use_bias):
    """`dead !x`: the positions are the union over the non-negated patterns; overlapping sections repeat items in front of k_multi_union"""
    pos = positions_of(QUERY)
    for scope in SCOPES.values():
        cp = corpus(scope, use_bias)
        for sort in SORTS:
            wants = [want_list(QUERY, sort, scope, sec, use_bias) for sec in SECTIONS]
            limits = limits_for(wants)
            assert {"ties", "keep_all", "empty"} <= relies_on(wants, limits, sort), [len(w) for w in wants]
            assert set(wants[0]["index"][:5].tolist()) <= set(wants[5]["index"][:5].tolist())  # repeated items inside one head list
            fm = multi_of(sort)
            for limit in limits:
                assert_sections_indices(fm.match_list_top_sections_indices(cp, SECTIONS, limit), wants, pos, limit, ("dead !x", sort, scope, limit))


def damaged_list():
    """test_gpu_facets' list with one needle byte of every third planted row overwritten: `deadbe` with one typo then matches with 5 or 6 positions"""
    hs = list(Data.get()["hs"])
    planted = [i for i, h in enumerate(hs) if h[3:9] == b"deadbe"]
    for i in planted[::3]:
        hs[i] = hs[i][:5] + b"q" + hs[i][6:]
    return hs


@pytest.mark.parametrize("sort", ("ScoreThenIndexAsc", "IndexDesc"))
def test_heads_with_different_position_counts(sort):
    d = Data.get()
    hs = damaged_list()
    om = O.Matcher("deadbe", lanes=LANES[64], sort="IndexAsc", max_typos=1)
    recs, idx = om.match_list_indices(hs)
    pos = {int(r["index"]): ix for r, ix in zip(recs, idx)}
    wants = []
    for sec in SECTIONS:
        vis = visible(d["tags"], *sec)
        sub = sub_list(hs, vis)
        wants.append(biased(mapped(om.match_list(sub), vis), d["bias"], sort) if sub else np.zeros(0, F.MATCH_DTYPE))
    cp = F.Corpus(hs)
    cp.set_tags(d["tags"])
    cp.set_bias(d["bias"])
    fm, _ = single("deadbe", sort=sort, max_typos=1)
    for limit in (7, 100, 1024):
        counts = [{len(pos[int(i)]) for i in w["index"][:limit]} for w in wants]
        assert any(len(c) >= 2 for c in counts) and set().union(*counts) == {5, 6}, "the heads carry two different position counts, one head both"
        assert totals(wants, 1024) > 2048 > totals(wants, 100)
        assert_sections_indices(fm.match_list_top_sections_indices(cp, SECTIONS, limit), wants, pos, limit, ("one typo", sort, limit))


def test_subset_and_capture():
    d = Data.get()
    scope = (2, 1)
    cp = corpus(scope, True)
    sub, cap, cap_plain = F.Subset(cp), F.Subset(cp), F.Subset(cp)
    sub.set_indices(d["sub"])
    a = np.intersect1d(Data.matches("deadbe"), d["sub"]).astype(np.uint32)  # the capture: the match set inside the subset, ahead of the scope
    assert 10 < len(a) < len(Data.matches("deadbe"))
    sort = "ScoreThenIndexDesc"
    wants = [want_list("deadbe", sort, scope, sec, True, True) for sec in SECTIONS]
    assert {"ties", "keep_all", "empty"} <= relies_on(wants, (5, 100), sort)
    fm, _ = single("deadbe", sort=sort)
    for limit in (5, 100):
        assert_sections_indices(fm.match_list_top_sections_indices(cp, SECTIONS, limit, subset=sub, capture=cap), wants, positions_of("deadbe"), limit, ("subset", limit))
        fm.match_list_top(cp, limit, subset=sub, capture=cap_plain)
        assert np.array_equal(cap.read(), cap_plain.read()) and np.array_equal(cap.read(), a)
    # the composition: subset and capture behind `dead !x`
    wants = [want_list(QUERY, sort, scope, sec, True, True) for sec in SECTIONS]
    mm = multi_of(sort)
    assert_sections_indices(mm.match_list_top_sections_indices(cp, SECTIONS, 100, subset=sub, capture=cap), wants, positions_of(QUERY), 100, ("dead !x", "subset"))
    mm.match_list_top(cp, 100, subset=sub, capture=cap_plain)
    assert len(cap.read()) > 10 and np.array_equal(cap.read(), cap_plain.read())


def test_an_attached_facet_sink_counts_what_the_plain_call_counts():
    d = Data.get()
    scope = (2, 1)
    cp = corpus(scope, True)
    sink = F.Facets(cp)
    a = Data.matches("g")
    want_words = facet_words(d["tags"][a], *scope)
    assert want_words[0] > want_words[1] > 0
    fm, _ = single("g")
    fm.set_facets(sink)
    wants = [want_list("g", "ScoreThenIndexAsc", scope, sec, True) for sec in SECTIONS]
    assert_sections_indices(fm.match_list_top_sections_indices(cp, SECTIONS, 250), wants, positions_of("g"), 250, "sink")
    assert sink.read_words().tolist() == want_words.tolist()


def device_sections_indices(matcher, cp, sections, limit, stride, extra=3, **kw):
    """the _device form -> (records with `extra` guard records, positions with `extra` guard words, the 2S + 4 words with two guard words)"""
    import torch

    want = len(sections) * min(limit, N)
    out = torch.full(((want + extra) * 16,), 0xEE, dtype=torch.uint8, device="cuda")
    pos = torch.full((want * stride + extra,), -3, dtype=torch.int32, device="cuda")
    cnt = torch.full((2 * len(sections) + 6,), -7, dtype=torch.int32, device="cuda")
    matcher.match_list_top_sections_indices_device(cp, sections, limit, out.data_ptr(), want, pos.data_ptr(), want * stride, cnt.data_ptr(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), pos.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("sort", ("ScoreThenIndexDesc", "IndexAsc"))
def test_the_device_forms(sort):
    import torch

    cp = corpus((0, 0), True)
    fm, _ = single("deadbe", sort=sort)
    for matcher, query, stride in ((fm, "deadbe", 6), (multi_of(sort), QUERY, 4)):
        posd = positions_of(query)
        wants = [want_list(query, sort, (0, 0), sec, True) for sec in SECTIONS]
        for limit in (0, 7, 300):
            raw, dense, cnt = device_sections_indices(matcher, cp, SECTIONS, limit, stride)
            want = S * limit
            assert (raw[want * 16:] == 0xEE).all() and (dense[want * stride:] == -3).all() and (cnt[2 * S + 4:] == -7).all(), "wrote beyond the stated room"
            kept = [min(limit, len(w)) for w in wants]
            assert cnt[:2 * S].tolist() == [x for k, w in zip(kept, wants) for x in (k, len(w))], (query, limit, cnt)
            assert cnt[2 * S] == sum(kept) and cnt[2 * S + 3] == 0
            recs = raw[: sum(kept) * 16].view(F.MATCH_INDICES_DTYPE)
            exp = [t for w in wants for t in expected(w, posd, limit)]  # the heads, densely concatenated in section order
            assert cnt[2 * S + 2] == sum(len(t[3]) for t in exp)
            begins = np.concatenate([[0], np.cumsum([len(t[3]) for t in exp])])[:len(exp)]
            assert recs["positions_begin"].tolist() == begins.tolist(), "the positions are dense over the whole block"
            got = [(int(r["index"]), int(r["score"]), bool(r["exact"]), dense[int(r["positions_begin"]):int(r["positions_begin"]) + int(r["positions_len"])].tolist()) for r in recs]
            assert got == exp, (query, sort, limit)
        # room short by one record, positions short by one dword: FZB_ERR_CAPACITY, nothing is written
        want = S * 7
        out = torch.full((want * 16,), 0xEE, dtype=torch.uint8, device="cuda")
        dense = torch.full((want * stride,), -3, dtype=torch.int32, device="cuda")
        cnt = torch.full((2 * S + 4,), -7, dtype=torch.int32, device="cuda")
        for cap, pcap in ((want - 1, want * stride), (want, want * stride - 1)):
            with pytest.raises(F.FrizbeeError) as e:
                matcher.match_list_top_sections_indices_device(cp, SECTIONS, 7, out.data_ptr(), cap, dense.data_ptr(), pcap, cnt.data_ptr())
            assert e.value.code == FZB_ERR_CAPACITY
        torch.cuda.synchronize()
        assert (out == 0xEE).all() and (dense == -3).all() and (cnt == -7).all()
        # on a stream of the caller's the call is ordered
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            matcher.match_list_top_sections_indices_device(cp, SECTIONS, 7, out.data_ptr(), want, dense.data_ptr(), want * stride, cnt.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        kept = [min(7, len(w)) for w in wants]
        assert cnt[:2 * S:2].tolist() == kept and cnt[2 * S].item() == sum(kept) and cnt[2 * S + 3].item() == 0
        recs = out.cpu().numpy()[: sum(kept) * 16].view(F.MATCH_INDICES_DTYPE)
        assert recs["index"].tolist() == [int(i) for w in wants for i in w["index"][:7]]


def test_the_empty_needle_and_the_empty_pattern_list():
    """the host forms answer with the prompt's records and no positions; the _device forms refuse and name the host form"""
    import torch

    cp = corpus((2, 1), True)
    buf = torch.zeros(4096, dtype=torch.int32, device="cuda")
    for sort in ("ScoreThenIndexAsc", "IndexDesc"):
        wants = [want_list("", sort, (2, 1), sec, True) for sec in SECTIONS]
        assert {"ties", "empty"} <= relies_on(wants, (1, 100), sort)
        none = {int(i): [] for w in wants for i in w["index"][:100]}
        for matcher, host in ((single("", sort=sort)[0], "fzb_match_list_top_sections_indices"),
                              (F.MultiMatcher([], F.Config(sort=F.SortStrategy[sort], pf_lanes=64)), "fzb_multi_match_list_top_sections_indices")):
            for limit in (0, 1, 100):
                assert_sections_indices(matcher.match_list_top_sections_indices(cp, SECTIONS, limit), wants, none, limit, ("empty", sort, limit))
            with pytest.raises(F.FrizbeeError) as e:
                matcher.match_list_top_sections_indices_device(cp, SECTIONS, 5, buf.data_ptr(), 64, buf.data_ptr() + 4096, 64, buf.data_ptr() + 8192)
            assert e.value.code == FZB_ERR_INVALID and host in str(e.value) and host + "_device" not in str(e.value)


def test_no_device_allocation_on_the_second_call():
    cp = corpus((2, 1), True)
    pos = positions_of("deadbe")
    wants = [want_list("deadbe", "ScoreThenIndexAsc", (2, 1), sec, True) for sec in SECTIONS]
    fm, _ = single("deadbe")
    fm.reserve(cp)
    fm.reserve_top_indices(cp, 300, 6)
    first = fm.match_list_top_sections_indices(cp, SECTIONS, 300)
    before = F.device_allocs()
    second = fm.match_list_top_sections_indices(cp, SECTIONS, 300)
    third = fm.match_list_top_sections_indices(cp, SECTIONS[:3], 20)
    assert F.device_allocs() == before
    assert_sections_indices(first, wants, pos, 300, "first")
    assert_sections_indices(second, wants, pos, 300, "second")
    assert_sections_indices(third, wants[:3], pos, 20, "smaller")
