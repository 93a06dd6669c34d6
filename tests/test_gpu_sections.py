"""Sectioned top-`limit` (fzb_match_list_top_sections and its siblings; sections.h, kernels_sections.hip): the best matches per tag section
from one device call.  The contract: element s is what `match_list_top(corpus, limit)` returns over a corpus whose scope is the corpus' own
scope AND section s's predicate.  So every expected value is the ORACLE's `match_list` over the sub-list of the haystacks visible under the
corpus scope and section s (and inside the candidate set, where there is one), every index mapped back to the full list's - with the bias
and the reference's ordering rule added in numpy where a bias is present - cut to `limit`; `found` is its length.  Never this library's own
output.  The list is test_gpu_facets' (20 517 haystacks of 16 bytes, random 16-bit tags, bias +-300, a one-in-three subset).  Each test
first asserts, from the oracle's data, what it relies on: a section whose ties at the threshold exceed its quota, a keep-all section, an
empty section, and - where scores pass 255 - two sections whose thresholds have different high bytes."""
import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from facets_model import facet_words
from test_gpu_facets import Data, N
from test_gpu_multi_subset import hip_patterns
from test_gpu_parity import LANES
from test_gpu_scope import mapped, sub_list, visible
from test_gpu_score_bias import biased
from test_gpu_topk import SORTS, assert_top, single

pytestmark = pytest.mark.gpu
SECTIONS = [(1, 0), (2, 1), (0, 0), (0xF0, 0), (1, 1), (1, 0), (0xFFF, 0), (0, 0x8000)]
NEEDLES = ("deadbe", "g")
SCOPES = {"none": (0, 0), "part": (2, 1)}
LIMITS = (0, 1, 5, 100, 1024)
BY_SCORE = ("ScoreThenIndexAsc", "ScoreThenIndexDesc")
_WANT = {}


QUERY = ("query", "dead !x")  # query syntax: a `from_patterns` matcher


def oracle_of(query, sort):
    """the oracle's matcher: a needle (str) or ("query", text) for the parsed pattern list"""
    if isinstance(query, str):
        return O.Matcher(query, lanes=LANES[64], sort=sort)
    return O.MultiMatcher(O.parse_query(query[1]), lanes=(64, 64, 32), sort=sort)


def multi_of(sort):
    return F.MultiMatcher(hip_patterns(O.parse_query(QUERY[1])), F.Config(sort=F.SortStrategy[sort], pf_lanes=64))


def want_list(query, sort, scope, section, use_bias, use_subset=False):
    """the whole ordered list of one section: the oracle over the sub-list, mapped back; computed once per key, never modified"""
    key = (query, sort, scope, section, use_bias, use_subset)
    if key not in _WANT:
        d = Data.get()
        vis = visible(d["tags"], *scope) & visible(d["tags"], *section)
        if use_subset:
            inside = np.zeros(N, bool)
            inside[d["sub"]] = True
            vis &= inside
        sub = sub_list(d["hs"], vis)
        if not sub:
            w = np.zeros(0, F.MATCH_DTYPE)
        elif use_bias:
            w = biased(mapped(oracle_of(query, "IndexAsc").match_list(sub), vis), d["bias"], sort)
        else:
            w = mapped(oracle_of(query, sort).match_list(sub), vis)
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def limits_for(wants):
    """0, 1, 5, 100, 1024 and the limits around each section's size (within the call's bound)"""
    return sorted(set(LIMITS) | {k for w in wants for k in (len(w) - 1, len(w), len(w) + 1) if 0 <= k <= F.SECTION_LIMIT_MAX})


def relies_on(wants, limits, sort):
    """what the oracle's lists exercise over these limits: {"ties", "keep_all", "empty", "high_bytes"}"""
    facts = set()
    by_score = sort in BY_SCORE
    for limit in limits:
        highs = set()
        for w in wants:
            if len(w) == 0:
                facts.add("empty")
            elif len(w) <= limit:
                facts.add("keep_all")
            elif limit:
                t = int(w["score"][limit - 1]) if by_score else None
                ties = int((w["score"] == t).sum()) if by_score else len(w)
                quota = limit - int((w["score"] > t).sum()) if by_score else limit
                if ties > quota:
                    facts.add("ties")
                if by_score:
                    highs.add(t >> 8)
        if len(highs) > 1:
            facts.add("high_bytes")
    return facts


def corpus(scope=(0, 0), use_bias=False):
    d = Data.get()
    cp = F.Corpus(d["hs"])
    cp.set_tags(d["tags"])
    if use_bias:
        cp.set_bias(d["bias"])
    cp.set_scope(*scope)
    return cp


def assert_sections(got, wants, limit, ctx):
    assert len(got) == len(wants), (ctx, len(got))
    for s, (g, w) in enumerate(zip(got, wants)):
        assert_top(g, w, limit, (ctx, "section", s, SECTIONS[s] if len(wants) == len(SECTIONS) else None))


@pytest.mark.parametrize("scope", sorted(SCOPES))
@pytest.mark.parametrize("use_bias", (False, True), ids=("plain", "bias"))
@pytest.mark.parametrize("sort", SORTS)
def test_eight_sections_against_the_oracle(sort, use_bias, scope):
    cp = corpus(SCOPES[scope], use_bias)
    for needle in NEEDLES:
        wants = [want_list(needle, sort, SCOPES[scope], sec, use_bias) for sec in SECTIONS]
        limits = limits_for(wants)
        facts = relies_on(wants, limits, sort)
        assert {"ties", "keep_all", "empty"} <= facts, (needle, facts, [len(w) for w in wants])
        if scope == "none":
            assert wants[0].tolist() == wants[5].tolist() and len(wants[0]) > 1024  # the duplicate section
            sizes = {"deadbe": [1306, 655, 2605, 147, 0, 1306, 0, 1333], "g": [6349, 3114, 12573, 798, 0, 6349, 2, 6359]}[needle]
            assert [len(w) for w in wants] == sizes
        fm, _ = single(needle, sort=sort)
        for limit in limits:
            assert_sections(fm.match_list_top_sections(cp, SECTIONS, limit), wants, limit, (needle, sort, use_bias, scope, limit))


@pytest.mark.parametrize("sort", BY_SCORE)
def test_sections_cut_in_different_high_bins_of_one_call(sort):
    """with the bias scores reach 396: at limit 100 section (0xF0, 0) cuts at T = 0 while the others cut above 255, and at limit 1024
    section (1, 0) cuts inside the ties clamped to zero"""
    wants = [want_list("deadbe", sort, (0, 0), sec, True) for sec in SECTIONS]
    assert int(wants[2]["score"].max()) > 255
    assert int(wants[3]["score"][99]) == 0 and int(wants[0]["score"][99]) > 255 and "high_bytes" in relies_on(wants, (100,), sort)
    assert int(wants[0]["score"][1023]) == 0 and int((wants[0]["score"] == 0).sum()) > 1024 - int((wants[0]["score"] > 0).sum()) > 0
    cp = corpus((0, 0), True)
    fm, _ = single("deadbe", sort=sort)
    for limit in (99, 100, 101, 1023, 1024):
        assert_sections(fm.match_list_top_sections(cp, SECTIONS, limit), wants, limit, (sort, limit))


def test_everything_is_match_list_top_record_for_record():
    for use_bias in (False, True):
        cp = corpus((2, 1), use_bias)
        for sort in SORTS:
            fm, _ = single("g", sort=sort)
            want = want_list("g", sort, (2, 1), (0, 0), use_bias)
            assert len(want) > 1024
            for limit in (0, 1, 20, 1024):
                (recs, found), = fm.match_list_top_sections(cp, [(0, 0)], limit)
                assert_top((recs, found), want, limit, (sort, use_bias))
                plain, plain_found = fm.match_list_top(cp, limit)
                assert recs.tolist() == plain.tolist() and found == plain_found
    assert single("g")[0].match_list_top_sections(cp, [], 5) == []


@pytest.mark.parametrize("use_bias", (False, True), ids=("plain", "bias"))
def test_subset_and_capture(use_bias):
    d = Data.get()
    scope = (2, 1)
    cp = corpus(scope, use_bias)
    sub, cap, cap_plain = F.Subset(cp), F.Subset(cp), F.Subset(cp)
    sub.set_indices(d["sub"])
    for needle in NEEDLES:
        a = np.intersect1d(Data.matches(needle), d["sub"]).astype(np.uint32)  # the capture: the match set inside the subset, ahead of the scope
        assert 10 < len(a) < len(Data.matches(needle))
        for sort in ("ScoreThenIndexDesc", "IndexAsc"):
            wants = [want_list(needle, sort, scope, sec, use_bias, True) for sec in SECTIONS]
            assert {"ties", "keep_all", "empty"} <= relies_on(wants, (5, 100, 1024), sort)
            fm, _ = single(needle, sort=sort)
            for limit in (5, 100, 1024):
                assert_sections(fm.match_list_top_sections(cp, SECTIONS, limit, subset=sub, capture=cap), wants, limit, (needle, sort, limit))
                fm.match_list_top(cp, limit, subset=sub, capture=cap_plain)
                assert np.array_equal(cap.read(), cap_plain.read()) and np.array_equal(cap.read(), a)
            assert_sections(fm.match_list_top_sections(cp, SECTIONS, 100, subset=sub), wants, 100, (needle, sort, "no capture"))
            got = fm.match_list_top_sections(cp, SECTIONS, 100, capture=cap)  # the whole list, captured
            assert_sections(got, [want_list(needle, sort, scope, sec, use_bias) for sec in SECTIONS], 100, (needle, sort, "capture alone"))
            assert np.array_equal(cap.read(), Data.matches(needle).astype(np.uint32))


def test_an_attached_facet_sink_counts_what_the_plain_call_counts():
    d = Data.get()
    for scope in SCOPES.values():
        cp = corpus(scope, True)
        sink = F.Facets(cp)
        for needle in NEEDLES:
            a = Data.matches(needle)
            want_words = facet_words(d["tags"][a], *scope)
            assert want_words[0] > want_words[1] > 0 or scope == (0, 0)
            fm, _ = single(needle)
            fm.set_facets(sink)
            fm.match_list_top(cp, 250)
            plain = sink.read_words().tolist()
            assert plain == want_words.tolist()
            wants = [want_list(needle, "ScoreThenIndexAsc", scope, sec, True) for sec in SECTIONS]
            assert {"keep_all", "empty"} <= relies_on(wants, (250,), "ScoreThenIndexAsc")
            assert_sections(fm.match_list_top_sections(cp, SECTIONS, 250), wants, 250, (needle, scope))
            assert sink.read_words().tolist() == plain


@pytest.mark.parametrize("use_bias", (False, True), ids=("plain", "bias"))
def test_query_syntax(use_bias):
    d = Data.get()
    for scope in SCOPES.values():
        cp = corpus(scope, use_bias)
        sub = F.Subset(cp)
        sub.set_indices(d["sub"])
        for sort in SORTS:
            wants = [want_list(QUERY, sort, scope, sec, use_bias) for sec in SECTIONS]
            limits = limits_for(wants)
            assert {"ties", "keep_all", "empty"} <= relies_on(wants, limits, sort), [len(w) for w in wants]
            fm = multi_of(sort)
            for limit in limits:
                assert_sections(fm.match_list_top_sections(cp, SECTIONS, limit), wants, limit, ("dead !x", sort, scope, limit))
            wants = [want_list(QUERY, sort, scope, sec, use_bias, True) for sec in SECTIONS]
            cap, cap_plain = F.Subset(cp), F.Subset(cp)
            assert_sections(fm.match_list_top_sections(cp, SECTIONS, 100, subset=sub, capture=cap), wants, 100, ("dead !x", sort, scope, "subset"))
            fm.match_list_top(cp, 100, subset=sub, capture=cap_plain)
            assert len(cap.read()) > 10 and np.array_equal(cap.read(), cap_plain.read())


@pytest.mark.parametrize("use_bias", (False, True), ids=("plain", "bias"))
def test_the_empty_needle(use_bias):
    """the empty prompt: every visible haystack of the section, score = the clamped bias, sorted only over a biased corpus"""
    d = Data.get()
    for scope in SCOPES.values():
        cp = corpus(scope, use_bias)
        sub = F.Subset(cp)
        sub.set_indices(d["sub"])
        for sort in SORTS:
            fm, _ = single("", sort=sort)
            for use_subset in (False, True):
                wants = [want_list("", sort, scope, sec, use_bias, use_subset) for sec in SECTIONS]
                assert {"ties", "empty"} <= relies_on(wants, (1, 100, 1024), sort) and any(0 < len(w) <= 1024 for w in wants)
                for limit in (0, 1, 100, 1024):
                    got = fm.match_list_top_sections(cp, SECTIONS, limit, subset=sub if use_subset else None)
                    assert_sections(got, wants, limit, ("empty needle", sort, scope, use_subset, limit))
    for needle in ("", "g"):  # an empty corpus: S empty heads
        got = single(needle)[0].match_list_top_sections(F.Corpus([]), SECTIONS[:3], 5)
        assert [(len(r), f) for r, f in got] == [(0, 0)] * 3


def device_sections(fm, cp, sections, limit, extra=5, **kw):
    """the _device form -> (the whole buffer as records, guard included; the 2S count words; the words behind them)"""
    import torch

    S = len(sections)
    out = torch.full(((S * limit + extra) * 8,), 0xEE, dtype=torch.uint8, device="cuda")
    cnt = torch.full((2 * S + 4,), -7, dtype=torch.int32, device="cuda")
    fm.match_list_top_sections_device(cp, sections, limit, out.data_ptr(), S * limit, cnt.data_ptr(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("sort", ("ScoreThenIndexDesc", "IndexDesc"))
def test_the_device_form(sort):
    import torch

    d = Data.get()
    cp = corpus((0, 0), True)
    fm, _ = single("deadbe", sort=sort)
    for matcher, query in ((fm, "deadbe"), (multi_of(sort), QUERY)):
        wants = [want_list(query, sort, (0, 0), sec, True) for sec in SECTIONS]
        assert {"ties", "keep_all", "empty"} <= relies_on(wants, (0, 7, 200), sort)
        for limit in (0, 7, 200):
            raw, cnt = device_sections(matcher, cp, SECTIONS, limit)
            assert (raw[len(SECTIONS) * limit * 8:] == 0xEE).all(), "wrote beyond n_sections * limit records"
            assert (cnt[2 * len(SECTIONS):] == -7).all(), "wrote beyond the 2S count words"
            recs = raw[: len(SECTIONS) * limit * 8].view(F.MATCH_DTYPE)
            for s, w in enumerate(wants):
                kept, found = int(cnt[2 * s]), int(cnt[2 * s + 1])
                assert kept == min(limit, len(w)) and found == len(w), (s, kept, found, len(w))
                assert_top((recs[s * limit:s * limit + kept], found), w, limit, (sort, "device", s))  # (what lies behind kept_s in the slab is not read)
    # a capacity below n_sections * limit is refused, on a stream of the caller's the call is ordered
    out = torch.zeros(8 * 64, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(16, dtype=torch.int32, device="cuda")
    with pytest.raises(F.FrizbeeError):
        fm.match_list_top_sections_device(cp, SECTIONS, 8, out.data_ptr(), 63, cnt.data_ptr())
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        fm.match_list_top_sections_device(cp, SECTIONS, 8, out.data_ptr(), 64, cnt.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    wants = [want_list("deadbe", sort, (0, 0), sec, True) for sec in SECTIONS]
    recs = out.cpu().numpy().view(F.MATCH_DTYPE)
    for s, w in enumerate(wants):
        assert cnt[2 * s].item() == min(8, len(w)) and cnt[2 * s + 1].item() == len(w)
        assert recs[s * 8:s * 8 + min(8, len(w))].tolist() == w[:8].tolist()


def test_a_corpus_without_tags():
    d = Data.get()
    cp = F.Corpus(d["hs"])
    fm, _ = single("deadbe")
    want = want_list("deadbe", "ScoreThenIndexAsc", (0, 0), (0, 0), False)
    got = fm.match_list_top_sections(cp, [(0, 0), (1, 0), (0, 1)], 10)
    assert_top(got[0], want, 10)
    assert_top(got[2], want, 10)
    assert got[1][1] == 0 and len(got[1][0]) == 0
