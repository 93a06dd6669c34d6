"""Tag facets (fzb_facets, facets.h): the per-tag match counts a sink attached to a matcher holds after a query.  Every expected value is the
ORACLE's match set (oracle_lib) plus numpy over the tags (tests/facets_model.py), never this library's own output; counts are integers and
must be identical.  The list is 20 * 1024 + 37 short haystacks, `deadbe` planted in about one in eight, random 16-bit tags.  Each test
first asserts that it is not vacuous: at least 10 members and 10 non-members of the oracle's match set under every one of the 16 bits, and
a non-empty hidden and a non-empty visible part under the scopes used."""
import ctypes as C

import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from facets_model import WORDS, facet_words, visible
from test_gpu_parity import LANES
from test_gpu_small_device import device_of
from test_gpu_subset import device_top
from test_gpu_topk import SORTS, single

pytestmark = pytest.mark.gpu
N = 20 * 1024 + 37
NEEDLE = "deadbe"
SCOPES = {"none": (0, 0), "part": (2, 1), "all_hidden": (1, 1)}  # (require, exclude); a bit in both masks hides everything
ALPHABET = np.frombuffer(b"ghijklmnopqrstuv", np.uint8)


class Data:
    """the list, its tags and the oracle's match sets: built once, never modified (every test uploads its own Corpus)"""
    _d = None

    @classmethod
    def get(cls):
        if cls._d is None:
            rng = np.random.default_rng(2024)
            rows = rng.choice(ALPHABET, (N, 16))
            planted = rng.random(N) < 0.125
            rows[planted, 3:9] = np.frombuffer(b"deadbe", np.uint8)
            rows[rng.random(N) < 0.3, 12] = ord("x")  # what the query's negated pattern removes
            hs = [bytes(r) for r in rows]
            tags = rng.integers(0, 65536, N).astype(np.uint16)
            bias = rng.integers(-300, 301, N).astype(np.int16)
            sub = np.flatnonzero(rng.random(N) < 1 / 3).astype(np.uint32)
            cls._d = dict(hs=hs, tags=tags, bias=bias, sub=sub, a={})
        return cls._d

    @classmethod
    def matches(cls, needle, lanes=64):
        """the oracle's match set of one needle over the whole list: ascending haystack indices"""
        d = cls.get()
        if (needle, lanes) not in d["a"]:
            d["a"][(needle, lanes)] = np.sort(O.Matcher(needle, lanes=LANES[lanes], sort="IndexAsc").match_list(d["hs"])["index"].astype(np.int64))
        return d["a"][(needle, lanes)]


def not_vacuous(a, tags, n, scopes=SCOPES.values()):
    """the condition every test states first: under every bit the match set has members and non-members, and the scopes split it"""
    t = np.asarray(tags, np.uint32)[a]
    for b in range(16):
        has = int(((t >> b) & 1).sum())
        assert has >= 10 and len(a) - has >= 10, (b, has, len(a))
    for require, exclude in scopes:
        vis = visible(t, require, exclude)
        if require & exclude:
            assert not vis.any()
        elif require | exclude:
            assert vis.any() and not vis.all(), (require, exclude)
    assert 10 <= len(a) <= n - 10


def check(sink, want, ctx, found=None):
    got = sink.read_words()
    assert got.tolist() == np.asarray(want).tolist(), (ctx, got.tolist(), np.asarray(want).tolist())
    if found is not None:
        assert int(got[1]) == found, (ctx, "visible != found", int(got[1]), found)
    r = sink.read()
    assert r["matched"] == int(want[0]) and r["visible"] == int(want[1]) and r["all_by_bit"].tolist() == want[2:18].tolist() and r["visible_by_bit"].tolist() == want[18:34].tolist()
    assert isinstance(r["all_by_bit"], np.ndarray) and len(r["all_by_bit"]) == 16 and len(r["visible_by_bit"]) == 16


def device_call(call, capacity):
    """a _device form with room for `capacity` records: (records written as an array, the two count words)"""
    import torch

    out = torch.full(((capacity + 8) * 8,), 0xEE, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    call(out.data_ptr(), capacity, cnt.data_ptr())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[capacity * 8:] == 0xEE).all(), "wrote beyond the capacity"
    words = cnt.tolist()[:2]
    return host[: words[0] * 8].view(F.MATCH_DTYPE), words


def device_list(fm, cp, capacity, **kw):
    return device_call(lambda out, cap, cnt: fm.match_list_device(cp, out, cap, cnt, **kw), capacity)[1]


@pytest.mark.parametrize("use_subset", (False, True), ids=("range", "subset"))
@pytest.mark.parametrize("scope", sorted(SCOPES))
def test_the_matrix(scope, use_subset):
    d = Data.get()
    hs, tags, sub = d["hs"], d["tags"], d["sub"]
    a_all = Data.matches(NEEDLE)
    not_vacuous(a_all, tags, N)
    a = np.intersect1d(a_all, sub) if use_subset else a_all
    not_vacuous(a, tags, len(sub) if use_subset else N)
    require, exclude = SCOPES[scope]
    want = facet_words(tags[a], require, exclude)
    found = int(want[1])
    cp = F.Corpus(hs)
    cp.set_tags(tags)
    cp.set_scope(require, exclude)
    sink = F.Facets(cp)
    s, cap = F.Subset(cp), F.Subset(cp)
    s.set_indices(sub)
    kw = dict(subset=s) if use_subset else {}
    for sort in SORTS:
        fm, _ = single(NEEDLE, sort=sort)
        fm.set_facets(sink)
        got = fm.match_list(cp, **kw)
        check(sink, want, (scope, sort, "match_list"), found=len(got))
        for limit in (1, found + 5):
            recs, nfound = fm.match_list_top(cp, limit, **kw)
            check(sink, want, (scope, sort, "top", limit), found=nfound)
            assert len(recs) == min(limit, found)
        # with capture=: matched is the captured count and the captured indices' tags reproduce all_by_bit
        recs, nfound = fm.match_list_top(cp, 3, capture=cap, **kw)
        check(sink, want, (scope, sort, "capture"), found=nfound)
        captured = cap.read()
        assert len(captured) == int(want[0]) and np.array_equal(captured, a.astype(np.uint32))
        assert facet_words(tags[captured], require, exclude).tolist() == sink.read_words().tolist()
        # positions: the count sits at the top stage
        recs, nfound = fm.match_list_top_indices(cp, 7, **kw)
        check(sink, want, (scope, sort, "top_indices"), found=nfound)
    fm, _ = single(NEEDLE)
    fm.set_facets(sink)
    # the _device forms: a head left in HBM; a list whose output has room for 10 records still counts every match
    _, words = device_top(fm, cp, 100, subset=s if use_subset else None)
    check(sink, want, (scope, "top_device"), found=words[1])
    if not use_subset:
        written, nfound = device_list(fm, cp, 10)
        assert written == min(10, found)
        check(sink, want, (scope, "device, capacity 10"), found=nfound)
        # a sub-range, numbered from an offset of its own
        first, count = 1500, 3000
        ar = a_all[(a_all >= first) & (a_all < first + count)]
        wr = facet_words(tags[ar], require, exclude)
        assert 10 < len(ar) < count
        for capacity in (count, 10):
            written, nfound = device_list(fm, cp, capacity, first=first, count=count, index_offset=7)
            assert written == min(capacity, int(wr[1]))
            check(sink, wr, (scope, "sub-range", capacity), found=nfound)
        got = fm.match_list_into(cp, first=first, count=count, index_offset=7)
        check(sink, wr, (scope, "match_list_into"), found=len(got))
        # the ordered _device form: with room for every match its records are the host form's, which the oracle's order holds with the scope off;
        # with room for 10 the producer goes through the scratch, the order plan takes what the drop wrote, and the counts stay exact
        for sort in SORTS:
            fs, om = single(NEEDLE, sort=sort)
            fs.set_facets(sink)
            recs, (written, nfound) = device_call(lambda out, cap, cnt: fs.match_list_sorted_device(cp, out, cap, cnt), N)
            assert written == found
            check(sink, want, (scope, sort, "sorted_device"), found=nfound)
            if scope == "none":
                assert recs.tolist() == om.match_list(hs).tolist(), (sort, "sorted_device against the oracle")
            recs, (written, nfound) = device_call(lambda out, cap, cnt: fs.match_list_sorted_device(cp, out, cap, cnt), 10)
            assert written == min(10, found) and set(recs["index"].tolist()) <= set(a_all.tolist())
            if sort.startswith("Score"):
                assert (np.diff(recs["score"].astype(np.int64)) <= 0).all(), (sort, recs)
            check(sink, want, (scope, sort, "sorted_device, capacity 10"), found=nfound)
    # a bias changes scores, never the counts
    cp.set_bias(d["bias"])
    got = fm.match_list(cp, **kw)
    check(sink, want, (scope, "bias"), found=len(got))
    recs, nfound = fm.match_list_top(cp, 5, **kw)
    check(sink, want, (scope, "bias, top"), found=nfound)
    # the 32-lane pair
    a32 = Data.matches(NEEDLE, 32)
    a32 = np.intersect1d(a32, sub) if use_subset else a32
    fm32, _ = single(NEEDLE, pf=32)
    fm32.set_facets(sink)
    recs, nfound = fm32.match_list_top(cp, 5, **kw)
    check(sink, facet_words(tags[a32], require, exclude), (scope, "32 lanes"), found=nfound)


def test_a_needle_with_no_match_leaves_every_word_zero():
    d = Data.get()
    cp = F.Corpus(d["hs"])
    cp.set_tags(d["tags"])
    sink = F.Facets(cp)
    assert len(O.Matcher("zzzzzq", lanes=LANES[64]).match_list(d["hs"])) == 0
    for scope in SCOPES.values():
        cp.set_scope(*scope)
        fm, _ = single(NEEDLE)
        fm.set_facets(sink)
        fm.match_list(cp)
        assert sink.read_words()[0] == len(Data.matches(NEEDLE))  # (the sink holds counts that the next query has to replace)
        fm.set_pattern("zzzzzq")
        assert len(fm.match_list(cp)) == 0
        check(sink, np.zeros(WORDS, np.uint32), ("no match", scope), found=0)
        assert fm.match_list_top(cp, 5)[1] == 0
        check(sink, np.zeros(WORDS, np.uint32), ("no match, top", scope), found=0)


@pytest.mark.parametrize("n", (37, 1024, 1025))
def test_lists_of_a_wave_a_tile_and_a_tile_and_one(n):
    d = Data.get()
    base = [h[:3] + b"ghijkl" + h[9:] for h in d["hs"][:n]]  # (nothing planted is left)
    hs = [h[:3] + b"deadbe" + h[9:] if k % 3 != 2 else h for k, h in enumerate(base)]  # two thirds match
    a = np.sort(O.Matcher(NEEDLE, lanes=LANES[64], sort="IndexAsc").match_list(hs)["index"].astype(np.int64))
    # tags by construction, so that even 25 matches split at least 10 : 10 under every bit: bit b of the k-th match alternates in runs of 1, 2 or 3
    tags = d["tags"][:n].copy()
    k = np.arange(len(a))
    tags[a] = sum((((k // (1 + b % 3)) % 2) << b) for b in range(16)).astype(np.uint16)
    not_vacuous(a, tags, n, [(2, 1)])
    cp = F.Corpus(hs)
    cp.set_tags(tags)
    sink = F.Facets(cp)
    fm, _ = single(NEEDLE)
    fm.set_facets(sink)
    for require, exclude in SCOPES.values():
        cp.set_scope(require, exclude)
        want = facet_words(tags[a], require, exclude)
        got = fm.match_list(cp)
        check(sink, want, (n, require, exclude), found=len(got))
        recs, nfound = fm.match_list_top(cp, 4)
        check(sink, want, (n, require, exclude, "top"), found=nfound)
        written, nfound = device_list(fm, cp, 3)
        check(sink, want, (n, require, exclude, "device"), found=nfound)


def composed(query):
    d = Data.get()
    return np.sort(O.MultiMatcher(O.parse_query(query), lanes=LANES[64], sort="IndexAsc").match_list(d["hs"])["index"].astype(np.int64))


@pytest.mark.parametrize("query", ("dead be !x", "deadbe"))
def test_query_syntax(query):
    d = Data.get()
    hs, tags = d["hs"], d["tags"]
    a = composed(query)
    not_vacuous(a, tags, N)
    if query != NEEDLE:
        assert len(a) < len(Data.matches(NEEDLE))  # the negated pattern removed some
    cp = F.Corpus(hs)
    cp.set_tags(tags)
    sink = F.Facets(cp)
    mm = F.MultiMatcher(F.parse_query(query), F.Config(pf_lanes=64, sw_lanes=0))
    mm.set_facets(sink)
    cap = F.Subset(cp)
    for require, exclude in SCOPES.values():
        cp.set_scope(require, exclude)
        want = facet_words(tags[a], require, exclude)
        got = mm.match_list(cp)
        check(sink, want, (query, require, exclude), found=len(got))
        for limit in (1, int(want[1]) + 5):
            recs, nfound = mm.match_list_top(cp, limit)
            check(sink, want, (query, "top", limit), found=nfound)
        recs, nfound = mm.match_list_top(cp, 3, capture=cap)
        check(sink, want, (query, "capture"), found=nfound)
        assert np.array_equal(cap.read(), a.astype(np.uint32))
        recs, nfound = mm.match_list_top_indices(cp, 9)  # the fused form with positions
        check(sink, want, (query, "fused"), found=nfound)
        # the head left in HBM, over the range and over a candidate set, with a capture
        recs, words = device_call(lambda out, cap_, cnt: mm.match_list_top_device(cp, 10, out, cap_, cnt), 10)
        check(sink, want, (query, "top_device"), found=words[1])
        assert words[0] == min(10, int(want[1]))
        s = F.Subset(cp)
        s.set_indices(d["sub"])
        a_sub = np.intersect1d(a, d["sub"])
        not_vacuous(a_sub, tags, len(d["sub"]))
        recs, words = device_call(lambda out, cap_, cnt: mm.match_list_top_device(cp, 10, out, cap_, cnt, subset=s, capture=cap), 10)
        check(sink, facet_words(tags[a_sub], require, exclude), (query, "top_subset_device"), found=words[1])
        assert np.array_equal(cap.read(), a_sub.astype(np.uint32))
        import torch
        out = torch.zeros(16 * 8, dtype=torch.uint8, device="cuda")
        cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        mm.match_list_device(cp, out.data_ptr(), 10, cnt.data_ptr())  # room for 10 records
        torch.cuda.synchronize()
        check(sink, want, (query, "device, capacity 10"), found=cnt.tolist()[1])
    # the sink survives set_patterns
    mm.set_patterns(F.parse_query("dead"))
    cp.set_scope(2, 1)
    recs, nfound = mm.match_list_top(cp, 3)
    check(sink, facet_words(tags[composed("dead")], 2, 1), "set_patterns", found=nfound)


def test_the_empty_prompt():
    d = Data.get()
    hs, tags = d["hs"], d["tags"]
    every = np.arange(N)
    not_vacuous(Data.matches(NEEDLE), tags, N)
    cp = F.Corpus(hs)
    sink = F.Facets(cp)
    fm = F.Matcher("", F.Config(pf_lanes=64, sw_lanes=64))
    fm.set_facets(sink)
    mm = F.MultiMatcher([], F.Config(pf_lanes=64, sw_lanes=0))
    mm.set_facets(sink)
    # no tags, no term: the closed-form host answers
    want = facet_words(np.zeros(N, np.uint16))
    assert len(fm.match_list(cp)) == N
    check(sink, want, "empty, no tags", found=N)
    cp.set_tags(tags)
    for require, exclude in SCOPES.values():
        cp.set_scope(require, exclude)
        want = facet_words(tags[every], require, exclude)
        for who, m in (("single", fm), ("multi", mm)):
            got = m.match_list(cp)
            check(sink, want, ("empty", who, require, exclude), found=len(got))
            recs, nfound = m.match_list_top(cp, 5)
            check(sink, want, ("empty top", who, require, exclude), found=nfound)
            recs, nfound = m.match_list_top_indices(cp, 5)
            check(sink, want, ("empty top_indices", who, require, exclude), found=nfound)
        import torch
        out = torch.zeros(16 * 8, dtype=torch.uint8, device="cuda")
        cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        fm.prompt_top_device(cp, 10, out.data_ptr(), 10, cnt.data_ptr())
        torch.cuda.synchronize()
        check(sink, want, ("prompt_top_device", require, exclude), found=cnt.tolist()[1])
        fm.prompt_list_device(cp, out.data_ptr(), 10, cnt.data_ptr(), first=1500, count=3000, index_offset=7)
        torch.cuda.synchronize()
        check(sink, facet_words(tags[1500:4500], require, exclude), ("prompt_list_device", require, exclude), found=cnt.tolist()[1])
    # over Subset.from_scope: the set is what another scope shows; the corpus' own scope still applies
    cp.set_scope(2, 1)
    s = F.Subset(cp)
    s.from_scope(4, 8)
    members = np.flatnonzero(visible(tags, 4, 8))
    want = facet_words(tags[members], 2, 1)
    assert 0 < want[1] < want[0] < N
    for who, m in (("single", fm), ("multi", mm)):
        recs, nfound = m.match_list_top(cp, 5, subset=s)
        check(sink, want, ("from_scope", who), found=nfound)
    # over a subset whose count the host does not know: filled by a _device capture
    q, _ = single(NEEDLE)
    cap = F.Subset(cp)
    device_top(q, cp, 10, capture=cap)
    import torch
    out = torch.zeros(16 * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    fm.prompt_top_device(cp, 10, out.data_ptr(), 10, cnt.data_ptr(), subset=cap)  # (nothing asked the subset for its count in between)
    torch.cuda.synchronize()
    check(sink, facet_words(tags[Data.matches(NEEDLE)], 2, 1), "device capture as input", found=cnt.tolist()[1])


def test_edits_the_counts_follow_the_compacted_column():
    d = Data.get()
    rng = np.random.default_rng(7)
    hs, tags = list(d["hs"]), d["tags"].copy()
    cp = F.Corpus(hs)
    cp.set_tags(tags)
    cp.set_scope(2, 1)
    sink = F.Facets(cp)
    fm, om = single(NEEDLE, sort="IndexAsc")
    fm.set_facets(sink)
    gone = np.sort(rng.choice(N, 3000, replace=False))
    cp.remove(gone)
    keep = np.ones(N, bool)
    keep[gone] = False
    hs = [h for h, k in zip(hs, keep) if k]
    tags = tags[keep]
    at = rng.choice(len(hs), 2000, replace=False)
    new = rng.integers(0, 65536, 2000).astype(np.uint16)
    cp.update_tags(at, new)
    tags[at] = new
    a = np.sort(om.match_list(hs)["index"].astype(np.int64))
    not_vacuous(a, tags, len(hs), [(2, 1)])
    want = facet_words(tags[a], 2, 1)
    got = fm.match_list(cp)
    check(sink, want, "after remove + update_tags", found=len(got))
    recs, nfound = fm.match_list_top(cp, 5)
    check(sink, want, "after remove + update_tags, top", found=nfound)


def test_corpora_without_tags():
    d = Data.get()
    a = Data.matches(NEEDLE)
    not_vacuous(a, d["tags"], N)
    want = facet_words(np.zeros(len(a), np.uint16))  # matched and visible, both rows zero
    assert want[0] == want[1] == len(a) and not want[2:].any()
    fm, _ = single(NEEDLE)
    cp = F.Corpus(d["hs"])  # no tags at all
    sink = F.Facets(cp)
    fm.set_facets(sink)
    check(sink, np.zeros(WORDS, np.uint32), "a new sink")
    got = fm.match_list(cp)
    check(sink, want, "no tags", found=len(got))
    assert device_list(fm, cp, 10)[1] == len(a)
    check(sink, want, "no tags, device capacity 10", found=len(a))
    cp2 = F.Corpus(d["hs"])  # tags set, then cleared
    cp2.set_tags(d["tags"])
    cp2.clear_tags()
    sink2 = F.Facets(cp2)
    fm.set_facets(sink2)
    recs, nfound = fm.match_list_top(cp2, 5)
    check(sink2, want, "cleared tags", found=nfound)
    # a sink created on one corpus is refused on another
    with pytest.raises(F.FrizbeeError) as e:
        fm.match_list(cp)
    assert e.value.code == 1 and "facet sink" in str(e.value) and "another corpus" in str(e.value)
    with pytest.raises(F.FrizbeeError):
        fm.match_list_top(cp, 5)
    fm.set_facets(None)
    assert len(fm.match_list(cp)) == len(a)


def test_entry_points_that_cannot_fill_a_sink_refuse_it():
    d = Data.get()
    hs = d["hs"][:2048]
    cp = F.Corpus(hs)
    sc = F.ShardedCorpus(hs, ndev=1)
    sink = F.Facets(cp)
    fm, _ = single(NEEDLE)
    mm = F.MultiMatcher(F.parse_query("dead be"), F.Config(pf_lanes=64, sw_lanes=0))

    def composed_top_indices(m):  # the composed (not fused) form: only the C ABI has it
        out, n, pos, found = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_uint64()
        F._check(F.lib().fzb_multi_match_list_top_indices(m.h, cp.h, 5, C.byref(out), C.byref(n), C.byref(pos), C.byref(found)))
        F.lib().fzb_match_indices_free(out, pos)

    calls = [
        (fm, "match_list_parallel", lambda m: m.match_list_parallel(cp, 2)), (fm, "match_list_indices", lambda m: m.match_list_indices(cp)),
        (fm, "match_list_indices_into", lambda m: m._indices_into(cp, 3)), (fm, "match_list_parallel_sharded", lambda m: m.match_list_parallel_sharded(sc)),
        (fm, "match_list_top_sharded", lambda m: m.match_list_top_sharded(sc, 5)),
        (mm, "multi match_list_parallel", lambda m: m.match_list_parallel(cp, 2)), (mm, "multi match_list_indices", lambda m: m.match_list_indices(cp)),
        (mm, "multi match_list_indices_into", lambda m: m._indices_into(cp, 3)), (mm, "multi match_list_parallel_sharded", lambda m: m.match_list_parallel_sharded(sc)),
        (mm, "multi match_list_top_sharded", lambda m: m.match_list_top_sharded(sc, 5)), (mm, "multi composed top_indices", composed_top_indices),
    ]
    for m, name, call in calls:
        m.set_facets(sink)
        with pytest.raises(F.FrizbeeError) as e:
            call(m)
        assert e.value.code == 1 and "set_facets(NULL)" in str(e.value), (name, str(e.value))
        m.set_facets(None)
        call(m)  # succeeds once the sink is detached


def test_no_allocation_after_reserve_with_a_sink_attached():
    import torch

    d = Data.get()
    cp = F.Corpus(d["hs"])
    cp.set_tags(d["tags"])
    sink = F.Facets(cp)
    fm, _ = single(NEEDLE)
    fm.set_facets(sink)
    fm.reserve(cp)
    mm = F.MultiMatcher(F.parse_query("dead be !x"), F.Config(pf_lanes=64, sw_lanes=0))
    mm.set_facets(sink)
    mm.reserve(cp)
    out = torch.zeros(128 * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    fm.match_list(cp)  # (pooled pinned result buffers, not device memory, warm up here)
    before = F.device_allocs()
    for needle in ("dead", "deadb", NEEDLE):
        fm.set_pattern(needle)
        for scope in ((0, 0), (2, 1), (0, 0), (1, 1)):
            cp.set_scope(*scope)
            fm.match_list(cp)
            fm.match_list_top(cp, 100)
            fm.match_list_device(cp, out.data_ptr(), 10, cnt.data_ptr())
            fm.match_list_top_device(cp, 100, out.data_ptr(), 100, cnt.data_ptr())
            mm.match_list_top(cp, 100)
            mm.match_list_device(cp, out.data_ptr(), 10, cnt.data_ptr())
            torch.cuda.synchronize()
    assert F.device_allocs() == before, (before, F.device_allocs())
    check(sink, facet_words(d["tags"][composed("dead be !x")], 1, 1), "the last query's counts")


def test_detached_means_unchanged():
    """under FZB_DEBUG_CUS the launch record of a query by a matcher that never had a sink equals the record of the same query after attach
    and detach, and holds no facets kernel"""
    d = Data.get()
    with device_of(5):
        cp = F.Corpus(d["hs"])
        cp.set_tags(d["tags"])
        sink = F.Facets(cp)
        for scope in ((0, 0), (2, 1)):
            cp.set_scope(*scope)
            records = []
            for attach in (False, True):
                fm, _ = single(NEEDLE)
                if attach:
                    fm.set_facets(sink)
                    fm.match_list_top(cp, 100)
                    assert any("facets" in k for k in F.launch_grids())  # attached: a facets kernel ran
                    fm.set_facets(None)
                else:
                    fm.match_list_top(cp, 100)  # (the same warm-up: first-use launches)
                F.launch_grids()
                fm.match_list_top(cp, 100)
                fm.match_list(cp)
                records.append(F.launch_grids())
            assert records[0] == records[1], (scope, records)
            assert records[0] and not any("facets" in k for k in records[0]), records[0]


def test_a_device_form_on_a_stream_of_the_callers():
    """read() behind a _device form on the caller's own stream waits for the sink's event - nothing else synchronises in between - and the
    sink is freed without touching that stream"""
    import torch

    d = Data.get()
    a = Data.matches(NEEDLE)
    not_vacuous(a, d["tags"], N)
    cp = F.Corpus(d["hs"])
    cp.set_tags(d["tags"])
    cp.set_scope(2, 1)
    want = facet_words(d["tags"][a], 2, 1)
    fm, _ = single(NEEDLE)
    sink = F.Facets(cp)
    fm.set_facets(sink)
    fm.reserve(cp)
    stream = torch.cuda.Stream()
    out = torch.zeros(128 * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        fm.match_list_top_device(cp, 100, out.data_ptr(), 100, cnt.data_ptr(), stream=stream.cuda_stream)
        assert sink.read_words().tolist() == want.tolist()  # (no synchronisation of ours: the read waits)
    stream.synchronize()
    assert cnt.tolist()[1] == int(want[1])
    fm.match_list_top_device(cp, 100, out.data_ptr(), 100, cnt.data_ptr(), stream=stream.cuda_stream)
    fm.set_facets(None)
    del sink  # freed with a query in flight: waits for the event, not for the stream
    recs, found = fm.match_list_top(cp, 5)  # then a host form on the null stream, no sink
    assert found == int(want[1])
