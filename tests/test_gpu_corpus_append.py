"""A resident corpus that grows (fzb_corpus_append / _reserve / _truncate / _info): after any sequence of appends and truncates the corpus
answers every query exactly as a fresh upload of the same list - and as the oracle - and its device arrays, read back through
fzb_debug_corpus_read, are the fresh upload's byte for byte (canonical layout) or decode to the same list (the filter's view, whose order
of equal-length haystacks inside a tile is free: corpus_layout_model.check_view)."""
import math
import random

import numpy as np
import pytest

import corpus_layout_model as L
import frizbee_amd as F
import oracle_lib as O
from test_gpu_parity import LANES, assert_same
from test_gpu_topk import single

pytestmark = pytest.mark.gpu
SORTS = ("ScoreThenIndexAsc", "ScoreThenIndexDesc", "IndexAsc", "IndexDesc")
VIEW_ARRAYS = ("vbytes", "vgofs", "vgnv", "vlen", "vperm", "vlong")
INFO_KEYS = ("items", "bytes", "max_len", "uniform_len", "has_view", "view_nv", "outliers", "ends_u64")
WORDS = ["src", "linux", "kernel", "test", "drivers", "net", "include", "lib", "main", "util", "fs", "arch", "x86", "README", "Makefile", "foo_bar", "Linux", "TEST"]
LONG_NEEDLE = "drivers/net/ethernet/intel/ice/a_rather_long_file_name_that_goes_on_and_on.c"  # 76 bytes: beyond 64
assert len(LONG_NEEDLE) > 64


# ---- the lists ----------------------------------------------------------------------------------------------------------------------
def _path(rng, lo, hi):
    target = rng.randint(lo, hi)
    s = ""
    while len(s) < target:
        s += rng.choice(WORDS) + rng.choice("/_.-")
    return s[:target]


def make_list(kind, n, seed=1):
    rng = random.Random(seed * 7919 + len(kind))
    if kind == "uniform32":
        return [_path(rng, 32, 32) for _ in range(n)]
    if kind == "ragged":
        return [_path(rng, 8, 128) for _ in range(n)]
    if kind == "outliers":  # paths with a few haystacks of 300-2000 bytes, some of which hold the long needle
        hs = [_path(rng, 8, 128) for _ in range(n)]
        for i in rng.sample(range(n), max(3, n // 400)):
            hs[i] = _path(rng, 150, 900) + (LONG_NEEDLE if rng.random() < 0.5 else "") + _path(rng, 150, 1000)
        return hs
    if kind == "utf8":
        alphabet = list("abéÉñ人_ -/linuxüß")
        hs = []
        for _ in range(n):
            s, target = "", rng.randint(1, 90)
            while len((s + "人").encode()) <= target:
                s += rng.choice(alphabet)
            hs.append(s)
        return hs
    if kind == "short":  # nothing beyond 32 bytes
        return [_path(rng, 1, 32) for _ in range(n)]
    if kind == "empties":
        return ["" if rng.random() < 0.2 else _path(rng, 1, 100) for _ in range(n)]
    raise KeyError(kind)


KINDS = ("uniform32", "ragged", "outliers", "utf8", "short", "empties")


def splits(n, size):
    out, at = [], 0
    while at < n:
        out.append((at, min(n, at + size)))
        at += size
    return out


def random_splits(n, seed):
    rng = random.Random(seed)
    cuts = sorted(set(rng.sample(range(1, n), min(n - 1, rng.randint(3, 12)))))
    edges = [0] + cuts + [n]
    return list(zip(edges[:-1], edges[1:]))


# ---- what is compared -----------------------------------------------------------------------------------------------------------------
def check_layout(cp, hs, fresh=None, view=True):
    """canonical bytes + tail + offsets == the numpy model's (and the fresh upload's); the view decodes to the list; info() as the fresh one's"""
    data, ends = L.canonical(hs)
    got_b, got_e = cp.debug_read("bytes"), cp.debug_read("ends")
    assert len(cp) == len(hs)
    assert got_e.tolist() == ends.tolist()
    assert len(got_b) == len(data) and np.array_equal(got_b, data), "canonical bytes differ from the model"
    info = cp.info()
    assert info["items"] == len(hs) and info["bytes"] == len(data) - 96 and info["item_capacity"] >= len(hs) and info["byte_capacity"] >= info["bytes"]
    assert bool(info["has_view"]) == L.wants_view(hs), (info, len(hs))
    if fresh is not None:
        assert np.array_equal(fresh.debug_read("bytes"), got_b) and np.array_equal(fresh.debug_read("ends"), got_e)
        fi = fresh.info()
        assert {k: info[k] for k in INFO_KEYS} == {k: fi[k] for k in INFO_KEYS}
    if view and info["has_view"]:
        L.check_view(hs, {k: cp.debug_read(k) for k in VIEW_ARRAYS})
        lens = [len(h.encode() if isinstance(h, str) else h) for h in hs]
        assert info["outliers"] == sum(x > 256 for x in lens) and info["view_nv"] == (max(x for x in lens if x <= 256) + 15) // 16
    return info


class Expected:
    """the oracle's answers for one list, computed once per query"""

    def __init__(self, hs):
        self.hs, self.cache = hs, {}

    def single(self, needle, sort="ScoreThenIndexAsc", **kw):
        key = (needle, sort, tuple(sorted(kw.items())))
        if key not in self.cache:
            fm, om = single(needle, sort=sort, **kw)
            self.cache[key] = (fm, om, om.match_list(self.hs))
        return self.cache[key]


def check_parity(cp, fresh, exp, needles, boundary=None, full=True):
    """every query form over the grown corpus == over the fresh upload == the oracle"""
    hs, n, matches = exp.hs, len(exp.hs), 0
    queries = []
    for needle, kw in needles:
        queries += [(needle, s, kw) for s in (SORTS if full else SORTS[:1])]
    if full:
        queries += [(needles[0][0], "ScoreThenIndexAsc", dict(max_typos=t)) for t in (1, 2, None)]
    for needle, sort, kw in queries:
        fm, om, want = exp.single(needle, sort, **kw)
        ctx = f"{needle!r} {sort} {kw} n={n}"
        got = fm.match_list(cp)
        assert_same(got, want, "grown vs oracle " + ctx)
        assert_same(fm.match_list(fresh), want, "fresh vs oracle " + ctx)
        matches += len(want)
        recs, found = fm.match_list_top(cp, 100)
        assert found == len(want) and recs.tolist() == want[:100].tolist(), "top " + ctx
        if sort == "ScoreThenIndexAsc" and len(want):
            sel = want["index"][:100].astype(np.uint32)
            ix = fm.match_list_indices(cp, sel)
            assert ix == fm.match_list_indices(fresh, sel), "indices " + ctx
            assert [(g.index, g.score, g.exact, g.indices) for g in ix] == om.match_list_indices_ordered([hs[int(i)] for i in sel]), "indices vs oracle " + ctx
        if sort == "IndexAsc" and n > 4:  # a sub-range that straddles an append boundary, numbered from an offset
            b = boundary if boundary and 2 <= boundary < n - 1 else n // 2
            first, count = max(0, b - min(b, 700)), min(n, b + 700) - max(0, b - min(b, 700))
            sub = om.match_list(hs[first:first + count])
            got = fm.match_list_into(cp, first, count, 1000)
            assert got.tolist() == fm.match_list_into(fresh, first, count, 1000).tolist(), "into " + ctx
            assert (got["index"] - 1000).tolist() == sub["index"].tolist() and got["score"].tolist() == sub["score"].tolist(), "into vs oracle " + ctx
    if full:
        q = "src linux !test"
        for sort in ("ScoreThenIndexAsc", "IndexDesc"):
            want = O.MultiMatcher(O.parse_query(q), lanes=LANES[64], sort=sort).match_list(hs)
            mm = F.MultiMatcher(F.parse_query(q), F.Config(sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=0))
            assert_same(mm.match_list(cp), want, f"multi grown {sort}")
            assert_same(mm.match_list(fresh), want, f"multi fresh {sort}")
            recs, found = mm.match_list_top(cp, 100)
            assert found == len(want) and recs.tolist() == want[:100].tolist()
            matches += len(want)
    return matches


def needles_for(kind):
    base = [("linux", {}), ("linux", dict(matching="Substring")), (LONG_NEEDLE, {})]
    if kind == "utf8":
        base = [("linux", {}), ("é人", {}), ("linux", dict(matching="Substring"))]
    return base


def grow(hs, pieces, start=None, each=None):
    cp = start if start is not None else F.Corpus([])
    for lo, hi in pieces:
        cp.append(hs[lo:hi])
        if each:
            each(cp, hi)
    return cp


# ---- parity and layout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_appended_corpus_answers_and_lies_like_a_fresh_upload(kind):
    n = 6200
    hs = make_list(kind, n)
    exp, fresh = Expected(hs), F.Corpus(hs)
    total = 0
    for label, pieces in [("63", splits(n, 63)), ("1024", splits(n, 1024)), ("1025", splits(n, 1025)), ("5000", splits(n, 5000)), ("random", random_splits(n, 11)),
                          ("random2", random_splits(n, 12))]:
        step = [0]

        def each(cp, hi):
            step[0] += 1
            check_layout(cp, hs[:hi], F.Corpus(hs[:hi]), view=(step[0] % 8 == 0 or hi == n))

        cp = grow(hs, pieces, each=each)
        check_layout(cp, hs, fresh)
        total += check_parity(cp, fresh, exp, needles_for(kind), boundary=pieces[len(pieces) // 2][0], full=label in ("63", "random"))
    assert total > 100, "the lists hold matches"
    # an uploaded, non-empty corpus grows the same way (the first append finds no room: one regrow)
    cp = F.Corpus(hs[:777])
    cp.append(hs[777:])
    assert cp.info()["regrows"] == 1
    check_layout(cp, hs, fresh)
    check_parity(cp, fresh, exp, needles_for(kind)[:1], boundary=777, full=False)


@pytest.mark.parametrize("kind", KINDS)
def test_one_haystack_at_a_time_across_a_tile_boundary(kind):
    hs = make_list(kind, 1100, seed=3)
    exp = Expected(hs)

    def each(cp, hi):
        check_layout(cp, hs[:hi], view=(hi % 64 == 1 or hi in (1023, 1024, 1025, 1100)))

    cp = grow(hs, splits(1100, 1), each=each)
    fresh = F.Corpus(hs)
    check_layout(cp, hs, fresh)
    check_parity(cp, fresh, exp, needles_for(kind), boundary=1024, full=True)


def test_set_len_promises_follow_the_appended_list():
    cp = F.Corpus(["a" * 32] * 10)
    assert cp.info()["uniform_len"] == 32 and cp.info()["max_len"] == 32
    cp.append(["b" * 50])
    assert cp.info()["uniform_len"] == 0 and cp.info()["max_len"] == 50
    l = F.lib()
    assert l.fzb_corpus_set_uniform_len(cp.h, 0) == 0 and l.fzb_corpus_set_uniform_len(cp.h, 32) == 1
    assert l.fzb_corpus_set_max_len(cp.h, 50) == 0 and l.fzb_corpus_set_max_len(cp.h, 32) == 1


# ---- transitions ----------------------------------------------------------------------------------------------------------------------
def _transition(stages, needles=(("linux", {}),)):
    hs, cp, seen = [], F.Corpus([]), []
    for batch in stages:
        boundary = len(hs)
        hs = hs + batch
        cp.append(batch)
        fresh = F.Corpus(hs)
        info = check_layout(cp, hs, fresh)
        check_parity(cp, fresh, Expected(hs), list(needles), boundary=boundary, full=False)
        seen.append((info["uniform_len"], info["has_view"]))
    return seen


def test_uniform_list_turns_ragged():
    seen = _transition([make_list("uniform32", 2000), make_list("ragged", 900, seed=2), make_list("uniform32", 100, seed=3)])
    assert seen == [(32, 0), (0, 1), (0, 1)]


def test_view_arrives_with_the_first_haystack_beyond_32_bytes():
    seen = _transition([make_list("short", 3000), make_list("short", 500, seed=2), make_list("short", 10, seed=3) + ["src/linux/" + "x" * 30], make_list("ragged", 300)])
    assert [v for _, v in seen] == [0, 0, 1, 1]


def test_view_goes_with_too_many_outliers_and_comes_back():
    many = ["src/linux/" + "y" * (300 + i) for i in range(100)]  # 2100 haystacks tolerate 2100 // 256 + 64 = 72
    seen = _transition([make_list("ragged", 2000), many, make_list("ragged", 300, seed=4), make_list("ragged", 10000, seed=5)])  # 12400 // 256 + 64 = 112
    assert [v for _, v in seen] == [1, 0, 0, 1]


def test_batch_that_ends_on_a_tile_boundary():
    seen = _transition([make_list("ragged", 1024), make_list("outliers", 1024, seed=2), make_list("ragged", 500, seed=3)])
    assert [v for _, v in seen] == [1, 1, 1]


# ---- capacity -------------------------------------------------------------------------------------------------------------------------
def test_reserved_corpus_and_matchers_never_allocate():
    hs = make_list("outliers", 64 * 100)
    raw = sum(len(h) for h in hs)
    cp = F.Corpus([])
    cp.reserve(len(hs), raw + 15 * len(hs))
    cap = cp.info()
    assert cap["item_capacity"] >= len(hs) and cap["byte_capacity"] >= raw + 15 * len(hs) and cap["items"] == 0
    fm = F.Matcher("linux", F.Config(pf_lanes=64))
    fm.reserve(cp)
    mm = F.MultiMatcher(F.parse_query("src linux !test"), F.Config(pf_lanes=64))
    mm.reserve(cp)
    before = F.device_allocs()
    for b in range(64):
        cp.append(hs[b * 100:(b + 1) * 100])
        got = fm.match_list(cp)
        top, found = fm.match_list_top(cp, 100)
        multi = mm.match_list(cp)
        assert F.device_allocs() == before, f"batch {b}: a device allocation inside the reserved room"
        assert found == len(got) and top.tolist() == got[:100].tolist() and len(multi) <= len(got)
    info = cp.info()
    assert info["regrows"] == 0 and info["item_capacity"] == cap["item_capacity"] and info["byte_capacity"] == cap["byte_capacity"] and info["has_view"] == 1
    fresh = F.Corpus(hs)
    check_layout(cp, hs, fresh)
    check_parity(cp, fresh, Expected(hs), [("linux", {})], full=False)


def test_unreserved_corpus_regrows_geometrically_and_copies_each_haystack_once():
    hs = make_list("ragged", 64 * 150)
    cp = F.Corpus([])
    sent = 0
    for b in range(64):
        batch = hs[b * 150:(b + 1) * 150]
        cp.append(batch)
        sent += sum(len(h) for h in batch) + 8 * len(batch)
        assert cp.info()["h2d_bytes"] == sent
    assert 1 <= cp.info()["regrows"] <= math.ceil(math.log2(64)) + 1
    check_layout(cp, hs, F.Corpus(hs))


# ---- truncate -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["outliers", "uniform32", "empties"])
def test_truncate_then_append_again(kind):
    hs = make_list(kind, 4000, seed=6)
    cp = grow(hs, splits(4000, 1300))
    cap = cp.info()

    def same_as_fresh(cur, boundary):
        fresh = F.Corpus(cur)
        info = check_layout(cp, cur, fresh)
        assert info["item_capacity"] == cap["item_capacity"] and info["byte_capacity"] == cap["byte_capacity"], "capacity is kept"
        if cur:
            check_parity(cp, fresh, Expected(cur), [("linux", {})], boundary=boundary, full=False)

    cp.truncate(4000)  # the current length: nothing changes
    same_as_fresh(hs, 2600)
    cp.truncate(1500)  # mid-tile
    same_as_fresh(hs[:1500], 1300)
    cp.append(hs[3000:3600])
    same_as_fresh(hs[:1500] + hs[3000:3600], 1500)
    cp.truncate(1024)  # a tile boundary
    same_as_fresh(hs[:1024], 1000)
    cp.append(hs[2000:2100])
    same_as_fresh(hs[:1024] + hs[2000:2100], 1024)
    cp.truncate(0)
    same_as_fresh([], 0)
    assert cp.info()["max_len"] == 0 and cp.info()["uniform_len"] == 0 and cp.info()["has_view"] == 0
    cp.append(hs[500:3900])
    same_as_fresh(hs[500:3900], 1700)
    with pytest.raises(F.FrizbeeError, match="beyond the corpus"):
        cp.truncate(3401)


def test_truncate_changes_what_the_list_calls_for():
    uni, rag = make_list("uniform32", 1500), make_list("ragged", 700, seed=9)
    cp = F.Corpus(uni + rag)
    assert cp.info()["has_view"] == 1
    cp.truncate(1500)  # the kept prefix is uniform: no view, offsets computed
    check_layout(cp, uni, F.Corpus(uni))
    assert cp.info()["uniform_len"] == 32 and cp.info()["has_view"] == 0
    many = ["src/linux/" + "y" * (300 + i) for i in range(100)]
    cp = grow(rag + many + rag, [(0, 700), (700, 800), (800, 1500)])
    assert cp.info()["has_view"] == 0
    cp.truncate(760)  # 60 outliers left of the 100: a view again
    check_layout(cp, (rag + many)[:760], F.Corpus((rag + many)[:760]))
    assert cp.info()["has_view"] == 1 and cp.info()["outliers"] == 60


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_borrowed_corpus_is_refused():
    import torch
    data = torch.zeros(4 * 32 + 96, dtype=torch.uint8, device="cuda")
    ends = torch.tensor([32, 64, 96, 128], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cp = F.Corpus.from_device(data.data_ptr(), ends.data_ptr(), 4, 4 * 32 + 96, keep=(data, ends))
    for call in (lambda: cp.append(["abc"]), lambda: cp.reserve(10, 1000), lambda: cp.truncate(2)):
        with pytest.raises(F.FrizbeeError, match="borrows") as e:
            call()
        assert e.value.args[0] == 1 or "borrows" in str(e.value)
    assert len(cp) == 4 and cp.info()["items"] == 4


def test_decreasing_offsets_leave_the_corpus_as_it_was():
    hs = make_list("outliers", 3000, seed=8)
    cp = grow(hs, splits(3000, 700))
    fm = F.Matcher("linux", F.Config(pf_lanes=64))
    before, info = fm.match_list(cp), cp.info()
    arrays = {k: cp.debug_read(k) for k in ("bytes", "ends") + VIEW_ARRAYS}
    data, ends = F.pack(make_list("ragged", 2500, seed=9))
    ends = ends.copy()
    ends[1200] = ends[1199] - 3
    with pytest.raises(F.FrizbeeError, match="end_offsets must be non-decreasing"):
        cp.append(packed=(data, ends))
    assert cp.info() == info and len(cp) == 3000
    assert fm.match_list(cp).tolist() == before.tolist()
    for k, a in arrays.items():
        assert np.array_equal(cp.debug_read(k), a), k
    cp.append([])  # a valid no-op
    assert cp.info() == info
    cp.append(hs[:10])
    check_layout(cp, hs + hs[:10], F.Corpus(hs + hs[:10]))
