"""A resident corpus that is edited (fzb_corpus_remove / _remove_device / _replace / _edit_info): after any sequence of upload, append,
reserve, truncate, remove and replace the corpus answers every query exactly as a fresh upload of the edited list - and as the oracle -
and its device arrays, read back through fzb_debug_corpus_read, are the fresh upload's byte for byte (canonical layout) or decode to the
same list (the filter's view).  The lists, the layout checks and the parity checks are test_gpu_corpus_append.py's."""
import os
import random

import numpy as np
import pytest

import corpus_layout_model as L
import frizbee_amd as F
import oracle_lib as O
from test_gpu_topk import single
from test_gpu_corpus_append import KINDS, LONG_NEEDLE, VIEW_ARRAYS, Expected, check_layout, check_parity, make_list, needles_for

pytestmark = pytest.mark.gpu
TILE = L.TILE


def blen(h):
    return len(h.encode() if isinstance(h, str) else h)


def without(hs, drop):
    gone = set(int(i) for i in drop)
    return [h for i, h in enumerate(hs) if i not in gone]


def start_of(hs, i):
    """byte at which haystack i starts in the padded-16 layout (i == len(hs): where the list ends)"""
    return sum((blen(h) + 15) & ~15 for h in hs[:i])


def same_as_fresh(cp, cur, needles=(("linux", {}),), full=False, view=True):
    fresh = F.Corpus(cur)
    info = check_layout(cp, cur, fresh, view=view)
    if cur:
        check_parity(cp, fresh, Expected(cur), list(needles), full=full)
    return info


def snapshot(cp):
    return {k: cp.debug_read(k) for k in ("bytes", "ends") + VIEW_ARRAYS}, cp.info()


def assert_untouched(cp, snap):
    arrays, info = snap
    assert cp.info() == info
    for k, a in arrays.items():
        assert np.array_equal(cp.debug_read(k), a), k


def check_edit_info(cp, old, i0, had_view):
    """fzb_corpus_edit_info after an edit of the list `old` whose smallest touched index is i0: the first changed haystack, the bound on
    the bytes written - the old used bytes behind start(i0), more only where the list grew, + 8 per offset behind i0 - and the view's tiles"""
    ei, info = cp.edit_info(), cp.info()
    assert ei["first"] == i0
    old_used, new_used, s0 = start_of(old, len(old)), info["bytes"], start_of(old, i0)
    assert ei["bytes_written"] <= max(old_used, new_used) - s0 + 8 * (len(old) - i0), (ei, old_used, new_used, s0)
    tiles = (len(cp) + TILE - 1) // TILE
    if info["has_view"]:
        assert ei["view_tiles"] == tiles - (min(i0, len(cp)) // TILE if had_view else 0), (ei, tiles, i0, had_view)
    else:
        assert ei["view_tiles"] == 0
    assert ei["temp_bytes"] > 0
    return ei


# ---- remove ---------------------------------------------------------------------------------------------------------------------------
def removal_cases(n, rng):
    tiles = (n + TILE - 1) // TILE
    block = (1000, 1050) if n > 1100 else (n // 2, n // 2 + 50)
    mixed = [rng.randrange(n) for _ in range(max(3, n // 50))]
    mixed = mixed + mixed[:len(mixed) // 3] + [n - 1, 0, n - 1]
    rng.shuffle(mixed)
    return [
        ("nothing", []),
        ("first", [0]),
        ("last", [n - 1]),
        ("everything", list(range(n))),
        ("one per tile", [t * TILE + (t * 37) % min(TILE, n - t * TILE) for t in range(tiles)]),
        ("block across a tile boundary", list(range(*block))),
        ("1 %", rng.sample(range(n), max(1, n // 100))),
        ("50 %", rng.sample(range(n), n // 2)),
        ("99 %", rng.sample(range(n), n * 99 // 100)),
        ("unsorted with repeats", mixed),
    ]


@pytest.mark.parametrize("n", [700, 3500, 70000])
@pytest.mark.parametrize("kind", KINDS)
def test_removal_answers_and_lies_like_a_fresh_upload(kind, n):
    hs = make_list(kind, n, seed=2)
    needles = needles_for(kind)
    total = 0
    for label, drop in removal_cases(n, random.Random(n + len(kind))):
        cp = F.Corpus(hs)
        had_view = cp.info()["has_view"]
        before = cp.debug_read("bytes")
        cp.remove(drop)
        cur = without(hs, drop)
        fresh = F.Corpus(cur)
        try:
            check_layout(cp, cur, fresh)
            if cur:
                total += check_parity(cp, fresh, Expected(cur), needles, full=True)
        except AssertionError as e:
            raise AssertionError(f"{kind} n={n} removing {label}: {e}") from e
        if drop:
            i0 = min(drop)
            check_edit_info(cp, hs, i0, had_view)
            s0 = start_of(hs, i0)
            assert np.array_equal(cp.debug_read("bytes")[:s0], before[:s0]), f"{label}: bytes in front of the first removed haystack changed"
        else:
            assert cp.edit_info() == dict(first=0, bytes_written=0, view_tiles=0, temp_bytes=0)
    assert total > 50, "the lists hold matches"


def test_index_list_on_the_device_drops_everything_that_matches():
    import torch
    hs = make_list("outliers", 30000, seed=4)
    n = len(hs)
    cp = F.Corpus(hs)
    fm, om = single("linux", sort="IndexAsc")
    hits = om.match_list(hs)["index"].tolist()
    assert 100 < len(hits) < n
    recs = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    fm.match_list_device(cp, recs.data_ptr(), n, cnt.data_ptr())
    torch.cuda.synchronize()
    assert int(cnt[0]) == len(hits)
    # max_count below the count: only the prefix of the records goes (they are in index order)
    cp.remove_device(recs.data_ptr(), 8, cnt.data_ptr(), 40)
    cur = without(hs, hits[:40])
    same_as_fresh(cp, cur)
    assert cp.edit_info()["first"] == hits[0]
    # the whole result of a query over the corpus as it is now, straight from the record buffer
    fm.match_list_device(cp, recs.data_ptr(), n, cnt.data_ptr())
    torch.cuda.synchronize()
    assert int(cnt[0]) == len(hits) - 40
    cp.remove_device(recs.data_ptr(), 8, cnt.data_ptr(), n)
    cur = without(hs, hits)
    assert len(fm.match_list(cp)) == 0 and len(cp) == n - len(hits)
    same_as_fresh(cp, cur, needles=(("src", {}), ("linux", {})))
    # a multi-pattern query's records, and a count of zero
    mm = F.MultiMatcher(F.parse_query("src !test"), F.Config(pf_lanes=64, sw_lanes=0))
    want = O.MultiMatcher(O.parse_query("src !test"), lanes=(64, 64, 32), sort="IndexAsc").match_list(cur)["index"].tolist()
    mm.match_list_device(cp, recs.data_ptr(), n, cnt.data_ptr())
    torch.cuda.synchronize()
    assert int(cnt[0]) == len(want) > 0
    cp.remove_device(recs.data_ptr(), 8, cnt.data_ptr(), n)
    cur = without(cur, want)
    same_as_fresh(cp, cur)
    last = cp.edit_info()
    cnt.zero_()
    torch.cuda.synchronize()
    cp.remove_device(recs.data_ptr(), 8, cnt.data_ptr(), n)
    assert len(cp) == len(cur) and cp.edit_info() == last
    # a plain index list: stride 4
    ix = torch.tensor([5, 1, 5, len(cur) - 1], dtype=torch.int32, device="cuda")
    cnt[0] = 4
    torch.cuda.synchronize()
    cp.remove_device(ix.data_ptr(), 4, cnt.data_ptr(), 100)
    same_as_fresh(cp, without(cur, [5, 1, len(cur) - 1]))


# ---- removals and replacements that change the corpus' figures ------------------------------------------------------------------------
def test_removing_every_outlier_and_bringing_them_back():
    hs = make_list("outliers", 5000, seed=5)
    out = [i for i, h in enumerate(hs) if blen(h) > 256]
    assert len(out) >= 10
    cp = F.Corpus(hs)
    assert cp.info()["outliers"] == len(out)
    cp.remove(out)
    cur = without(hs, out)
    info = same_as_fresh(cp, cur, needles=(("linux", {}), (LONG_NEEDLE, {})))
    assert info["outliers"] == 0 and info["has_view"] == 1 and info["max_len"] == max(blen(h) for h in cur) <= 128
    at = [7, 2047, 2048, len(cur) - 1]
    cur2 = list(cur)
    for k, i in enumerate(at):
        cur2[i] = hs[out[k]]
    cp.replace(at, [cur2[i] for i in at])
    info = same_as_fresh(cp, cur2, needles=(("linux", {}), (LONG_NEEDLE, {})))
    assert info["outliers"] == 4 and info["max_len"] == max(blen(h) for h in cur2) > 256
    # more outliers than a view tolerates (5000 // 256 + 64 = 83): the view goes, and comes back when they do
    many = list(range(100, 200))
    cur3 = list(cur2)
    for i in many:
        cur3[i] = "src/linux/" + "y" * (300 + i)
    cp.replace(many, [cur3[i] for i in many])
    assert same_as_fresh(cp, cur3)["has_view"] == 0
    cp.remove(many[:60])
    assert same_as_fresh(cp, without(cur3, many[:60]))["has_view"] == 1


def test_removing_until_the_list_is_uniform_and_back():
    uni, rag = make_list("uniform32", 3000), make_list("ragged", 600, seed=9)
    rng = random.Random(3)
    hs = list(uni)
    where = sorted(rng.sample(range(len(hs)), len(rag)))
    for k, i in enumerate(where):
        hs[i] = rag[k] if blen(rag[k]) != 32 else rag[k] + "x"
    cp = F.Corpus(hs)
    assert cp.info()["has_view"] == 1 and cp.info()["uniform_len"] == 0
    cp.remove(where)
    cur = without(hs, where)
    info = same_as_fresh(cp, cur)
    assert info["uniform_len"] == 32 and info["has_view"] == 0 and info["max_len"] == 32
    l = F.lib()
    assert l.fzb_corpus_set_uniform_len(cp.h, 32) == 0 and l.fzb_corpus_set_uniform_len(cp.h, 16) == 1
    # one haystack of another length: ragged again, with a view
    cur2 = list(cur)
    cur2[1500] = "src/linux/kernel/a_path_of_more_than_thirty_two_bytes.c"
    cp.replace([1500], [cur2[1500]])
    info = same_as_fresh(cp, cur2)
    assert info["uniform_len"] == 0 and info["has_view"] == 1 and info["max_len"] == blen(cur2[1500])
    # ... and the same length again: the list is uniform once more
    cp.replace([1500], [cur[1500]])
    assert same_as_fresh(cp, cur)["uniform_len"] == 32


def test_removing_everything_beyond_32_bytes_and_back():
    hs = make_list("ragged", 4000, seed=6)
    long_ones = [i for i, h in enumerate(hs) if blen(h) > 32]
    cp = F.Corpus(hs)
    assert cp.info()["has_view"] == 1
    cp.remove(long_ones)
    cur = without(hs, long_ones)
    info = same_as_fresh(cp, cur)
    assert info["has_view"] == 0 and info["max_len"] <= 32 and len(cur) > 100
    cur2 = list(cur)
    cur2[len(cur) // 2] = "src/linux/" + "x" * 30
    cp.replace([len(cur) // 2], [cur2[len(cur) // 2]])
    assert same_as_fresh(cp, cur2)["has_view"] == 1
    assert cp.edit_info()["view_tiles"] == (len(cur2) + TILE - 1) // TILE  # (no view before: every tile is built)


def test_removing_the_single_longest_item_and_back():
    hs = make_list("ragged", 3000, seed=7)
    hs[1234] = "src/linux/" + "z" * 190
    cp = F.Corpus(hs)
    assert cp.info()["max_len"] == 200 and cp.info()["view_nv"] == 13
    cp.remove([1234])
    cur = without(hs, [1234])
    info = same_as_fresh(cp, cur)
    assert info["max_len"] == max(blen(h) for h in cur) <= 128 and info["view_nv"] == 8
    l = F.lib()
    assert l.fzb_corpus_set_max_len(cp.h, info["max_len"]) == 0 and l.fzb_corpus_set_max_len(cp.h, info["max_len"] - 1) == 1
    cur2 = list(cur)
    cur2[2999 - 1] = hs[1234]
    cp.replace([2998], [hs[1234]])
    info = same_as_fresh(cp, cur2)
    assert info["max_len"] == 200 and info["view_nv"] == 13


# ---- replace --------------------------------------------------------------------------------------------------------------------------
def new_content(rng, old):
    what = rng.randrange(6)
    if what == 0:
        return old[:len(old) // 2]
    if what == 1:
        return old + "/linux_" + "w" * rng.randint(1, 60)
    if what == 2:
        return ""
    if what == 3:
        return "é人ü/linux/" + "ñ" * rng.randint(0, 20)
    if what == 4:
        return "src/linux/" + "q" * rng.randint(250, 700)
    return "".join(reversed(old)) if old.isascii() else old  # the same length


@pytest.mark.parametrize("n", [700, 9000])
@pytest.mark.parametrize("kind", KINDS)
def test_replacement_answers_and_lies_like_a_fresh_upload(kind, n):
    hs = make_list(kind, n, seed=3)
    rng = random.Random(n * 31 + len(kind))
    cp, cur = F.Corpus(hs), list(hs)
    for count in (1, 5, n // 20, n // 3):
        had_view = cp.info()["has_view"]
        before = cp.debug_read("bytes")
        at = rng.sample(range(n), count)
        old = list(cur)
        for i in at:
            cur[i] = new_content(rng, cur[i])
        cp.replace(at, [cur[i] for i in at])
        same_as_fresh(cp, cur, needles=needles_for(kind), full=(count == n // 20))
        check_edit_info(cp, old, min(at), had_view)
        s0 = start_of(old, min(at))
        assert np.array_equal(cp.debug_read("bytes")[:s0], before[:s0]), "bytes in front of the first replaced haystack changed"
    cp.replace([], [])
    assert len(cp) == n


def test_replace_that_forces_a_regrow_and_one_that_does_not():
    hs = make_list("ragged", 5000, seed=8)
    at = list(range(40, 5000, 50))
    cur = list(hs)
    for i in at:
        cur[i] = hs[i] + "/linux/" + "g" * 100
    cp = F.Corpus(hs)
    assert cp.info()["regrows"] == 0 and cp.info()["byte_capacity"] == cp.info()["bytes"]
    cp.replace(at, [cur[i] for i in at])
    assert cp.info()["regrows"] == 1 and cp.info()["byte_capacity"] >= 2 * start_of(hs, len(hs))
    same_as_fresh(cp, cur)
    # the second one finds room: no regrow
    cur2 = list(cur)
    for i in at[:10]:
        cur2[i] = cur[i] + "h" * 64
    cp.replace(at[:10], [cur2[i] for i in at[:10]])
    assert cp.info()["regrows"] == 1
    same_as_fresh(cp, cur2)
    # a reserved corpus: nothing regrows, capacity is kept
    cp = F.Corpus(hs)
    cp.reserve(6000, 2 * start_of(hs, len(hs)))
    cap = cp.info()
    cp.replace(at, [cur[i] for i in at])
    info = same_as_fresh(cp, cur)
    assert info["regrows"] == 0 and info["item_capacity"] == cap["item_capacity"] and info["byte_capacity"] == cap["byte_capacity"]
    cp.remove(at)
    info = same_as_fresh(cp, without(cur, at))
    assert info["regrows"] == 0 and info["item_capacity"] == cap["item_capacity"] and info["byte_capacity"] == cap["byte_capacity"]


# ---- interleaving ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_random_sequences_of_every_call(seed):
    rng = random.Random(seed)
    kind = KINDS[seed % len(KINDS)]
    pool = make_list(kind, 9000, seed=seed) + make_list("outliers", 600, seed=seed + 10) + make_list("uniform32", 400, seed=seed + 20)
    rng.shuffle(pool)
    cur = pool[:rng.randint(0, 2500)]
    cp = F.Corpus(cur)
    ops = []
    for step in range(24):
        op = rng.choice(["append", "truncate", "reserve", "remove", "remove", "replace", "replace"]) if cur else "append"
        if op == "append":
            batch = [rng.choice(pool) for _ in range(rng.choice([1, 63, 1024, 1500]))]
            cp.append(batch)
            cur = cur + batch
        elif op == "truncate":
            n = rng.randint(max(0, len(cur) - 1200), len(cur))
            cp.truncate(n)
            cur = cur[:n]
        elif op == "reserve":
            cp.reserve(len(cur) + rng.randint(0, 3000), start_of(cur, len(cur)) + rng.randint(0, 200000))
        elif op == "remove":
            drop = rng.sample(range(len(cur)), rng.choice([1, max(1, len(cur) // 100), max(1, len(cur) // 3)]))
            drop += drop[:2]
            cp.remove(drop)
            cur = without(cur, drop)
        else:
            at = rng.sample(range(len(cur)), rng.choice([1, min(len(cur), 30), max(1, len(cur) // 10)]))
            cur = list(cur)
            for i in at:
                cur[i] = new_content(rng, cur[i]) if rng.random() < 0.7 else rng.choice(pool)
            cp.replace(at, [cur[i] for i in at])
        ops.append((op, len(cur)))
        try:
            check_layout(cp, cur, F.Corpus(cur), view=(step % 3 == 2 or step == 23))
        except AssertionError as e:
            raise AssertionError(f"seed {seed} after {ops}: {e}") from e
    if len(cur) < 50:
        cp.append(pool[:500])
        cur = cur + pool[:500]
    same_as_fresh(cp, cur, needles=needles_for(kind), full=True)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_corpus_untouched():
    import torch
    hs = make_list("outliers", 3000, seed=8)
    cp = F.Corpus(hs[:2000])
    cp.append(hs[2000:])
    cp.remove([17, 2500])
    cur = without(hs, [17, 2500])
    n = len(cur)
    fm = F.Matcher("linux", F.Config(pf_lanes=64))
    before, snap, last = fm.match_list(cp), snapshot(cp), cp.edit_info()
    assert snap[1]["has_view"] == 1

    def refused(call, match):
        with pytest.raises(F.FrizbeeError, match=match) as e:
            call()
        assert e.value.code == 1
        assert_untouched(cp, snap)
        assert cp.edit_info() == last and len(cp) == n

    refused(lambda: cp.remove([3, n, 5]), f"index {n} at position 1")
    refused(lambda: cp.replace([3, n], ["a", "b"]), f"index {n} at position 1")
    refused(lambda: cp.replace([3, 900, 3], ["a", "b", "c"]), "named twice")
    data, ends = F.pack(["abc", "defgh", "ij"])
    ends = ends.copy()
    ends[1] = 2
    refused(lambda: cp.replace([1, 2, 3], packed=(data, ends)), "end_offsets must be non-decreasing")
    ix = torch.tensor([4, 8, n + 7, 15, n, 16], dtype=torch.int32, device="cuda")
    cnt = torch.tensor([6, 0], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    refused(lambda: cp.remove_device(ix.data_ptr(), 4, cnt.data_ptr(), 6), "position 2")
    refused(lambda: cp.remove_device(ix.data_ptr(), 8, cnt.data_ptr(), 3), "position 1")  # (words 0, 2, 4)
    refused(lambda: cp.remove_device(ix.data_ptr(), 6, cnt.data_ptr(), 6), "stride_bytes")
    assert fm.match_list(cp).tolist() == before.tolist()
    cp.remove_device(ix.data_ptr(), 4, cnt.data_ptr(), 2)  # the entries in front of the bad one are fine on their own
    same_as_fresh(cp, without(cur, [4, 8]))


def test_borrowed_corpus_is_refused():
    import torch
    data = torch.zeros(4 * 32 + 96, dtype=torch.uint8, device="cuda")
    ends = torch.tensor([32, 64, 96, 128], dtype=torch.int32, device="cuda")
    ix = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cp = F.Corpus.from_device(data.data_ptr(), ends.data_ptr(), 4, 4 * 32 + 96, keep=(data, ends))
    for call in (lambda: cp.remove([1]), lambda: cp.replace([1], ["abc"]), lambda: cp.remove_device(ix.data_ptr(), 4, ix.data_ptr() + 4, 1)):
        with pytest.raises(F.FrizbeeError, match="borrows") as e:
            call()
        assert e.value.code == 1
    assert len(cp) == 4 and cp.info()["items"] == 4 and ends.tolist() == [32, 64, 96, 128]
    assert cp.edit_info() == dict(first=0, bytes_written=0, view_tiles=0, temp_bytes=0)


def test_wrong_current_device_is_refused():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    hs = make_list("ragged", 2000)
    cp = F.Corpus(hs)
    snap = snapshot(cp)
    try:
        torch.cuda.set_device(1)
        for call in (lambda: cp.remove([1]), lambda: cp.replace([1], ["abc"])):
            with pytest.raises(F.FrizbeeError, match="current device"):
                call()
    finally:
        torch.cuda.set_device(0)
    assert_untouched(cp, snap)


# ---- the chunks of the pass -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ragged", "outliers", "uniform32"])
def test_small_chunks_give_the_same_corpus(kind):
    """FZB_EDIT_CHUNK_ITEMS=8192: the 70 000-haystack list goes through the pass in 9 chunks (by default: in one)"""
    n = 70000
    hs = make_list(kind, n, seed=2)
    rng = random.Random(99)
    cases = [c for c in removal_cases(n, rng) if c[0] in ("first", "one per tile", "1 %", "50 %", "99 %", "unsorted with repeats")]
    at = rng.sample(range(n), 700)
    shrunk, mixed = list(hs), list(hs)
    for i in at:
        shrunk[i] = hs[i][:blen(hs[i]) // 2] if hs[i].isascii() else ""
        mixed[i] = new_content(rng, hs[i])
    whole = {}
    for label, drop in cases[:2]:
        cp = F.Corpus(hs)
        cp.remove(drop)
        whole[label] = cp.edit_info()["temp_bytes"]
    saved = os.environ.get("FZB_EDIT_CHUNK_ITEMS")
    try:
        os.environ["FZB_EDIT_CHUNK_ITEMS"] = "8192"
        F.lib().fzb_debug_reload_knobs()
        for label, drop in cases:
            cp = F.Corpus(hs)
            cp.remove(drop)
            try:
                same_as_fresh(cp, without(hs, drop), full=(label == "50 %"))
            except AssertionError as e:
                raise AssertionError(f"{kind} removing {label} in chunks: {e}") from e
            if label in whole:  # the scratch holds one chunk of at most 8192 haystacks, not the suffix
                assert cp.edit_info()["temp_bytes"] < whole[label] / 4, (label, cp.edit_info(), whole[label])
        for new in (shrunk, mixed):  # a replace that only shrinks goes chunk by chunk; one that grows items may have to go in one piece
            cp = F.Corpus(hs)
            cp.replace(at, [new[i] for i in at])
            same_as_fresh(cp, new)
    finally:
        if saved is None:
            os.environ.pop("FZB_EDIT_CHUNK_ITEMS", None)
        else:
            os.environ["FZB_EDIT_CHUNK_ITEMS"] = saved
        F.lib().fzb_debug_reload_knobs()


# ---- one large list -------------------------------------------------------------------------------------------------------------------
def test_two_million_haystacks():
    """the hazard the pass must avoid - a destination that overlaps a source another workgroup has not read - only shows across many
    workgroups: 2.2 M ragged haystacks, two chunks of the default size"""
    n = 2_200_000
    rng = random.Random(5)
    words = ["src", "linux", "kernel", "test", "drivers", "net", "include", "lib", "main", "util", "fs", "arch", "x86"]
    hs = ["/".join(rng.choice(words) for _ in range(rng.randint(1, 14))) + str(i) for i in range(n)]
    cp = F.Corpus(hs)
    drop = rng.sample(range(n), n // 100)
    cp.remove(drop)
    cur = without(hs, drop)
    assert cp.edit_info()["first"] == min(drop)
    at = rng.sample(range(len(cur)), 1000)
    for i in at:
        cur[i] = new_content(rng, cur[i])
    cp.replace(at, [cur[i] for i in at])
    fresh = F.Corpus(cur)
    check_layout(cp, cur, fresh, view=False)
    for k in ("vlen", "vgnv", "vgofs"):  # (vperm's order of equal lengths is free; lengths, group codes and block offsets are not)
        assert np.array_equal(cp.debug_read(k), fresh.debug_read(k)), k
    fm, om = single("linuxkerneltest")
    want = om.match_list(cur)
    assert len(want) > 1000
    assert fm.match_list(cp).tolist() == want.tolist() and fm.match_list(fresh).tolist() == want.tolist()
