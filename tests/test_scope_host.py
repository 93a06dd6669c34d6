"""frizbee_amd/csrc/scope.h on the host (tests/kernel_host/scope_host.cpp): the visibility predicate over random tags and masks, and the
flag-then-compact walk of the drop pass over record lists against numpy's boolean-mask indexing - with the grid and the batch of tiles as
parameters, so that several tiles per workgroup and more than one batch of tiles are reached at small sizes."""
import numpy as np
import pytest

import scope_host_lib as S

pytestmark = pytest.mark.skipif(not S.available(), reason="ROCm clang++ not installed")

LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)


def visible(tags, require, exclude):
    t = np.asarray(tags, np.uint32)
    return ((t & require) == require) & ((t & exclude) == 0)


def test_predicate_over_random_tags_and_masks():
    rng = np.random.default_rng(3)
    assert S.lib().sh_tile() == 1024
    tags = np.concatenate([np.arange(65536), rng.integers(0, 65536, 20000)]).astype(np.uint16)
    masks = [(0, 0), (1, 0), (0, 1), (1, 1), (0xFFFF, 0), (0, 0xFFFF), (0xFFFF, 0xFFFF), (0x8000, 0x0001), (6, 6), (3, 2)]
    masks += [(int(a), int(b)) for a, b in rng.integers(0, 65536, (20, 2))]
    masks += [(int(a) & int(b) | 4, int(b) | 4) for a, b in rng.integers(0, 65536, (5, 2))]  # require & exclude != 0
    for require, exclude in masks:
        out = np.zeros(len(tags), np.uint8)
        S.lib().sh_visible(tags.ctypes.data, len(tags), require, exclude, out.ctypes.data)
        assert np.array_equal(out.astype(bool), visible(tags, require, exclude)), (require, exclude)
        if require & exclude:  # a bit in both masks hides what has it and what lacks it
            assert not out.any()
    out = np.zeros(len(tags), np.uint8)
    S.lib().sh_visible(tags.ctypes.data, len(tags), 0, 0, out.ctypes.data)
    assert out.all()


def drop(recs, tags, first, index_offset, require, exclude, grid, batch, capacity, order=None):
    n = len(recs)
    order = np.arange(grid, dtype=np.uint32) if order is None else np.asarray(order, np.uint32)
    out = np.full((capacity + 8, 2), 0xABABABAB, np.uint32)
    pair = np.full(2, 0xFFFFFFFF, np.uint32)
    words = np.ascontiguousarray(recs, np.uint32)
    S.lib().sh_drop(words.ctypes.data if n else None, n, tags.ctypes.data, len(tags), first, index_offset, require, exclude, grid, batch, order.ctypes.data, out.ctypes.data, capacity,
                    pair.ctypes.data)
    return out, pair


def records(rng, n, span, index_offset):
    """n index-ordered records over `span` haystacks of a range numbered from index_offset: (index, payload) pairs"""
    at = np.sort(rng.choice(span, n, replace=False)) if n else np.zeros(0, np.int64)
    recs = np.zeros((n, 2), np.uint32)
    recs[:, 0] = (at + index_offset).astype(np.uint32)
    recs[:, 1] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return recs, at


@pytest.mark.parametrize("n", LENGTHS)
def test_flag_then_compact_against_numpy(n):
    rng = np.random.default_rng(100 + n)
    first, index_offset = 37, 4_000_000_000 if n < 3000 else 9
    span = n + n // 3 + 5
    n_tags = first + span
    recs, at = records(rng, n, span, index_offset)
    tag_sets = {
        "random": rng.integers(0, 8, n_tags).astype(np.uint16),
        "all_visible": np.full(n_tags, 1, np.uint16),
        "none_visible": np.full(n_tags, 2, np.uint16),
    }
    for name, tags in tag_sets.items():
        keep = visible(tags[first + at], 1, 2)
        want = recs[keep]
        for grid, batch in ((1, 256), (1, 1), (2, 2), (3, 1), (5, 256), (7, 3), (512, 256)):
            out, pair = drop(recs, tags, first, index_offset, 1, 2, grid, batch, n + 1, order=rng.permutation(grid))
            assert pair.tolist() == [len(want), len(want)], (name, grid, batch)
            assert np.array_equal(out[: len(want)], want), (name, grid, batch)
            assert (out[len(want):] == 0xABABABAB).all(), (name, grid, batch, "wrote beyond the kept count")


@pytest.mark.parametrize("n", (65, 1025, 5000))
def test_too_little_room_writes_the_prefix_and_reports_the_kept_count(n):
    rng = np.random.default_rng(n)
    recs, at = records(rng, n, n, 0)
    tags = (rng.random(n) < 0.5).astype(np.uint16)
    want = recs[visible(tags[at], 0, 1)]
    for capacity in (0, 1, len(want) // 2, len(want) - 1, len(want)):
        out, pair = drop(recs, tags, 0, 0, 0, 1, 4, 2, capacity)
        assert pair.tolist() == [min(capacity, len(want)), len(want)], capacity
        assert np.array_equal(out[:capacity], want[:capacity]) and (out[capacity:] == 0xABABABAB).all(), capacity


def test_a_record_outside_the_tags_has_tag_zero():
    """the array's invariant (every entry at or behind the list's length is zero) as the predicate sees it"""
    recs = np.array([[0, 1], [5, 2], [900, 3]], np.uint32)
    tags = np.array([1, 1, 1, 1, 1, 1], np.uint16)
    out, pair = drop(recs, tags, 0, 0, 1, 0, 1, 256, 3)
    assert pair.tolist() == [2, 2] and out[:2].tolist() == [[0, 1], [5, 2]]
    out, pair = drop(recs, tags, 0, 0, 0, 1, 1, 256, 3)
    assert pair.tolist() == [1, 1] and out[:1].tolist() == [[900, 3]]
