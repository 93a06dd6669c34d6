"""frizbee_amd/csrc/prompt_records.h on the host (tests/kernel_host/prompt_host.cpp): the empty prompt's per-item rule - visible under the
scope, index = index_offset + the item, score = clamp(bias, 0, 65535), exact 0 - over ranges and item lists, against a numpy model; the
flag-then-compact walk with the grid and the batch of tiles as parameters, so that several tiles per workgroup and more than one batch are
reached at small sizes."""
import numpy as np
import pytest

import prompt_host_lib as P

pytestmark = pytest.mark.skipif(not P.available(), reason="ROCm clang++ not installed")

LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)
EDGE_BIASES = (-32768, -1, 0, 1, 255, 256, 32767)


def model(n, items, tags, bias, first, index_offset, require, exclude):
    """(index, rest) rows of the rule: rest = the score in the low half, exact = valid = 0"""
    local = np.arange(n, dtype=np.int64) if items is None else np.asarray(items, np.int64)
    h = first + local
    keep = np.ones(len(local), bool)
    if tags is not None:
        t = tags[h].astype(np.uint32)
        keep = ((t & require) == require) & ((t & exclude) == 0)
    out = np.zeros((int(keep.sum()), 2), np.uint32)
    out[:, 0] = ((index_offset + local[keep]) & 0xFFFFFFFF).astype(np.uint32)
    if bias is not None:
        out[:, 1] = np.clip(bias[h[keep]].astype(np.int64), 0, 65535).astype(np.uint32)
    return out


def biases(rng, n):
    b = rng.integers(-32768, 32768, n).astype(np.int16)
    at = rng.integers(0, n, min(n, 4 * len(EDGE_BIASES)))
    b[at] = np.resize(np.array(EDGE_BIASES, np.int16), len(at))
    return b


def ptr(a):
    return None if a is None else a.ctypes.data


def compact(n, items, tags, bias, n_cols, first, index_offset, require, exclude, grid, batch, capacity, order=None):
    order = np.arange(grid, dtype=np.uint32) if order is None else np.asarray(order, np.uint32)
    out = np.full((capacity + 8, 2), 0xABABABAB, np.uint32)
    pair = np.full(2, 0xFFFFFFFF, np.uint32)
    P.lib().ph_compact(ptr(items), n, ptr(tags), n_cols, ptr(bias), n_cols, first, index_offset, require, exclude, grid, batch, order.ctypes.data, out.ctypes.data, capacity,
                       pair.ctypes.data)
    return out, pair


@pytest.mark.parametrize("n", LENGTHS)
def test_whole_range_without_a_scope(n):
    rng = np.random.default_rng(n)
    assert P.lib().ph_tile() == 1024
    for first, index_offset in ((0, 0), (37, 50), (5, 4_000_000_000)):
        total = first + n + 3
        for bias in (None, biases(rng, total)):
            want = model(n, None, None, bias, first, index_offset, 0, 0)
            for capacity in sorted({n + 1, n, n // 2, 0}):
                out = np.full((capacity + 8, 2), 0xABABABAB, np.uint32)
                pair = np.full(2, 0xFFFFFFFF, np.uint32)
                P.lib().ph_records(out.ctypes.data, n, capacity, ptr(bias), total, first, index_offset, pair.ctypes.data)
                w = min(n, capacity)
                assert pair.tolist() == [w, n], (first, capacity)
                assert np.array_equal(out[:w], want[:w]) and (out[w:] == 0xABABABAB).all(), (first, capacity)


@pytest.mark.parametrize("n", LENGTHS)
def test_scoped_range_against_numpy(n):
    rng = np.random.default_rng(100 + n)
    for first, index_offset in ((0, 0), (37, 50)):
        total = first + n + 5
        bias = biases(rng, total)
        tag_sets = {
            "random": rng.integers(0, 65536, total).astype(np.uint16),
            "few_bits": rng.integers(0, 8, total).astype(np.uint16),
        }
        for name, tags in tag_sets.items():
            scopes = [(0, 0), (1, 2), (0, 0xFFFF), (0xFFFF, 0), (4, 4), (int(rng.integers(0, 8)), int(rng.integers(0, 8)))]
            for require, exclude in scopes:  # (0, 0) and (0, 0 over tags of 0) hide none; (4, 4) hides all
                for b in (bias, None):
                    want = model(n, None, tags, b, first, index_offset, require, exclude)
                    for grid, batch in ((1, 256), (2, 2), (3, 1), (7, 3), (512, 256)):
                        out, pair = compact(n, None, tags, b, total, first, index_offset, require, exclude, grid, batch, n + 1, order=rng.permutation(grid))
                        assert pair.tolist() == [len(want), len(want)], (name, require, exclude, grid, batch)
                        assert np.array_equal(out[: len(want)], want), (name, require, exclude, grid, batch)
                        assert (out[len(want):] == 0xABABABAB).all(), "wrote beyond the kept count"
                if require & exclude:
                    assert len(want) == 0
        hides_none = model(n, None, np.zeros(total, np.uint16), bias, first, index_offset, 0, 1)
        assert len(hides_none) == n


@pytest.mark.parametrize("total", (1, 65, 1025, 5000))
def test_item_lists_from_empty_to_all(total):
    rng = np.random.default_rng(7 + total)
    bias = biases(rng, total)
    tags = rng.integers(0, 4, total).astype(np.uint16)
    for k in sorted({0, 1, total // 20, total // 2, total - 1, total}):
        items = np.sort(rng.choice(total, k, replace=False)).astype(np.uint32)
        for t, b, require, exclude in ((None, None, 0, 0), (None, bias, 0, 0), (tags, None, 1, 0), (tags, bias, 1, 2), (tags, bias, 0, 3), (tags, bias, 2, 2)):
            want = model(k, items, t, b, 0, 0, require, exclude)
            for grid, batch in ((1, 256), (2, 1), (5, 2)):
                out, pair = compact(k, items if k else None, t, b, total, 0, 0, require, exclude, grid, batch, total)
                assert pair.tolist() == [len(want), len(want)], (k, require, exclude, grid)
                assert np.array_equal(out[: len(want)], want) and (out[len(want):] == 0xABABABAB).all(), (k, require, exclude, grid)


@pytest.mark.parametrize("n", (65, 1025, 5000))
def test_too_little_room_writes_the_prefix_and_reports_the_kept_count(n):
    rng = np.random.default_rng(n)
    bias = biases(rng, n)
    tags = (rng.random(n) < 0.5).astype(np.uint16)
    want = model(n, None, tags, bias, 0, 0, 0, 1)
    for capacity in (0, 1, len(want) // 2, len(want) - 1, len(want)):
        out, pair = compact(n, None, tags, bias, n, 0, 0, 0, 1, 4, 2, capacity)
        assert pair.tolist() == [min(capacity, len(want)), len(want)], capacity
        assert np.array_equal(out[:capacity], want[:capacity]) and (out[capacity:] == 0xABABABAB).all(), capacity


def test_a_haystack_outside_the_columns_has_tag_and_bias_zero():
    items = np.array([0, 5, 900], np.uint32)
    tags = np.ones(6, np.uint16)
    bias = np.full(6, 9, np.int16)
    out, pair = compact(3, items, tags, bias, 6, 0, 0, 1, 0, 1, 256, 3)
    assert pair.tolist() == [2, 2] and out[:2].tolist() == [[0, 9], [5, 9]]
    out, pair = compact(3, items, tags, bias, 6, 0, 0, 0, 1, 1, 256, 3)
    assert pair.tolist() == [1, 1] and out[:1].tolist() == [[900, 0]]
