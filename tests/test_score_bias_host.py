"""frizbee_amd/csrc/score_bias.h on the host (tests/kernel_host/bias_host.cpp): the clamp-add over every u16 score, the one-pass decision on
both sides of 256, and the tile body of the remove compaction against numpy's boolean-mask indexing."""
import numpy as np
import pytest

import bias_host_lib as B

pytestmark = pytest.mark.skipif(not B.available(), reason="ROCm clang++ not installed")

TILE = 1024


def test_clamp_add_over_every_score():
    rng = np.random.default_rng(11)
    scores = np.arange(65536, dtype=np.uint16)
    biases = [-32768, -1, 0, 1, 255, 32767] + rng.integers(-32768, 32768, 10).tolist()
    for b in biases:
        bs = np.full(65536, b, np.int16)
        out = np.zeros(65536, np.uint16)
        B.lib().bh_clamp_add(scores.ctypes.data, bs.ctypes.data, 65536, out.ctypes.data)
        want = np.clip(scores.astype(np.int64) + b, 0, 65535).astype(np.uint16)
        assert np.array_equal(out, want), b
    # random pairs
    s = rng.integers(0, 65536, 200000).astype(np.uint16)
    b = rng.integers(-32768, 32768, 200000).astype(np.int16)
    out = np.zeros(len(s), np.uint16)
    B.lib().bh_clamp_add(s.ctypes.data, b.ctypes.data, len(s), out.ctypes.data)
    assert np.array_equal(out, np.clip(s.astype(np.int64) + b, 0, 65535).astype(np.uint16))


def test_one_pass_decision_on_both_sides_of_256():
    l = B.lib()
    assert l.bh_tile() == TILE
    for bound in (0, 1, 84, 200, 255, 256, 257, 4000, 65535, 1 << 40):
        for hi in (0, 1, 55, 171, 172, 255, 256, 32767):
            assert l.bh_one_pass(bound, hi) == int(bound + hi < 256), (bound, hi)
    # the default scoring's 6-byte needle: 6 x 12 + 12 (prefix) + 8 (exact) + ... stays below 256 until the bias takes it there
    assert l.bh_one_pass(255, 0) == 1 and l.bh_one_pass(255, 1) == 0 and l.bh_one_pass(0, 255) == 1 and l.bh_one_pass(0, 256) == 0


def bitmap_of(removed):
    n = len(removed)
    words = np.zeros((n + 31) // 32 + 1, np.uint32)
    for i in np.flatnonzero(removed):
        words[i >> 5] |= np.uint32(1 << (i & 31))
    return words


def compact(removed, values, t0):
    """one tile through the header's tile body, at base 0; removed: bool per haystack of the LIST"""
    words = bitmap_of(removed)
    out = np.full(TILE, 12345, np.int16)
    k = B.lib().bh_compact_tile(words.ctypes.data, values.ctypes.data, len(removed), t0, 0, out.ctypes.data, TILE)
    return out[:k], out[k:]


@pytest.mark.parametrize("t0", [0, 32, 7, 1000, 1024 + 13])  # a first tile that starts mid-word: i0 % 32 != 0
@pytest.mark.parametrize("last", [1, 63, 64, 65, 1023, 1024])
def test_compaction_tile_against_numpy(t0, last):
    rng = np.random.default_rng(t0 * 31 + last)
    n = t0 + last
    values = rng.integers(-32768, 32768, n).astype(np.int16)
    patterns = {
        "random": rng.random(n) < 0.3,
        "mostly_removed": rng.random(n) < 0.95,
        "all_kept": np.zeros(n, bool),
        "none_kept": np.ones(n, bool),
        "single_survivor": np.ones(n, bool),
    }
    patterns["single_survivor"][t0 + int(rng.integers(0, last))] = False
    for name, removed in patterns.items():
        got, rest = compact(removed, values, t0)
        want = values[t0:n][~removed[t0:n]]
        assert np.array_equal(got, want), (name, t0, last)
        assert (rest == 12345).all(), (name, "wrote beyond the kept count")


def test_compaction_of_a_list_tile_by_tile():
    """a removal from a non-tile-aligned i0 on: tiles of 1024 source haystacks from i0, each at its scanned kept count"""
    rng = np.random.default_rng(5)
    n, i0 = 5000, 1234
    values = rng.integers(-100, 100, n).astype(np.int16)
    removed = rng.random(n) < 0.4
    removed[:i0] = False
    removed[i0] = True
    parts = [compact(removed, values, t0)[0] for t0 in range(i0, n, TILE)]
    assert np.array_equal(np.concatenate(parts), values[i0:][~removed[i0:]])
    # the way the kernel composes them: every tile writes at its scanned base into ONE scratch of the suffix' length, in any tile order
    words = bitmap_of(removed)
    starts = list(range(i0, n, TILE))
    bases = np.concatenate([[0], np.cumsum([int((~removed[t0:t0 + TILE]).sum()) for t0 in starts])])
    out = np.full(n - i0 + 8, 12345, np.int16)
    for k in rng.permutation(len(starts)):
        got = B.lib().bh_compact_tile(words.ctypes.data, values.ctypes.data, n, starts[k], int(bases[k]), out.ctypes.data, n - i0)
        assert got == bases[k + 1] - bases[k]
    kept = int(bases[-1])
    assert np.array_equal(out[:kept], values[i0:][~removed[i0:]]) and (out[kept:] == 12345).all()


def test_a_place_beyond_the_scratch_is_not_written():
    """the out_cap guard of the tile body: a base that would take a tile beyond the scratch writes nothing there"""
    n = 200
    values = np.arange(n, dtype=np.int16)
    words = bitmap_of(np.zeros(n, bool))
    out = np.full(n + 64, 12345, np.int16)
    assert B.lib().bh_compact_tile(words.ctypes.data, values.ctypes.data, n, 0, 150, out.ctypes.data, n) == n
    assert np.array_equal(out[150:n], values[:50]) and (out[:150] == 12345).all() and (out[n:] == 12345).all()
