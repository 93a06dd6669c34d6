"""frizbee_amd/csrc/tile_compact.h on the host (tests/kernel_host/tile_compact_host.cpp): the partition of tiles into runs against
arithmetic written here, both rank functions against numpy's bit counts, and the prefix / scan / rank walk of the record compaction over
random bitmaps against numpy.flatnonzero - with the grid and the batch of tiles as parameters and the workgroups in every order."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

import tile_compact_host_lib as T

pytestmark = pytest.mark.skipif(not T.available(), reason="ROCm clang++ not installed")

TILE = 1024
GRIDS = list(range(1, 71))


def run_of(ntiles, per, b):
    out = (C.c_uint32 * 2)()
    T.lib().tch_run(ntiles, per, b, out)
    return out[0], out[1]


@pytest.mark.parametrize("ntiles", list(range(0, 71)) + [(1 << 22) - 1, 1 << 22, (1 << 22) + 1, (1 << 31) - 1, (1 << 32) - 70, (1 << 32) - 1])
def test_runs_are_disjoint_ascending_and_cover_every_tile(ntiles):
    """(1 << 22: the tiles of 2^32 items; near 2^32 the products block * per and t0 + per leave 32 bits)"""
    assert T.lib().tch_tile() == TILE
    for grid in GRIDS:
        per = T.lib().tch_tiles_per_run(ntiles, grid)
        assert per == -(-ntiles // grid), (ntiles, grid)
        nxt = 0
        for b in range(grid):
            t0, t1 = run_of(ntiles, per, b)
            assert (t0, t1) == (min(b * per, ntiles), min(b * per + per, ntiles)), (ntiles, grid, b)  # Python integers: no wrap
            assert t0 == nxt and t0 <= t1 <= ntiles, (ntiles, grid, b)
            nxt = t1
        assert nxt == ntiles, (ntiles, grid)
        if grid > ntiles:  # a tile each, then empty runs
            assert per == (1 if ntiles else 0) and run_of(ntiles, per, grid - 1) == (ntiles, ntiles)
    assert T.lib().tch_tiles_per_run(ntiles, 0) == 0


def test_grid_of_a_pass():
    for units, grid_max, want in ((0, 8, 1), (1, 8, 1), (7, 8, 7), (8, 8, 8), (9, 8, 8), (5, 0, 1), (5, -3, 1), (0, 0, 1), (1 << 40, 512, 512)):
        assert T.lib().tch_grid(units, grid_max) == want, (units, grid_max)


def special_words(bits):
    full = (1 << bits) - 1
    return [0, full, 1, 1 << (bits - 1), full ^ 1, full >> 1] + [1 << b for b in range(bits)]


@pytest.mark.parametrize("bits", (64, 32))
def test_rank_against_numpy_bit_counts(bits):
    rng = np.random.default_rng(bits)
    dt = np.uint64 if bits == 64 else np.uint32
    words = np.concatenate([np.array(special_words(bits), dt), rng.integers(0, 1 << bits, 3000, dtype=np.uint64).astype(dt)])
    words = np.repeat(words, bits)
    at = np.tile(np.arange(bits, dtype=np.uint32), len(words) // bits)  # every bit position of every word: 0, 31 and 63 among them
    before = rng.integers(0, 1 << 31, len(words)).astype(np.uint32)
    out = np.zeros(len(words), np.uint32)
    fn = T.lib().tch_rank64 if bits == 64 else T.lib().tch_rank32
    fn(words.ctypes.data, at.ctypes.data, before.ctypes.data, len(words), out.ctypes.data)
    below = words.astype(np.uint64) & ((np.uint64(1) << at.astype(np.uint64)) - np.uint64(1))
    want = before + np.unpackbits(below.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.uint32)
    assert np.array_equal(out, want)


def walk(bitmap, n, grid, batch, order, bounded, capacity):
    out = np.full(capacity + 8, 0xABABABAB, np.uint32)
    pair = np.full(2, 0xFFFFFFFF, np.uint32)
    order = np.asarray(order, np.uint32)
    T.lib().tch_walk(bitmap.ctypes.data, n, grid, batch, order.ctypes.data, int(bounded), out.ctypes.data, capacity, pair.ctypes.data)
    return out, pair


def orders(rng, grid):
    """every order of up to four workgroups; the two plain ones and three random ones beyond"""
    if grid <= 4:
        return list(itertools.permutations(range(grid)))
    return [np.arange(grid), np.arange(grid)[::-1].copy()] + [rng.permutation(grid) for _ in range(3)]


@pytest.mark.parametrize("ntiles", (0, 1, 2, 3, 5, 8, 13, 40))
def test_prefix_scan_and_rank_against_flatnonzero(ntiles):
    rng = np.random.default_rng(500 + ntiles)
    for n in sorted({0 if not ntiles else (ntiles - 1) * TILE + k for k in (1, 63, 65, 1023, 1024)}):
        for density in (0.0, 0.03, 0.5, 1.0):
            keep = rng.random(n) < density if density < 1 else np.ones(n, bool)
            bits = np.zeros(-(-n // TILE) * TILE, np.uint8)
            bits[:n] = keep
            bitmap = np.packbits(bits, bitorder="little").view(np.uint64) if n else np.zeros(1, np.uint64)
            want = np.flatnonzero(keep).astype(np.uint32)
            for grid, batch in ((1, 256), (1, 1), (2, 3), (3, 1), (4, 256), (7, 3), (64, 256)):
                for order in orders(rng, grid):
                    out, pair = walk(bitmap, n, grid, batch, order, False, len(want))
                    assert pair[0] == len(want), (n, density, grid, batch)
                    assert np.array_equal(out[:len(want)], want) and (out[len(want):] == 0xABABABAB).all(), (n, density, grid, batch, list(order))
                for capacity in sorted({0, 1, len(want) // 2, max(len(want), 1) - 1, len(want), len(want) + 5}):
                    out, pair = walk(bitmap, n, grid, batch, rng.permutation(grid), True, capacity)
                    assert pair.tolist() == [min(capacity, len(want)), len(want)], (n, density, grid, batch, capacity)
                    k = min(capacity, len(want))
                    assert np.array_equal(out[:k], want[:k]) and (out[k:] == 0xABABABAB).all(), (n, density, grid, batch, capacity)


def test_the_walk_as_a_stand_alone_program_under_address_and_ub_sanitizers():
    """the same source with its own main, built with -fsanitize=address,undefined and run as a process of its own"""
    r = subprocess.run([T.build_sanitized()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith(" 0 mismatches") and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])
