"""frizbee_amd/csrc/seg_list.h on the host (tests/kernel_host/seg_host.cpp): which segment holds survivor j - the LAST one whose exclusive
prefix is <= j, with empty segments anywhere -, the slot of a set bit inside its tile, and the runs of tiles the filter's workgroups own."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest

import seg_host_lib as S

pytestmark = pytest.mark.skipif(not S.available(), reason="needs ROCm's clang++")


def map_all(counts):
    """(total, segment of j, slot of j) for j in [0, total] through seg_find"""
    n = len(counts)
    c = (C.c_uint32 * max(n, 1))(*counts)
    total = int(sum(counts))
    pre = (C.c_uint32 * max(n, 1))()
    seg = (C.c_uint32 * (total + 1))()
    slot = (C.c_uint32 * (total + 1))()
    assert S.lib().sg_map_all(c, n, pre, seg, slot) == total
    return total, list(pre)[:n], list(seg), list(slot)


def want_map(counts):
    return [(s, k) for s, c in enumerate(counts) for k in range(c)]


def check(counts):
    total, pre, seg, slot = map_all(counts)
    assert pre == [int(x) for x in np.concatenate(([0], np.cumsum(counts)[:-1]))]
    assert list(zip(seg[:total], slot[:total])) == want_map(counts), counts
    # j = total maps to nothing: whatever segment the search names, the slot is not below that segment's count
    assert slot[total] >= counts[seg[total]], counts


def test_every_count_vector_up_to_six_segments():
    n = 0
    for length in range(1, 7):
        for counts in itertools.product(range(4), repeat=length):
            check(list(counts))
            n += 1
    assert n == sum(4 ** k for k in range(1, 7))


def test_random_vectors_of_2048_segments_with_long_runs_of_zeros():
    assert S.lib().sg_max() == 2048
    rng = random.Random(5)
    check([0] * 2048)  # a zero total: nothing to map, j = 0 maps to nothing
    check([0] * 2047 + [3])
    check([2] + [0] * 2047)
    for it in range(40):
        counts = []
        while len(counts) < 2048:
            if rng.random() < 0.5:
                counts += [0] * rng.randint(1, 300 if it % 2 else 1500)
            else:
                counts += [rng.choice((1, 2, 5, 1024, 5120)) if rng.random() < 0.3 else rng.randint(0, 40) for _ in range(rng.randint(1, 60))]
        nseg = 2048 if it % 3 else rng.randint(1, 2048)  # the grid is below the maximum on small devices and small lists
        check(counts[:nseg])


def test_first_step_of_the_search():
    for nseg in list(range(1, 70)) + [1023, 1024, 1025, 2047, 2048]:
        top = S.lib().sg_top(nseg)
        assert top & (top - 1) == 0 and (top < nseg or nseg == 1) and (2 * top >= nseg)


def test_slots_inside_a_tile():
    rng = random.Random(9)
    for density in (0.0, 0.002, 0.05, 0.5, 1.0):
        for _ in range(6):
            bits = [1 if rng.random() < density else 0 for _ in range(1024)]
            words = (C.c_uint32 * 32)(*[sum(bits[32 * w + b] << b for b in range(32)) for w in range(32)])
            out = (C.c_uint32 * 1024)(*([0xFFFFFFFF] * 1024))
            n = S.lib().sg_rank_tile(words, out)
            assert n == sum(bits) and list(out)[:n] == [i for i, b in enumerate(bits) if b]


def test_runs_partition_the_tiles():
    out = (C.c_uint32 * 2)()
    for ntiles, grid in ((1, 1), (20, 3), (9766, 2048), (5, 8), (2048, 2048), (2049, 2048), (7, 2), (4194304, 2048)):
        T = S.lib().sg_tiles_per_run(ntiles, grid)
        assert T == -(-ntiles // grid)
        nxt = 0
        for b in range(grid):
            S.lib().sg_run(ntiles, T, b, out)
            assert out[0] == min(b * T, ntiles) == min(nxt, ntiles) and out[1] == min((b + 1) * T, ntiles)
            nxt = out[1]
        assert nxt == ntiles
