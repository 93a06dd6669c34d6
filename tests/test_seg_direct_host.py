"""frizbee_amd/csrc/seg_list.h on the host (tests/kernel_host/seg_direct_host.cpp): the scorer's work assignment over the segmented survivor
list.  Workgroup b takes the first 128 survivors of segment b directly, everything else is a pool walked grid-strided; the union of both must
be every (segment, slot) pair exactly once, and the output positions exactly 0 .. total - 1 in ascending index order - against brute-force
enumeration in numpy, with the plain search and with the kernel's padded eleven-step form."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "kernel_host")
CSRC = os.path.join(ROOT, "frizbee_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SEG_MAX = 2048
THREADS = 128  # k2b_dp_short's workgroup
STRIDE = 5 * 1024  # a segment of five tiles, every row a survivor

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="needs ROCm's clang++")

_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libseg_direct_host.so")
        src = os.path.join(HERE, "seg_direct_host.cpp")
        deps = [src, os.path.join(HERE, "shim", "hip", "hip_runtime.h"), os.path.join(CSRC, "seg_list.h"), os.path.join(CSRC, "tile_compact.h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            tmp = so + ".tmp.%d" % os.getpid()
            subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + os.path.join(HERE, "shim"), "-I" + CSRC, "-Wall", "-Werror", "-o", tmp, src])
            os.replace(tmp, so)
        l = C.CDLL(so)
        u32, p32 = C.c_uint32, C.POINTER(C.c_uint32)
        l.sd_direct_max.restype = u32
        for f in (l.sd_direct, l.sd_rest):
            f.argtypes = [u32, u32, u32]
            f.restype = u32
        l.sd_walk.argtypes = [p32, u32, u32, u32, C.c_int, p32, p32, p32, p32, p32, p32, p32, C.c_uint64]
        l.sd_walk.restype = C.c_int64
        _lib = l
    return _lib


def ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def walk(counts, G, padded):
    counts = np.ascontiguousarray(counts, np.uint32)
    nseg, total = len(counts), int(counts.sum(dtype=np.uint64))
    pre, rpre, totals = np.zeros(SEG_MAX, np.uint32), np.zeros(SEG_MAX, np.uint32), np.zeros(2, np.uint32)
    out = [np.full(total + 1, 0xFFFFFFFF, np.uint32) for _ in range(4)]
    n = lib().sd_walk(ptr(counts), nseg, G, THREADS, int(padded), ptr(pre), ptr(rpre), ptr(totals), *[ptr(o) for o in out], total)
    return n, pre[:nseg], rpre[:nseg], totals, [o[:total] for o in out]


def check(counts, G):
    counts = np.asarray(counts, np.uint32)
    nseg, total = len(counts), int(counts.sum(dtype=np.uint64))
    seg_of = np.arange(nseg)
    d = np.where(seg_of < G, np.minimum(counts, 128), 0)
    want_pre = np.concatenate(([0], np.cumsum(counts, dtype=np.uint64)[:-1])).astype(np.uint32)
    want_rpre = np.concatenate(([0], np.cumsum(counts - d, dtype=np.uint64)[:-1])).astype(np.uint32)
    # brute force: every (segment, slot) pair in ascending order is output position 0, 1, 2, ...
    want_seg = np.repeat(seg_of, counts).astype(np.uint32)
    want_slot = (np.arange(total, dtype=np.uint64) - np.repeat(want_pre.astype(np.uint64), counts)).astype(np.uint32)
    for padded in (False, True):
        n, pre, rpre, totals, (seg, slot, pos, wg) = walk(counts, G, padded)
        ctx = (nseg, G, padded, counts[:12].tolist())
        assert n == total, ctx  # (-1: more items than pairs)
        assert totals.tolist() == [total, total - int(d.sum())], ctx
        assert np.array_equal(pre, want_pre) and np.array_equal(rpre, want_rpre), ctx
        order = np.argsort(pos, kind="stable")
        assert np.array_equal(pos[order], np.arange(total, dtype=np.uint32)), ctx  # exactly 0 .. total - 1, each once
        assert np.array_equal(seg[order], want_seg) and np.array_equal(slot[order], want_slot), ctx  # ... in ascending index order, every pair once
        direct = slot < d[seg] if total else np.zeros(0, bool)
        assert np.array_equal(wg[direct], seg[direct]), ctx  # a direct item is scored by its segment's own workgroup
        assert int(direct.sum()) == int(d.sum()), ctx


def grids(nseg):
    """below, equal to and above nseg"""
    return sorted({1, max(1, nseg // 2), max(1, nseg - 1), nseg, nseg + 1, 2 * nseg + 3})


def test_direct_and_rest_of_one_segment():
    l = lib()
    assert l.sd_direct_max() == THREADS == 128
    for c in (0, 1, 127, 128, 129, STRIDE):
        for s, G in ((0, 1), (4, 5), (5, 5), (6, 5), (2047, 2048)):
            want = min(c, 128) if s < G else 0
            assert (l.sd_direct(c, s, G), l.sd_rest(c, s, G)) == (want, c - want), (c, s, G)


@pytest.mark.parametrize("nseg", (1, 2, 3))
def test_every_vector_of_the_edge_counts_on_up_to_three_segments(nseg):
    import itertools

    for counts in itertools.product((0, 1, 127, 128, 129, STRIDE), repeat=nseg):
        for G in grids(nseg):
            check(counts, G)


@pytest.mark.parametrize("nseg", (2047, 2048))
def test_random_vectors_with_long_runs_of_empty_segments(nseg):
    rng = random.Random(nseg)
    for G in grids(nseg):
        check([0] * nseg, G)  # a total of 0
    check([0] * (nseg - 1) + [129], nseg)
    check([STRIDE] + [0] * (nseg - 1), nseg - 1)
    for it in range(12):
        counts = []
        while len(counts) < nseg:
            if rng.random() < 0.5:
                counts += [0] * rng.randint(1, 300 if it % 2 else 1500)
            else:
                counts += [rng.choice((0, 1, 127, 128, 129)) if rng.random() < 0.7 else rng.randint(0, 400) for _ in range(rng.randint(1, 60))]
        counts = counts[:nseg]
        for k in rng.sample(range(nseg), 8):  # a few dense segments, first and last among them
            counts[k] = STRIDE
        counts[0 if it % 2 else nseg - 1] = STRIDE
        check(counts, grids(nseg)[it % 6])


def test_all_survivors_in_one_segment():
    for nseg, at in ((3, 1), (2048, 0), (2048, 1000), (2048, 2047), (2047, 2046)):
        for c in (1, 127, 128, 129, STRIDE):
            for G in (1, nseg, nseg + 1):
                counts = [0] * nseg
                counts[at] = c
                check(counts, G)
