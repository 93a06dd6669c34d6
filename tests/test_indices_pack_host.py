"""frizbee_amd/csrc/indices_pack.h - the arithmetic of the packing step behind the fused top + matched-positions query
(kernels_indices.hip) - compiled for the host through the stand-in <hip/hip_runtime.h> and fuzzed against numpy: `positions_begin` is the
exclusive sum of the clamped lengths, the dense array is the concatenation of every record's first `len` positions, the total is right -
for one tile and for the multi-tile decomposition - and a traced record that differs from the head's, or a count that is off, raises the
inconsistency word."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "kernel_host")
CSRC = os.path.join(ROOT, "frizbee_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
REC = np.dtype([("index", "<u4"), ("score", "<u2"), ("exact", "u1"), ("_pad", "u1")])
OUT = np.dtype([("index", "<u4"), ("score", "<u2"), ("exact", "u1"), ("_pad", "u1"), ("positions_begin", "<u4"), ("positions_len", "<u4")])
BAD_COUNT, BAD_RECORD = 1, 2

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ not installed")

_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libpack_host.so")
        srcs = [os.path.join(HERE, "pack_host.cpp"), os.path.join(HERE, "shim", "hip", "hip_runtime.h"), os.path.join(CSRC, "indices_pack.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + os.path.join(HERE, "shim"), "-I" + CSRC, "-Wall", "-Werror", "-o", so,
                                   os.path.join(HERE, "pack_host.cpp")])
        _lib = C.CDLL(so)
        _lib.ph_pack.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ph_pack.restype = C.c_uint32
        _lib.ph_tile.restype = C.c_uint32
    return _lib


def make(rng, n, stride):
    head = np.zeros(max(n, 1), REC)
    head["index"][:n] = rng.permutation(max(n * 3, 1))[:n]
    head["score"][:n] = rng.integers(0, 65536, n)
    head["exact"][:n] = rng.integers(0, 2, n)
    npos = rng.integers(0, stride + 4, max(n, 1)).astype(np.uint32)  # 0 .. stride + 3: beyond the stride is clamped
    pos = rng.integers(0, 1 << 32, max(n, 1) * stride, dtype=np.uint64).astype(np.uint32)
    return head, npos, pos


def pack(head, n, traced, traced_count, npos, pos, stride, max_records, found=12345):
    out = np.zeros(max(n, 1), OUT)
    dense = np.full(max(n, 1) * stride + 1, 0xDEADBEEF, np.uint32)
    counts = np.zeros(4, np.uint32)
    tiles = lib().ph_pack(head.ctypes.data, n, found, traced.ctypes.data, traced_count, npos.ctypes.data, pos.ctypes.data, stride, max_records, out.ctypes.data, dense.ctypes.data,
                          counts.ctypes.data)
    return out[:n], dense, [int(x) for x in counts], tiles


def check(head, n, npos, pos, stride, max_records):
    out, dense, counts, tiles = pack(head, n, head.copy(), n, npos, pos, stride, max_records)
    lens = np.minimum(npos[:n], stride).astype(np.int64)
    begins = np.concatenate([[0], np.cumsum(lens)[:-1]]) if n else np.zeros(0, np.int64)
    total = int(lens.sum())
    assert counts == [n, 12345, total, 0]
    assert out["positions_len"].tolist() == lens.tolist()
    assert out["positions_begin"].tolist() == begins.tolist()
    for f in ("index", "score", "exact"):
        assert out[f].tolist() == head[f][:n].tolist()
    want = np.concatenate([pos[k * stride : k * stride + lens[k]] for k in range(n)]) if n else np.zeros(0, np.uint32)
    assert np.array_equal(dense[:total], want)
    assert dense[total] == 0xDEADBEEF  # nothing behind the total is written
    return tiles


@pytest.mark.parametrize("stride", [1, 6, 64])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049, 4097, 10_000])
def test_pack_matches_numpy(n, stride):
    tile = lib().ph_tile()
    assert tile == 2048
    rng = np.random.default_rng(n * 131 + stride)
    head, npos, pos = make(rng, n, stride)
    if n <= tile:  # the picker's form: one launch, one tile
        assert check(head, n, npos, pos, stride, max_records=max(n, 1)) == (1 if n else 0)
    # the multi-tile decomposition, also for heads that would fit one tile (a limit beyond the tile with few matches)
    assert check(head, n, npos, pos, stride, max_records=max(n, tile + 1)) == (n + tile - 1) // tile


@pytest.mark.parametrize("zeros", ["all", "none", "runs"])
def test_records_without_positions(zeros):
    """the owner of a dense position is found by bisection of the begins: records with no positions share their begin with a neighbour"""
    rng = np.random.default_rng(7)
    n, stride = 3000, 6
    head, npos, pos = make(rng, n, stride)
    if zeros == "all":
        npos[:] = 0
    elif zeros == "none":
        npos[:] = stride
    else:
        npos[rng.random(len(npos)) < 0.7] = 0
        npos[100:400] = 0
        npos[2040:2060] = 0
    check(head, n, npos, pos, stride, max_records=n)
    check(head, 2048, npos, pos, stride, max_records=2048)


@pytest.mark.parametrize("n,max_records", [(100, 100), (5000, 5000)])
def test_mismatch_raises_the_flag(n, max_records):
    rng = np.random.default_rng(n)
    stride = 6
    head, npos, pos = make(rng, n, stride)
    k = n - 3
    traced = head.copy()
    traced["index"][k] += 1
    assert pack(head, n, traced, n, npos, pos, stride, max_records)[2][3] == BAD_RECORD
    traced = head.copy()
    traced["score"][k] ^= 1
    assert pack(head, n, traced, n, npos, pos, stride, max_records)[2][3] == BAD_RECORD
    traced = head.copy()
    traced["exact"][0] ^= 1
    assert pack(head, n, traced, n, npos, pos, stride, max_records)[2][3] == BAD_RECORD
    assert pack(head, n, head.copy(), n - 1, npos, pos, stride, max_records)[2][3] == BAD_COUNT
    assert pack(head, n, head.copy(), n + 1, npos, pos, stride, max_records)[2][3] == BAD_COUNT
    traced = head.copy()
    traced["score"][1] ^= 1
    assert pack(head, n, traced, n - 1, npos, pos, stride, max_records)[2][3] == BAD_COUNT | BAD_RECORD
    assert pack(head, n, head.copy(), n, npos, pos, stride, max_records)[2][3] == 0
