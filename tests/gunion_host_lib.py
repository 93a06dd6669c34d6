"""TEST INFRASTRUCTURE: builds tests/kernel_host/libgunion_host.so - frizbee_amd/csrc/indices_union_groups.h, the union step of the grouped
top + matched-positions query, compiled for the host with g++ and no HIP header - and loads it with ctypes, so that the CPU suite can fuzz
what k_gunion_where / k_gunion_merge call.  Never imported by the product."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "kernel_host")
CSRC = os.path.join(ROOT, "frizbee_amd", "csrc")
SRC = os.path.join(HERE, "gunion_host.cpp")
REC = np.dtype([("index", "<u4"), ("score", "<u2"), ("exact", "u1"), ("pad", "u1")])
BAD_COUNT, BAD_RECORD = 1, 2
NONE = 0xFFFFFFFF


def available():
    return shutil.which("g++") is not None


def build():
    so = os.path.join(HERE, "libgunion_host.so")
    srcs = [SRC] + [os.path.join(CSRC, h) for h in ("indices_union_groups.h", "indices_union.h", "indices_pack.h", "anyof.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + CSRC, "-Wall", "-Werror", "-o", so, SRC])
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build())
        u32, vp = C.c_uint32, C.c_void_p
        l.gh_by_value.restype = u32
        l.gh_absent.restype = u32
        l.gh_where.argtypes = [u32, vp, vp, vp, vp, u32, u32]
        l.gh_where.restype = None
        l.gh_union.argtypes = [u32] + [vp] * 8 + [u32, u32, u32] + [vp] * 5
        l.gh_union.restype = u32
        l.gh_check.argtypes = [vp, u32, vp, u32, u32]
        l.gh_check.restype = u32
        _lib = l
    return _lib


class _Keep:
    def __init__(self):
        self.keep = []

    def arr(self, a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        if a.size == 0:
            a = np.zeros(1, dt)
        self.keep.append(a)
        return a.ctypes.data

    def ptrs(self, xs):
        return self.arr(np.array(list(xs) + [0], np.uint64), np.uint64)


def where_maps(sources, head, n_hay):
    """sources: list of (recs REC[count..], count, npos, pos, stride, term, grouped); -> per source a u32[n] map (None for a plain one), filled the
    way the device fills them"""
    k = _Keep()
    n = len(head)
    maps = [np.full(max(n, 1), 0xABABABAB, np.uint32) if s[6] else None for s in sources]
    recs = k.ptrs(k.arr(s[0], REC) for s in sources)
    counts = k.arr([s[1] for s in sources], np.uint32)
    where = k.ptrs(0 if m is None else m.ctypes.data for m in maps)
    lib().gh_where(len(sources), recs, counts, where, k.arr(head, REC), n, n_hay)
    return [None if m is None else m[:n] for m in maps]


def union(sources, maps, head, head_count=None, max_records=None, U=None):
    """-> (combined REC[n], combined count, npos_u u32[n], pos_u u32[n, U], carrier_of u32[n, P])"""
    k = _Keep()
    P = len(sources)
    n_head = len(head) if head_count is None else head_count
    cap = n_head if max_records is None else max_records
    n = min(n_head, cap)
    recs = k.ptrs(k.arr(s[0], REC) for s in sources)
    npos = k.ptrs(k.arr(s[2], np.uint32) for s in sources)
    pos = k.ptrs(k.arr(s[3], np.uint32) for s in sources)
    counts = k.arr([s[1] for s in sources], np.uint32)
    strides = k.arr([s[4] for s in sources], np.uint32)
    terms = k.arr([s[5] for s in sources], np.uint32)
    where = k.ptrs(0 if m is None else k.arr(m, np.uint32) for m in maps)
    out = np.zeros(max(n, 1), REC)
    out_count = np.zeros(1, np.uint32)
    npos_u = np.zeros(max(n, 1), np.uint32)
    pos_u = np.full(max(n * U, 1), 0xFFFFFFFF, np.uint32)
    carrier_of = np.full(max(n * P, 1), 0xEEEEEEEE, np.uint32)
    walked = lib().gh_union(P, recs, counts, npos, pos, strides, where, terms, k.arr(head, REC), n_head, cap, U, out.ctypes.data, out_count.ctypes.data, npos_u.ctypes.data,
                            pos_u.ctypes.data, carrier_of.ctypes.data)
    assert walked == n
    return out[:n], int(out_count[0]), npos_u[:n], (pos_u[: n * U].reshape(n, U) if U else np.zeros((n, 0), np.uint32)), carrier_of[: n * P].reshape(n, P)


def check(head, head_count, comb, comb_count):
    head = np.ascontiguousarray(head, dtype=REC)
    comb = np.ascontiguousarray(comb, dtype=REC)
    n = min(len(head), len(comb))
    h = head if n else np.zeros(1, REC)
    c = comb if n else np.zeros(1, REC)
    return int(lib().gh_check(h.ctypes.data, head_count, c.ctypes.data, comb_count, n))
