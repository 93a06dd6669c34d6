"""TEST INFRASTRUCTURE: builds tests/kernel_host/libunion_host.so - frizbee_amd/csrc/indices_union.h, the union step of the fused
multi-pattern top + matched-positions query, compiled for the host with ROCm's clang++ through the stand-in <hip/hip_runtime.h> - and loads
it with ctypes, so that the CPU suite can fuzz what k_multi_union calls.  Never imported by the product."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "kernel_host")
CSRC = os.path.join(ROOT, "frizbee_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
REC = np.dtype([("index", "<u4"), ("score", "<u2"), ("exact", "u1"), ("pad", "u1")])
BAD_COUNT, BAD_RECORD = 1, 2


def available():
    return os.path.exists(CLANG)


def build():
    so = os.path.join(HERE, "libunion_host.so")
    srcs = [os.path.join(HERE, "union_host.cpp"), os.path.join(HERE, "shim", "hip", "hip_runtime.h"), os.path.join(CSRC, "indices_union.h"), os.path.join(CSRC, "indices_pack.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + os.path.join(HERE, "shim"), "-I" + CSRC, "-Wall", "-Werror",
                               "-o", so, os.path.join(HERE, "union_host.cpp")])
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.uh_by_value.restype = C.c_uint32
        _lib.uh_union.argtypes = [C.c_uint32] + [C.c_void_p] * 6 + [C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4
        _lib.uh_union.restype = C.c_uint32
        _lib.uh_check.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
        _lib.uh_check.restype = C.c_uint32
    return _lib


def union(sources, head, head_count=None, max_records=None, U=None):
    """sources: list of (recs REC[>= n], count, npos u32[>= n], pos u32[>= n * stride], stride); head: REC[n].
    -> (combined REC[n], combined count, npos_u u32[n], pos_u u32[n, U])"""
    P = len(sources)
    n_head = len(head) if head_count is None else head_count
    cap = n_head if max_records is None else max_records
    n = min(n_head, cap)
    U = sum(s[4] for s in sources) if U is None else U
    keep = []

    def arr(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        if a.size == 0:
            a = np.zeros(1, dt)
        keep.append(a)
        return a.ctypes.data

    ptrs = lambda xs: arr(np.array(xs + [0], np.uint64), np.uint64)  # noqa: E731
    recs = ptrs([arr(s[0], REC) for s in sources])
    npos = ptrs([arr(s[2], np.uint32) for s in sources])
    pos = ptrs([arr(s[3], np.uint32) for s in sources])
    counts = arr([s[1] for s in sources], np.uint32)
    strides = arr([s[4] for s in sources], np.uint32)
    out = np.zeros(max(n, 1), REC)
    out_count = np.zeros(1, np.uint32)
    npos_u = np.zeros(max(n, 1), np.uint32)
    pos_u = np.full(max(n * U, 1), 0xFFFFFFFF, np.uint32)
    walked = lib().uh_union(P, recs, counts, npos, pos, strides, arr(head, REC), n_head, cap, U, out.ctypes.data, out_count.ctypes.data, npos_u.ctypes.data, pos_u.ctypes.data)
    assert walked == n
    return out[:n], int(out_count[0]), npos_u[:n], pos_u[: n * U].reshape(n, U) if U else np.zeros((n, 0), np.uint32)


def check(head, head_count, comb, comb_count):
    head = np.ascontiguousarray(head, dtype=REC)
    comb = np.ascontiguousarray(comb, dtype=REC)
    n = min(len(head), len(comb))
    h = head if n else np.zeros(1, REC)
    c = comb if n else np.zeros(1, REC)
    return int(lib().uh_check(h.ctypes.data, head_count, c.ctypes.data, comb_count, n))
