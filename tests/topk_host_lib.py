"""TEST INFRASTRUCTURE: builds tests/kernel_host/libtopk_host.so - frizbee_amd/csrc/topk_select.h, the decisions of the top-`limit`
selection stage, compiled for the host with ROCm's clang++ through the stand-in <hip/hip_runtime.h> - and loads it with ctypes, so that
the CPU suite can fuzz what the GPU kernels call.  Never imported by the product."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "kernel_host")
CSRC = os.path.join(ROOT, "frizbee_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
NOT_KEPT = 0xFFFFFFFF


def available():
    return os.path.exists(CLANG)


def build():
    so = os.path.join(HERE, "libtopk_host.so")
    srcs = [os.path.join(HERE, "topk_host.cpp"), os.path.join(HERE, "shim", "hip", "hip_runtime.h"), os.path.join(CSRC, "topk_select.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + os.path.join(HERE, "shim"), "-I" + CSRC, "-Wall", "-Werror",
                               "-o", so, os.path.join(HERE, "topk_host.cpp")])
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.th_select.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _lib.th_select.restype = C.c_uint32
    return _lib


def select(scores, limit, by_score=True, desc=False, one_pass=False):
    """scores: u16 array in record order -> (dest: u32 array, position in the selected list or NOT_KEPT; cut: dict; kept: int)"""
    scores = np.ascontiguousarray(scores, dtype=np.uint16)
    n = len(scores)
    dest = np.zeros(max(n, 1), np.uint32)
    cut = np.zeros(6, np.uint32)
    buf = scores if n else np.zeros(1, np.uint16)
    kept = lib().th_select(buf.ctypes.data, n, min(int(limit), 0xFFFFFFFF), int(by_score), int(desc), int(one_pass), dest.ctypes.data, cut.ctypes.data)
    names = ("T", "gt", "ties", "quota", "lo", "keep_all")
    return dest[:n], dict(zip(names, (int(x) for x in cut))), int(kept)
