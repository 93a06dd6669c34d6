"""TEST INFRASTRUCTURE: builds tests/kernel_host/libsig_repeat_host.so - the repeat signature of frizbee_amd/csrc/sig_filter.h compiled for
the host with ROCm's clang++ through the stand-in <hip/hip_runtime.h> - and loads it with ctypes; also the plain Python count the host and
GPU tests compare with.  Never imported by the product."""
import ctypes as C
import os
import subprocess

import numpy as np

from sig_host_lib import py_sig_bit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "kernel_host")
CSRC = os.path.join(ROOT, "frizbee_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def available():
    return os.path.exists(CLANG)


def build():
    so = os.path.join(HERE, "libsig_repeat_host.so")
    srcs = [os.path.join(HERE, "sig_repeat_host.cpp"), os.path.join(HERE, "shim", "hip", "hip_runtime.h"), os.path.join(CSRC, "sig_filter.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + os.path.join(HERE, "shim"), "-I" + CSRC, "-Wall", "-Werror",
                               "-o", so, os.path.join(HERE, "sig_repeat_host.cpp")])
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build())
        for name in ("sr_sig_of_bytes", "sr_sig2_of_bytes", "sr_needle_sig", "sr_needle_sig2"):
            getattr(l, name).argtypes = [C.c_char_p, C.c_size_t]
            getattr(l, name).restype = C.c_uint32
        l.sr_sig2_of_words.argtypes = [C.c_void_p, C.c_size_t]
        l.sr_sig2_of_words.restype = C.c_uint32
        l.sr_passes.argtypes = [C.c_uint32] * 4
        l.sr_transpose.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        l.sr_transpose.restype = None
        l.sr_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
        l.sr_candidates.restype = C.c_uint64
        _lib = l
    return _lib


def py_sig2(bs):
    """sig_filter.h restated: bit b set <=> at least two non-zero bytes of `bs` have signature bit b"""
    count = [0] * 32
    for b in bytes(bs):
        if b:
            count[py_sig_bit(b)] += 1
    return sum(1 << b for b in range(32) if count[b] >= 2)


def want_sig2(hs):
    return np.array([py_sig2(h) for h in hs], np.uint32)
