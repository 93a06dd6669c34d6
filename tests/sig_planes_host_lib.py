"""TEST INFRASTRUCTURE: builds tests/kernel_host/libsig_planes_host.so - the bit-plane layout of frizbee_amd/csrc/sig_filter.h compiled for
the host with ROCm's clang++ through the stand-in <hip/hip_runtime.h> - and loads it with ctypes; also the plain numpy transposition the
host and GPU tests compare with.  Never imported by the product."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "kernel_host")
CSRC = os.path.join(ROOT, "frizbee_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
TILE, WORDS = 1024, 16


def available():
    return os.path.exists(CLANG)


def build():
    so = os.path.join(HERE, "libsig_planes_host.so")
    srcs = [os.path.join(HERE, "sig_planes_host.cpp"), os.path.join(HERE, "shim", "hip", "hip_runtime.h"), os.path.join(CSRC, "sig_filter.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + os.path.join(HERE, "shim"), "-I" + CSRC, "-Wall", "-Werror",
                               "-o", so, os.path.join(HERE, "sig_planes_host.cpp")])
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build())
        for name, args in (("sp_tiles", [C.c_uint64]), ("sp_words", [C.c_uint64]), ("sp_index", [C.c_uint64, C.c_uint32, C.c_uint32]),
                           ("sp_valid", [C.c_uint64, C.c_uint32, C.c_uint64]), ("sp_candidates", [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32])):
            getattr(l, name).argtypes = args
            getattr(l, name).restype = C.c_uint64
        l.sp_transpose.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        l.sp_transpose.restype = None
        l.sp_passes.argtypes = [C.c_uint32, C.c_uint32]
        l.sp_needle_sig.argtypes = [C.c_char_p, C.c_size_t]
        l.sp_needle_sig.restype = C.c_uint32
        l.sp_batch_tiles.restype = C.c_uint32
        _lib = l
    return _lib


def py_planes(sig):
    """the layout restated: planes[tile][bit][word] bit i = bit `bit` of sig[1024 tile + 64 word + i], zero at and beyond len(sig)"""
    sig = np.asarray(sig, dtype=np.uint32)
    n = len(sig)
    tiles = (n + TILE - 1) // TILE
    padded = np.zeros(tiles * TILE, np.uint32)
    padded[:n] = sig
    bits = (padded.reshape(tiles, WORDS, 64, 1) >> np.arange(32, dtype=np.uint32)) & 1       # [tile][word][i][bit]
    words = (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64).reshape(1, 1, 64, 1)).sum(axis=2, dtype=np.uint64)  # [tile][word][bit]
    return np.ascontiguousarray(words.transpose(0, 2, 1)).reshape(-1)
