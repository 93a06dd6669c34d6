"""TEST INFRASTRUCTURE: builds tests/kernel_host/libtrace_host.so - frizbee_amd/csrc/trace_walk.h, the walk back through the score /
match matrices that lane 0 of the traced scorer runs, compiled for the host with ROCm's clang++ through the stand-in
<hip/hip_runtime.h> - and loads it with ctypes, so that the CPU suite can hold the walk the GPU kernel calls to the oracle's.  Never
imported by the product."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "kernel_host")
CSRC = os.path.join(ROOT, "frizbee_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
POISON = 0xDEADBEEF  # what every cell the scorer does not write holds: the walk must never read one


def available():
    return os.path.exists(CLANG)


def build():
    so = os.path.join(HERE, "libtrace_host.so")
    srcs = [os.path.join(HERE, "trace_host.cpp"), os.path.join(HERE, "shim", "hip", "hip_runtime.h"), os.path.join(CSRC, "trace_walk.h"), os.path.join(CSRC, "fzb_internal.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + os.path.join(HERE, "shim"), "-I" + CSRC, "-Wall", "-Werror",
                               "-o", so, os.path.join(HERE, "trace_host.cpp")])
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.tw_walk.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_void_p, C.c_uint32]
        _lib.tw_walk.restype = C.c_int
    return _lib


def trace_w():
    return lib().tw_trace_w()


def pack_cells(matrices, rows, lanes):
    """The matrices of sw_second_transcription.score_haystack[_unicode] ({(row, chunk): [lanes]}, chunk 0 = the zero chunk) in the layout
    k2c_generic<.., TRACE = true> writes: (rows + 1) x TRACE_W dwords, score | match bit << 16, chunk c at columns c * lanes ...; what
    the kernel does not write (row 0, the zero chunk, the columns past the last chunk) is poisoned.  -> (cells, chunks after the zero one)"""
    S, MM, chunks = matrices["S"], matrices["MM"], matrices["chunks"]
    W = trace_w()
    cells = np.full((rows + 1, W), POISON, np.uint32)
    for r in range(1, rows + 1):
        for c in range(1, chunks):
            s = np.asarray(S[(r, c)], np.uint32)
            mm = np.asarray(MM[(r, c)], np.uint32)
            cells[r, c * lanes : (c + 1) * lanes] = s | ((mm != 0).astype(np.uint32) << 16)
    return cells, chunks - 1


def walk(cells, nchunks, rows, lanes, unicode, score, max_typos, window, start_pos, ulen=None, stride=None, guard=8, sentinel=0xA5A5A5A5):
    """first column of the last row holding `score`, then trace_walk.h's walk -> (positions in walk order, the `guard` words behind
    the `stride` the walk may fill - still `sentinel` unless it wrote past the end)"""
    window = bytes(window)
    stride = len(window) if stride is None else stride
    posv = np.full(stride + guard, sentinel, np.uint32)
    ul = bytes(ulen) if ulen is not None else b"\0"
    n = lib().tw_walk(cells.ctypes.data, rows, nchunks, lanes, int(unicode), score, -1 if max_typos is None else max_typos, window, len(window), start_pos, ul,
                      posv.ctypes.data, stride)
    if n < 0:
        raise RuntimeError({-1: "no column of the last row holds the score", -2: "unsupported lane count"}[n])
    assert n <= stride
    assert (posv[n:stride] == sentinel).all()
    return posv[:n].tolist(), posv[stride:].tolist()
