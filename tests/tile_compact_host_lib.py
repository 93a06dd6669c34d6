"""TEST INFRASTRUCTURE: builds tests/kernel_host/libtile_compact_host.so - frizbee_amd/csrc/tile_compact.h, the tile scheme's plain
functions, compiled for the host with ROCm's clang++ - and loads it with ctypes; build_sanitized() builds the same source as a stand-alone
program under AddressSanitizer + UBSan (its own main, never loaded into Python).  Never imported by the product."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "kernel_host")
CSRC = os.path.join(ROOT, "frizbee_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(HERE, "tile_compact_host.cpp")


def available():
    return os.path.exists(CLANG)


def _stale(out):
    srcs = [SRC, os.path.join(CSRC, "tile_compact.h")]
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)


def build():
    so = os.path.join(HERE, "libtile_compact_host.so")
    if _stale(so):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + CSRC, "-Wall", "-Werror", "-o", so, SRC])
    return so


def build_sanitized():
    exe = os.path.join(HERE, "tile_compact_host_san")
    if _stale(exe):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-DTCH_MAIN",
                               "-I" + CSRC, "-Wall", "-Werror", "-o", exe, SRC])
    return exe


_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build())
        u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
        l.tch_tile.restype = u32
        l.tch_tiles_per_run.argtypes = [u32, u32]
        l.tch_tiles_per_run.restype = u32
        l.tch_run.argtypes = [u32, u32, u32, C.POINTER(u32)]
        l.tch_run.restype = None
        l.tch_grid.argtypes = [u64, C.c_int]
        l.tch_grid.restype = C.c_int
        l.tch_rank64.argtypes = [vp, vp, vp, u32, vp]
        l.tch_rank64.restype = None
        l.tch_rank32.argtypes = [vp, vp, vp, u32, vp]
        l.tch_rank32.restype = None
        l.tch_walk.argtypes = [vp, u32, u32, u32, vp, C.c_int, vp, u32, vp]
        l.tch_walk.restype = None
        _lib = l
    return _lib
