"""TEST INFRASTRUCTURE: builds tests/kernel_host/libanyof_host.so - frizbee_amd/csrc/anyof.h, the arithmetic of an any-of group, and the
accumulate / flag / compact loops over it, compiled for the host with ROCm's clang++ - and loads it with ctypes; build_sanitized() builds the
same source as a stand-alone program under AddressSanitizer + UBSan (its own main, never loaded into Python).  Never imported by the product."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "kernel_host")
CSRC = os.path.join(ROOT, "frizbee_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(HERE, "anyof_host.cpp")


def available():
    return os.path.exists(CLANG)


def _stale(out):
    srcs = [SRC, os.path.join(CSRC, "anyof.h"), os.path.join(CSRC, "tile_compact.h")]
    return not os.path.exists(out) or any(os.path.getmtime(s) > os.path.getmtime(out) for s in srcs)


def build():
    so = os.path.join(HERE, "libanyof_host.so")
    if _stale(so):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + CSRC, "-Wall", "-Werror", "-o", so, SRC])
    return so


def build_sanitized():
    exe = os.path.join(HERE, "anyof_host_san")
    if _stale(exe):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-DAOH_MAIN",
                               "-I" + CSRC, "-Wall", "-Werror", "-o", exe, SRC])
    return exe


_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build())
        u32, vp = C.c_uint32, C.c_void_p
        l.aoh_alts_max.restype = u32
        l.aoh_pack.argtypes = [vp, vp, u32, vp]
        l.aoh_combine.argtypes = [vp, vp, u32, vp]
        l.aoh_unpack.argtypes = [vp, u32, vp, vp, vp]
        l.aoh_join.argtypes = [vp, vp, vp, u32, vp, vp]
        l.aoh_find.argtypes = [vp, u32, vp, u32, vp]
        for f in (l.aoh_pack, l.aoh_combine, l.aoh_unpack, l.aoh_join, l.aoh_find):
            f.restype = None
        l.aoh_group.argtypes = [vp, vp, u32, u32, u32, vp, vp, u32, vp]
        l.aoh_group.restype = u32
        _lib = l
    return _lib
