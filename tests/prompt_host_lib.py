"""TEST INFRASTRUCTURE: builds tests/kernel_host/libprompt_host.so - frizbee_amd/csrc/prompt_records.h, the per-item rule of the empty
prompt, compiled for the host with ROCm's clang++ through the stand-in <hip/hip_runtime.h> - and loads it with ctypes.  Never imported by
the product."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "kernel_host")
CSRC = os.path.join(ROOT, "frizbee_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def available():
    return os.path.exists(CLANG)


def build():
    so = os.path.join(HERE, "libprompt_host.so")
    srcs = [os.path.join(HERE, "prompt_host.cpp"), os.path.join(HERE, "shim", "hip", "hip_runtime.h")] + [os.path.join(CSRC, h) for h in
                                                                                                           ("prompt_records.h", "scope.h", "score_bias.h", "tile_compact.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + os.path.join(HERE, "shim"), "-I" + CSRC, "-Wall", "-Werror",
                               "-o", so, os.path.join(HERE, "prompt_host.cpp")])
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build())
        l.ph_tile.restype = C.c_uint32
        l.ph_records.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p]
        l.ph_records.restype = None
        l.ph_compact.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                 C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        l.ph_compact.restype = None
        _lib = l
    return _lib
