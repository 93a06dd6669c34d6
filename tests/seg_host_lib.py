"""TEST INFRASTRUCTURE: builds tests/kernel_host/libseg_host.so - frizbee_amd/csrc/seg_list.h, the arithmetic of the segmented survivor
list, compiled for the host with ROCm's clang++ through the stand-in <hip/hip_runtime.h> - and loads it with ctypes.  Never imported
by the product."""
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
    so = os.path.join(HERE, "libseg_host.so")
    srcs = [os.path.join(HERE, "seg_host.cpp"), os.path.join(HERE, "shim", "hip", "hip_runtime.h"), os.path.join(CSRC, "seg_list.h"), os.path.join(CSRC, "tile_compact.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + os.path.join(HERE, "shim"), "-I" + CSRC, "-Wall", "-Werror",
                               "-o", so, os.path.join(HERE, "seg_host.cpp")])
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build())
        u32, p32 = C.c_uint32, C.POINTER(C.c_uint32)
        l.sg_max.restype = u32
        l.sg_tiles_per_run.argtypes = [u32, u32]
        l.sg_tiles_per_run.restype = u32
        l.sg_run.argtypes = [u32, u32, u32, p32]
        l.sg_run.restype = None
        l.sg_top.argtypes = [u32]
        l.sg_top.restype = u32
        l.sg_map_all.argtypes = [p32, u32, p32, p32, p32]
        l.sg_map_all.restype = u32
        l.sg_rank_tile.argtypes = [p32, p32]
        l.sg_rank_tile.restype = u32
        _lib = l
    return _lib
