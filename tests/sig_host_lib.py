"""TEST INFRASTRUCTURE: builds tests/kernel_host/libsig_host.so - frizbee_amd/csrc/sig_filter.h, the letter signatures of the streaming
filter, compiled for the host with ROCm's clang++ through the stand-in <hip/hip_runtime.h> - and loads it with ctypes.  Never imported
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
    so = os.path.join(HERE, "libsig_host.so")
    srcs = [os.path.join(HERE, "sig_host.cpp"), os.path.join(HERE, "shim", "hip", "hip_runtime.h"), os.path.join(CSRC, "sig_filter.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + os.path.join(HERE, "shim"), "-I" + CSRC, "-Wall", "-Werror",
                               "-o", so, os.path.join(HERE, "sig_host.cpp")])
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build())
        for name in ("sh_sig_bit", "sh_sig_of_byte", "sh_sig_of_word"):
            getattr(l, name).argtypes = [C.c_uint32]
            getattr(l, name).restype = C.c_uint32
        for name in ("sh_sig_of_bytes", "sh_needle_sig"):
            getattr(l, name).argtypes = [C.c_char_p, C.c_size_t]
            getattr(l, name).restype = C.c_uint32
        l.sh_eligible.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int]
        l.sh_gather_max.restype = C.c_uint32
        _lib = l
    return _lib


def py_sig_bit(b):
    """sig_filter.h restated: letters of either case -> 0..25, every other non-zero byte -> 26 + b % 6"""
    if ord("a") <= b <= ord("z"):
        return b - ord("a")
    if ord("A") <= b <= ord("Z"):
        return b - ord("A")
    return 26 + b % 6


def py_sig(bs):
    s = 0
    for b in bytes(bs):
        if b:
            s |= 1 << py_sig_bit(b)
    return s
