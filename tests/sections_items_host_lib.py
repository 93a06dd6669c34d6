"""TEST INFRASTRUCTURE: builds tests/kernel_host/libsections_items_host.so - the placement arithmetic of frizbee_amd/csrc/sections.h (the
sectioned stage's slabs -> one dense head), compiled for the host with ROCm's clang++ - and loads it with ctypes; build_sanitized() builds the
same source with its own main under AddressSanitizer + UBSan as a stand-alone program.  Never imported by the product."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "kernel_host")
CSRC = os.path.join(ROOT, "frizbee_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(HERE, "sections_items_host.cpp")


def available():
    return os.path.exists(CLANG)


def _stale(target):
    srcs = [SRC] + [os.path.join(CSRC, h) for h in ("sections.h", "scope.h", "topk_select.h")]
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in srcs)


def build():
    so = os.path.join(HERE, "libsections_items_host.so")
    if _stale(so):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + CSRC, "-Wall", "-Werror", "-o", so, SRC])
    return so


def build_sanitized():
    exe = os.path.join(HERE, "sections_items_host_san")
    if _stale(exe):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-DSIH_MAIN",
                               "-I" + CSRC, "-Wall", "-Werror", "-o", exe, SRC])
    return exe


_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build())
        l.sih_no_slot.restype = C.c_uint32
        l.sih_items.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.sih_items.restype = C.c_uint32
        _lib = l
    return _lib
