"""TEST INFRASTRUCTURE: builds tests/kernel_host/libitems_host.so - frizbee_amd/csrc/items_filter.h, the per-item decision of the item-list
filter for large candidate sets, compiled for the host with ROCm's clang++ through the stand-in <hip/hip_runtime.h> - and loads it with
ctypes.  Never imported by the product."""
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
    so = os.path.join(HERE, "libitems_host.so")
    srcs = [os.path.join(HERE, "items_filter_host.cpp"), os.path.join(HERE, "shim", "hip", "hip_runtime.h"), os.path.join(CSRC, "items_filter.h"), os.path.join(CSRC, "sig_filter.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        tmp = so + ".tmp.%d" % os.getpid()
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + os.path.join(HERE, "shim"), "-I" + CSRC, "-Wall", "-Werror",
                               "-o", tmp, os.path.join(HERE, "items_filter_host.cpp")])
        os.replace(tmp, so)
    return so


_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build())
        u32 = C.c_uint32
        l.ifh_wants_row.argtypes = [C.c_int, u32, u32, u32, u32]
        l.ifh_vecs.argtypes = [u32]
        l.ifh_vecs.restype = u32
        l.ifh_vec_bytes.argtypes = [u32, u32]
        l.ifh_vec_bytes.restype = u32
        for name in ("ifh_sig_of_bytes", "ifh_needle_sig"):
            getattr(l, name).argtypes = [C.c_char_p, C.c_size_t]
            getattr(l, name).restype = u32
        l.ifh_sig_passes.argtypes = [u32, u32]
        l.ifh_chain_vec.argtypes = [u32, C.POINTER(u32), u32, C.c_char_p]
        l.ifh_chain_vec.restype = u32
        l.ifh_decide.argtypes = [C.c_int, u32, u32, C.c_char_p, u32, u32, u32, C.c_char_p]
        _lib = l
    return _lib


def subsequence_dfa(rows_c, rows_f):
    """the ordered-subsequence automaton as the library builds it (host.hip, build_filter_tables): state s = rows matched so far, byte b takes
    it to s + 1 iff b is row s' byte or its case flip; the last state is absorbing.  (rows + 1) x 256 bytes."""
    n = len(rows_c)
    t = bytearray((n + 1) * 256)
    for s in range(n + 1):
        for b in range(256):
            t[s * 256 + b] = s + 1 if s < n and b in (rows_c[s], rows_f[s]) else s
    return bytes(t)
