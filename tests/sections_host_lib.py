"""TEST INFRASTRUCTURE: builds tests/kernel_host/libsections_host.so - frizbee_amd/csrc/sections.h, the decisions of the sectioned
top-`limit` stage, compiled for the host with ROCm's clang++ - and loads it with ctypes; plus the numpy model of a sectioned call that the
host walk, the GPU tests and tools/bench_sections.py are held against.  Never imported by the product."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "kernel_host")
CSRC = os.path.join(ROOT, "frizbee_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
REC = np.dtype([("index", "<u4"), ("score", "<u2"), ("exact", "u1"), ("_pad", "u1")])


def available():
    return os.path.exists(CLANG)


def build():
    so = os.path.join(HERE, "libsections_host.so")
    srcs = [os.path.join(HERE, "sections_host.cpp"), os.path.join(HERE, "shim", "hip", "hip_runtime.h")] + [os.path.join(CSRC, h) for h in ("sections.h", "scope.h", "topk_select.h", "tile_compact.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + os.path.join(HERE, "shim"), "-I" + CSRC, "-Wall", "-Werror",
                               "-o", so, os.path.join(HERE, "sections_host.cpp")])
    return so


def build_sanitized():
    """the same source with its own main (SEC_MAIN), under AddressSanitizer + UBSan: a program of its own, never loaded into Python"""
    exe = os.path.join(HERE, "sections_host_san")
    srcs = [os.path.join(HERE, "sections_host.cpp")] + [os.path.join(CSRC, h) for h in ("sections.h", "scope.h", "topk_select.h", "tile_compact.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-DSEC_MAIN",
                               "-I" + os.path.join(HERE, "shim"), "-I" + CSRC, "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "sections_host.cpp")])
    return exe


_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(build())
        for name in ("sec_sections_max", "sec_limit_max", "sec_tile", "sec_state_words"):
            getattr(l, name).restype = C.c_uint32
        l.sec_masks.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        l.sec_masks.restype = None
        l.sec_ranks.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
        l.sec_ranks.restype = None
        l.sec_walk.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                               C.c_void_p]
        l.sec_walk.restype = None
        _lib = l
    return _lib


def _split(sections):
    req = np.ascontiguousarray([s[0] for s in sections], dtype=np.uint16)
    exc = np.ascontiguousarray([s[1] for s in sections], dtype=np.uint16)
    return req, exc


def masks(tags, sections):
    tags = np.ascontiguousarray(tags, dtype=np.uint16)
    req, exc = _split(sections)
    out = np.zeros(len(tags), np.uint32)
    lib().sec_masks(tags.ctypes.data, len(tags), req.ctypes.data, exc.ctypes.data, len(sections), out.ctypes.data)
    return out


def ranks(slab, by_score, desc):
    slab = np.ascontiguousarray(slab, dtype=REC)
    out = np.zeros(len(slab), np.uint32)
    lib().sec_ranks(slab.ctypes.data, len(slab), int(by_score), int(desc), out.ctypes.data)
    return out


def walk(recs, tags, sections, limit, by_score, desc, one_pass):
    """the host walk of the stage -> ([head per section], [found per section], cuts[S, 6])"""
    recs = np.ascontiguousarray(recs, dtype=REC)
    S = len(sections)
    req, exc = _split(sections)
    out = np.zeros(max(S * limit, 1), REC)
    counts = np.zeros(max(2 * S, 1), np.uint32)
    cuts = np.zeros((max(S, 1), 6), np.uint32)
    if tags is not None:
        tags = np.ascontiguousarray(tags, dtype=np.uint16)
    lib().sec_walk(recs.ctypes.data, len(recs), tags.ctypes.data if tags is not None else None, len(tags) if tags is not None else 0, req.ctypes.data, exc.ctypes.data, S, limit,
                   int(by_score), int(desc), int(one_pass), out.ctypes.data, counts.ctypes.data, cuts.ctypes.data)
    heads = [out[s * limit:s * limit + int(counts[2 * s])].copy() for s in range(S)]
    return heads, [int(counts[2 * s + 1]) for s in range(S)], cuts


# ---- the numpy model: what a sectioned call returns, by the definition ------------------------------------------------------------------
def member(tags, require, exclude):
    tags = np.asarray(tags, dtype=np.uint32)
    return ((tags & require) == require) & ((tags & exclude) == 0)


def model_head(recs, rec_tags, require, exclude, limit, by_score, desc):
    """recs: index-ordered records; rec_tags: the tag of each record's haystack.  `match_list`'s order over the section's records - reverse
    for the *Desc strategies, then the stable sort by descending score - cut to `limit`; found = the section's records."""
    sel = recs[member(rec_tags, require, exclude)]
    if desc:
        sel = sel[::-1]
    if by_score:
        sel = sel[np.argsort(-sel["score"].astype(np.int64), kind="stable")]
    return sel[:limit].copy(), len(sel)


def model(recs, rec_tags, sections, limit, by_score, desc):
    out = [model_head(recs, rec_tags, r, e, limit, by_score, desc) for r, e in sections]
    return [h for h, _ in out], [f for _, f in out]
