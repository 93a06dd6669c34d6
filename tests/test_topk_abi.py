"""The boundary of the top-`limit` queries without a GPU: the new symbols are exported and declared, NULL arguments are refused before
anything touches a device, scoring without a device fails loudly, and the C++ host side compiles with a call to `match_list_top`."""
import ctypes as C
import os
import re
import subprocess

import pytest

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_facade_topk")
TOP = ("fzb_match_list_top", "fzb_match_list_top_device", "fzb_multi_match_list_top", "fzb_match_list_top_sharded", "fzb_multi_match_list_top_sharded")
FZB_ERR_INVALID = 1


def build_facade():
    src = EXE + ".cpp"
    hdrs = [os.path.join(ROOT, "include", h) for h in ("frizbee_hip.hpp", "frizbee_hip.h")]
    lib = os.path.join(ROOT, "frizbee_amd", "libfrizbee_hip.so")
    if not os.path.exists(EXE) or any(os.path.getmtime(f) > os.path.getmtime(EXE) for f in [src, lib] + hdrs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", EXE, "-L", os.path.join(ROOT, "frizbee_amd"),
                               "-lfrizbee_hip", "-Wl,-rpath," + os.path.join(ROOT, "frizbee_amd")])
    return EXE


def test_top_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "frizbee_hip.h")).read()
    declared = set(re.findall(r"\b(fzb_[a-z0-9_]+)\s*\(", header))
    for name in TOP:
        assert name in declared and name in F.SYMBOLS
        fn = getattr(F.lib(), name)
        assert fn.argtypes is not None and len(fn.argtypes) in (6, 7)
    # the header says what the result is a prefix of
    assert "src/matcher/mod.rs:215-221" in header[header.index("TOP-`limit` QUERIES"):header.index("int fzb_match_list_top(")]


def test_null_arguments_are_refused():
    l = F.lib()
    m = F.Matcher("abc")       # a matcher needs no device
    mm = F.MultiMatcher(F.parse_query("abc !d"))
    out, n, found = C.c_void_p(), C.c_size_t(), C.c_uint64()
    fake = C.c_void_p(64)  # never dereferenced: the NULL checks come first
    null = C.c_void_p(None)
    assert l.fzb_match_list_top(null, fake, 1, C.byref(out), C.byref(n), C.byref(found)) == FZB_ERR_INVALID
    assert l.fzb_match_list_top(m.h, null, 1, C.byref(out), C.byref(n), C.byref(found)) == FZB_ERR_INVALID
    assert l.fzb_match_list_top(m.h, null, 1, None, C.byref(n), None) == FZB_ERR_INVALID
    assert l.fzb_match_list_top(m.h, null, 1, C.byref(out), None, None) == FZB_ERR_INVALID
    assert b"null" in l.fzb_last_error()
    assert l.fzb_match_list_top_device(null, fake, 1, fake, 1, fake, None) == FZB_ERR_INVALID
    assert l.fzb_match_list_top_device(m.h, null, 1, fake, 1, fake, None) == FZB_ERR_INVALID
    assert l.fzb_multi_match_list_top(null, fake, 1, C.byref(out), C.byref(n), None) == FZB_ERR_INVALID
    assert l.fzb_multi_match_list_top(mm.h, null, 1, C.byref(out), C.byref(n), None) == FZB_ERR_INVALID
    assert l.fzb_multi_match_list_top(mm.h, null, 1, None, None, None) == FZB_ERR_INVALID
    assert l.fzb_match_list_top_sharded(null, fake, 1, C.byref(out), C.byref(n), None) == FZB_ERR_INVALID
    assert l.fzb_match_list_top_sharded(m.h, null, 1, C.byref(out), C.byref(n), None) == FZB_ERR_INVALID
    assert l.fzb_multi_match_list_top_sharded(null, fake, 1, C.byref(out), C.byref(n), None) == FZB_ERR_INVALID
    assert l.fzb_multi_match_list_top_sharded(mm.h, null, 1, C.byref(out), C.byref(n), None) == FZB_ERR_INVALID
    assert out.value is None and n.value == 0


def test_top_queries_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(F.FrizbeeError):
        F.Matcher("abc").match_list_top(["abc"], 1)
    with pytest.raises(F.FrizbeeError):
        F.MultiMatcher(F.parse_query("abc !d")).match_list_top(["abc"], 1)


def test_cpp_facade_compiles_with_match_list_top():
    r = subprocess.run([build_facade()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_facade_topk: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_match_list_top_through_the_cpp_facade():
    r = subprocess.run([build_facade(), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_facade_topk: ok" in r.stdout, r.stdout + r.stderr
