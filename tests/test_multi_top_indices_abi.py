"""The boundary of the device-fused multi-pattern top + matched-positions query without a GPU: the three new symbols are exported, declared
(behind the host composition's declaration) and listed, NULL arguments are refused before anything touches a device, the queries fail loudly
without a device, the mirrors name the calls, and the C++ host side compiles with them."""
import ctypes as C
import os
import re
import subprocess

import pytest

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_facade_multi_top_indices")
NEW = {"fzb_multi_match_list_top_indices_device": 9, "fzb_multi_match_list_top_indices_fused": 7, "fzb_multi_matcher_reserve_top_indices": 4}
FZB_ERR_INVALID = 1


def build_facade():
    src = EXE + ".cpp"
    hdrs = [os.path.join(ROOT, "include", h) for h in ("frizbee_hip.hpp", "frizbee_hip.h")]
    lib = os.path.join(ROOT, "frizbee_amd", "libfrizbee_hip.so")
    if not os.path.exists(EXE) or any(os.path.getmtime(f) > os.path.getmtime(EXE) for f in [src, lib] + hdrs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", EXE, "-L", os.path.join(ROOT, "frizbee_amd"),
                               "-lfrizbee_hip", "-Wl,-rpath," + os.path.join(ROOT, "frizbee_amd")])
    return EXE


def test_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "frizbee_hip.h")).read()
    declared = set(re.findall(r"\b(fzb_[a-z0-9_]+)\s*\(", header))
    composed = header.index("int fzb_multi_match_list_top_indices(")
    for name, nargs in NEW.items():
        assert name in declared and name in F.SYMBOLS
        assert header.index("int " + name + "(") > composed  # the new entry points come after the host composition's declaration
        fn = getattr(F.lib(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    # the header says what the union is, which patterns are traced and what the positions need room for
    block = header[composed:header.index("int fzb_multi_match_list_top_indices_device(")]
    assert "src/matcher/multi.rs:56-82" in block and "NON-NEGATED" in block and "no host synchronisation" in block
    hpp = open(os.path.join(ROOT, "include", "frizbee_hip.hpp")).read()
    rs = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    for name in NEW:
        assert name in hpp and ("fn " + name + "(") in rs, name
    multi = rs[rs.index("impl HipMultiMatcher"):rs.index("impl Drop for HipMultiMatcher")]
    assert "fzb_multi_match_list_top_indices_fused(self.handle" in multi and "fzb_multi_matcher_reserve_top_indices(self.handle" in multi
    assert "fn match_list_top_indices_device" in multi and "fn reserve_top_indices" in multi


def test_null_arguments_are_refused():
    l = F.lib()
    mm = F.MultiMatcher(F.parse_query("abc ab !d"))  # a matcher needs no device
    out, n, pos, found = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_uint64()
    fake = C.c_void_p(64)  # never dereferenced: the NULL checks come first
    null = C.c_void_p(None)
    fn = l.fzb_multi_match_list_top_indices_fused
    assert fn(null, fake, 1, C.byref(out), C.byref(n), C.byref(pos), C.byref(found)) == FZB_ERR_INVALID
    assert fn(mm.h, null, 1, C.byref(out), C.byref(n), C.byref(pos), C.byref(found)) == FZB_ERR_INVALID
    assert fn(mm.h, null, 1, None, C.byref(n), C.byref(pos), None) == FZB_ERR_INVALID
    assert fn(mm.h, null, 1, C.byref(out), None, C.byref(pos), None) == FZB_ERR_INVALID
    assert fn(mm.h, null, 1, C.byref(out), C.byref(n), None, None) == FZB_ERR_INVALID
    assert b"null" in l.fzb_last_error()
    dev = l.fzb_multi_match_list_top_indices_device
    assert dev(null, fake, 1, fake, 1, fake, 8, fake, None) == FZB_ERR_INVALID
    assert dev(mm.h, null, 1, fake, 1, fake, 8, fake, None) == FZB_ERR_INVALID
    assert dev(mm.h, fake, 1, fake, 1, fake, 8, null, None) == FZB_ERR_INVALID   # no count words
    assert dev(mm.h, fake, 1, null, 1, fake, 8, fake, None) == FZB_ERR_INVALID   # room for a record, no buffer
    assert dev(mm.h, fake, 1, fake, 1, null, 8, fake, None) == FZB_ERR_INVALID   # room for positions, no buffer
    assert b"null" in l.fzb_last_error()
    assert l.fzb_multi_matcher_reserve_top_indices(null, fake, 1, 8) == FZB_ERR_INVALID
    assert l.fzb_multi_matcher_reserve_top_indices(mm.h, null, 1, 8) == FZB_ERR_INVALID
    assert out.value is None and pos.value is None and n.value == 0


def test_queries_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    mm = F.MultiMatcher(F.parse_query("abc ab !d"))
    with pytest.raises(F.FrizbeeError):
        mm.match_list_top_indices(["abc"], 1)
    with pytest.raises(F.FrizbeeError):
        F.MultiMatcher(F.parse_query("!d")).match_list_top_indices(["abc"], 1)
    assert hasattr(mm, "match_list_top_indices_device") and hasattr(mm, "reserve_top_indices")


def test_cpp_facade_compiles_with_the_fused_calls():
    r = subprocess.run([build_facade()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_facade_multi_top_indices: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_fused_call_through_the_cpp_facade():
    r = subprocess.run([build_facade(), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_facade_multi_top_indices: ok" in r.stdout, r.stdout + r.stderr
