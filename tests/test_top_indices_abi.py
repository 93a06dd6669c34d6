"""The boundary of the fused top + matched-positions query without a GPU: the new symbols are exported, declared and listed, NULL arguments
are refused before anything touches a device, the query fails loudly without a device, and the C++ host side compiles with a call to
`match_list_top_indices`."""
import ctypes as C
import os
import re
import subprocess

import pytest

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_facade_top_indices")
NEW = {"fzb_match_list_top_indices": 7, "fzb_match_list_top_indices_device": 9, "fzb_matcher_reserve_top_indices": 4, "fzb_multi_match_list_top_indices": 7}
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
    for name, nargs in NEW.items():
        assert name in declared and name in F.SYMBOLS
        fn = getattr(F.lib(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    # the header says what the result is a prefix of, and that the multi form is a host composition that re-orders nothing
    block = header[header.index("TOP-`limit` WITH MATCHED POSITIONS"):header.index("int fzb_match_list_top_indices(")]
    assert "src/matcher/mod.rs:234-275" in block
    multi = header[header.index("fzb_match_list_top_indices for a `from_patterns` matcher"):header.index("int fzb_multi_match_list_top_indices(")]
    assert "src/matcher/mod.rs:234-275" in multi and "HOST composition" in multi and "nothing is re-ordered" in multi
    for mirror, call in (("include/frizbee_hip.hpp", "match_list_top_indices"), ("rust/src/hip.rs", "fn match_list_top_indices"), ("rust/src/hip.rs", "fn reserve_top_indices")):
        assert call in open(os.path.join(ROOT, mirror)).read(), (mirror, call)


def test_null_arguments_are_refused():
    l = F.lib()
    m = F.Matcher("abc")       # a matcher needs no device
    mm = F.MultiMatcher(F.parse_query("abc !d"))
    out, n, pos, found = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_uint64()
    fake = C.c_void_p(64)  # never dereferenced: the NULL checks come first
    null = C.c_void_p(None)
    for fn, h in ((l.fzb_match_list_top_indices, m.h), (l.fzb_multi_match_list_top_indices, mm.h)):
        assert fn(null, fake, 1, C.byref(out), C.byref(n), C.byref(pos), C.byref(found)) == FZB_ERR_INVALID
        assert fn(h, null, 1, C.byref(out), C.byref(n), C.byref(pos), C.byref(found)) == FZB_ERR_INVALID
        assert fn(h, null, 1, None, C.byref(n), C.byref(pos), None) == FZB_ERR_INVALID
        assert fn(h, null, 1, C.byref(out), None, C.byref(pos), None) == FZB_ERR_INVALID
        assert fn(h, null, 1, C.byref(out), C.byref(n), None, None) == FZB_ERR_INVALID
        assert b"null" in l.fzb_last_error()
    dev = l.fzb_match_list_top_indices_device
    assert dev(null, fake, 1, fake, 1, fake, 8, fake, None) == FZB_ERR_INVALID
    assert dev(m.h, null, 1, fake, 1, fake, 8, fake, None) == FZB_ERR_INVALID
    assert l.fzb_matcher_reserve_top_indices(null, fake, 1, 8) == FZB_ERR_INVALID
    assert l.fzb_matcher_reserve_top_indices(m.h, null, 1, 8) == FZB_ERR_INVALID
    assert out.value is None and pos.value is None and n.value == 0


def test_queries_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(F.FrizbeeError):
        F.Matcher("abc").match_list_top_indices(["abc"], 1)
    with pytest.raises(F.FrizbeeError):
        F.MultiMatcher(F.parse_query("abc !d")).match_list_top_indices(["abc"], 1)


def test_cpp_facade_compiles_with_match_list_top_indices():
    r = subprocess.run([build_facade()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_facade_top_indices: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_match_list_top_indices_through_the_cpp_facade():
    r = subprocess.run([build_facade(), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_facade_top_indices: ok" in r.stdout, r.stdout + r.stderr
