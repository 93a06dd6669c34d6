"""The boundary of the sectioned top-`limit` calls (fzb_match_list_top_sections, its _device form and the fzb_multi_* pair), without a GPU:
the symbols are declared, listed and exported, the header states the limits and what is not offered, too many sections, too large a limit
and null arguments are refused with FZB_ERR_INVALID before anything touches a device, sections.h is HIP-free, shared by the kernels and a
build dependency, and the C++ host side compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_facade_sections")
NEW = ("fzb_match_list_top_sections", "fzb_match_list_top_sections_device", "fzb_multi_match_list_top_sections", "fzb_multi_match_list_top_sections_device")
FZB_ERR_INVALID = 1


def build_facade():
    src = EXE + ".cpp"
    hdrs = [os.path.join(ROOT, "include", h) for h in ("frizbee_hip.hpp", "frizbee_hip.h")]
    lib = os.path.join(ROOT, "frizbee_amd", "libfrizbee_hip.so")
    if not os.path.exists(EXE) or any(os.path.getmtime(f) > os.path.getmtime(EXE) for f in [src, lib] + hdrs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", EXE, "-L", os.path.join(ROOT, "frizbee_amd"),
                               "-lfrizbee_hip", "-Wl,-rpath," + os.path.join(ROOT, "frizbee_amd")])
    return EXE


def header_text():
    return open(os.path.join(ROOT, "include", "frizbee_hip.h")).read()


def test_symbols_are_declared_listed_and_exported():
    header = header_text()
    declared = set(re.findall(r"\b(fzb_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in F.SYMBOLS, name
        assert getattr(F.lib(), name).argtypes is not None
    assert "#define FZB_SECTIONS_MAX 8" in header and "#define FZB_SECTION_LIMIT_MAX 1024" in header
    assert "typedef struct { uint16_t require, exclude; } fzb_section;" in header
    assert F.SECTIONS_MAX == 8 and F.SECTION_LIMIT_MAX == 1024
    for cls in (F.Matcher, F.MultiMatcher):
        for name in ("match_list_top_sections", "match_list_top_sections_device"):
            assert callable(getattr(cls, name)), (cls, name)
    import inspect
    for cls in (F.Matcher, F.MultiMatcher):
        p = inspect.signature(cls.match_list_top_sections).parameters
        assert list(p)[:4] == ["self", "corpus", "sections", "limit"] and p["subset"].default is None and p["capture"].default is None
        assert p["subset"].kind is inspect.Parameter.KEYWORD_ONLY and p["capture"].kind is inspect.Parameter.KEYWORD_ONLY
    for mirror, names in (("include/frizbee_hip.hpp", ("match_list_top_sections", "match_list_top_sections_device", "SectionHead") + NEW), ("rust/src/hip.rs", NEW + ("FzbSection",))):
        text = open(os.path.join(ROOT, mirror)).read()
        for name in names:
            assert name in text, (mirror, name)


def test_the_header_states_the_contract_the_limits_and_what_is_left_out():
    header = header_text()
    text = " ".join(header[header.index("SECTIONED TOP-`limit`"):header.index("int fzb_match_list_top_sections(")].replace("*", " ").split())
    for phrase in ("(tag(i) & require) == require && (tag(i) & exclude) == 0", "the corpus' own scope AND section s's predicate", "ONE pass of the filter and the scorers",
                   "one host wait", "may overlap, repeat or be empty", "(0, 0) is \"everything\"", "first-match-wins", "at most FZB_SECTIONS_MAX sections",
                   "limit <= FZB_SECTION_LIMIT_MAX", "FZB_ERR_INVALID before anything touches the device", "n_sections == 0 returns nothing", "limit == 0 returns empty heads",
                   "capacity >= n_sections limit", "dev_out + s limit", "dev_counts[2s + 1]", "must not be read", "An attached facet sink is filled",
                   "NOT OFFERED: sharded and RCCL forms, matched positions (_indices)"):
        assert phrase.lower() in text.lower(), phrase


def test_bad_arguments_are_refused_before_any_device_is_touched():
    l = F.lib()
    fake = C.c_void_p(64)  # never dereferenced: the argument checks come first
    secs = np.zeros((9, 2), np.uint16)
    out, lens, found = C.c_void_p(), (C.c_size_t * 9)(), (C.c_uint64 * 9)()
    for fn in (l.fzb_match_list_top_sections, l.fzb_multi_match_list_top_sections):
        assert fn(fake, fake, secs.ctypes.data, 9, 10, None, None, C.byref(out), lens, found) == FZB_ERR_INVALID and not out.value
        assert b"FZB_SECTIONS_MAX" in l.fzb_last_error()
        assert fn(fake, fake, secs.ctypes.data, 8, 1025, None, None, C.byref(out), lens, found) == FZB_ERR_INVALID
        assert b"FZB_SECTION_LIMIT_MAX" in l.fzb_last_error()
        for args in ((None, fake, secs.ctypes.data, 1, 1, None, None, C.byref(out), lens, found), (fake, None, secs.ctypes.data, 1, 1, None, None, C.byref(out), lens, found),
                     (fake, fake, None, 1, 1, None, None, C.byref(out), lens, found), (fake, fake, secs.ctypes.data, 1, 1, None, None, None, lens, found),
                     (fake, fake, secs.ctypes.data, 1, 1, None, None, C.byref(out), None, found)):
            assert fn(*args) == FZB_ERR_INVALID and b"null" in l.fzb_last_error(), args
    for fn in (l.fzb_match_list_top_sections_device, l.fzb_multi_match_list_top_sections_device):
        assert fn(fake, fake, secs.ctypes.data, 9, 10, None, None, fake, 90, fake, None) == FZB_ERR_INVALID and b"FZB_SECTIONS_MAX" in l.fzb_last_error()
        assert fn(fake, fake, secs.ctypes.data, 8, 1025, None, None, fake, 8200, fake, None) == FZB_ERR_INVALID and b"FZB_SECTION_LIMIT_MAX" in l.fzb_last_error()
        for args in ((None, fake, secs.ctypes.data, 1, 1, None, None, fake, 1, fake, None), (fake, None, secs.ctypes.data, 1, 1, None, None, fake, 1, fake, None),
                     (fake, fake, None, 1, 1, None, None, fake, 1, fake, None), (fake, fake, secs.ctypes.data, 1, 1, None, None, None, 1, fake, None),
                     (fake, fake, secs.ctypes.data, 1, 1, None, None, fake, 1, None, None)):
            assert fn(*args) == FZB_ERR_INVALID and b"null" in l.fzb_last_error(), args


def test_the_python_mirror_refuses_what_the_library_refuses():
    class Handle:  # stands in for a Corpus: the checks come before the handle is used
        h = C.c_void_p(64)

    m = F.Matcher("abc")
    with pytest.raises(F.FrizbeeError):
        m.match_list_top_sections(Handle, [(0, 0)] * 9, 5)
    with pytest.raises(F.FrizbeeError):
        m.match_list_top_sections(Handle, [(0, 0)], 1025)
    with pytest.raises(ValueError):
        m.match_list_top_sections(Handle, [(0x10000, 0)], 5)
    mm = F.MultiMatcher(F.parse_query("a b"))
    with pytest.raises(F.FrizbeeError):
        mm.match_list_top_sections(Handle, [(0, 0)] * 9, 5)
    with pytest.raises(F.FrizbeeError):
        mm.match_list_top_sections_device(Handle, [(0, 0)], 1025, 64, 2000, 64)


def test_sections_header_is_a_build_dependency_hip_free_and_shared_by_the_kernels():
    csrc = os.path.join(ROOT, "frizbee_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert " sections.h " in mk and "kernels_sections.o" in mk
    src = open(os.path.join(csrc, "sections.h")).read()
    assert "FZB_SEC_FN" in src and "hipStream_t" not in src and "#include <hip" not in src and "__global__" not in src and "__shared__" not in src
    for name in ("sections_mask", "sections_pick_hi", "sections_cut_score", "sections_class", "sections_rank", "sections_before", "topk_pick_bin(", "topk_cut_by_score(",
                 "topk_cut_keep_all(", "SECTIONS_MAX 8", "SECTIONS_LIMIT_MAX 1024"):
        assert name in src, name
    assert len(re.findall(r"\bscope_visible\(", src)) == 1  # the predicate is called, not restated
    for restated in ("TOPK_HD uint32_t topk_pick_bin", "TopkCut topk_cut_by_score(uint32_t hi_bin", "uint32_t topk_dest(const"):
        assert restated not in src, restated  # reused from topk_select.h, unchanged
    kern = open(os.path.join(csrc, "kernels_sections.hip")).read()
    for name in ("k_sec_hist", "k_sec_cut", "k_sec_tile_counts", "k_sec_scan", "k_sec_scatter", "k_sec_order", "sections_mask(", "sections_pick_hi(", "sections_cut_score(",
                 "topk_cut_by_index(", "sections_class(", "topk_dest(", "sections_rank(", "scope_tag_of(", "FZB_LAUNCH(", "tc_grid("):
        assert name in kern, name
    assert "hipLaunchKernelGGL" not in kern and "<<<" not in kern  # every launch goes through FZB_LAUNCH
    host = open(os.path.join(csrc, "host.hip")).read()
    assert host.count("fzb_launch_sections_select(") == 1  # one helper launches the stage
    assert "fzb_grow_dev(&s.words" in host and "fzb_sections_release(s.sections)" in host and "fzb_sections_release(mm->sections)" in host


def test_cpp_facade_compiles_with_sections():
    r = subprocess.run([build_facade()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_facade_sections: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_sections_through_the_cpp_facade():
    r = subprocess.run([build_facade(), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_facade_sections: ok" in r.stdout, r.stdout + r.stderr
