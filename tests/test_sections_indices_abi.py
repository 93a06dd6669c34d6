"""The boundary of the sectioned top-`limit` calls with matched positions (fzb_match_list_top_sections_indices, its _device form and the
fzb_multi_* pair), without a GPU: the symbols are declared, listed, exported and mirrored, the header states the contract and the 2S + 4
count words and no longer lists matched positions for sectioned heads as not offered, too many sections, too large a limit and null arguments
are refused with FZB_ERR_INVALID before anything touches a device, the placement arithmetic lives in sections.h and the fused queries share
one tail, and the C++ host side compiles."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_facade_sections_indices")
NEW = ("fzb_match_list_top_sections_indices", "fzb_match_list_top_sections_indices_device", "fzb_multi_match_list_top_sections_indices",
       "fzb_multi_match_list_top_sections_indices_device")
FZB_ERR_INVALID = 1


def build_facade():
    src = EXE + ".cpp"
    hdrs = [os.path.join(ROOT, "include", h) for h in ("frizbee_hip.hpp", "frizbee_hip.h")]
    lib = os.path.join(ROOT, "frizbee_amd", "libfrizbee_hip.so")
    if not os.path.exists(EXE) or any(os.path.getmtime(f) > os.path.getmtime(EXE) for f in [src, lib] + hdrs):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", EXE, "-L", os.path.join(ROOT, "frizbee_amd"),
                               "-lfrizbee_hip", "-Wl,-rpath," + os.path.join(ROOT, "frizbee_amd")])
    return EXE


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_symbols_are_declared_listed_exported_and_mirrored():
    header = read("include", "frizbee_hip.h")
    declared = set(re.findall(r"\b(fzb_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in F.SYMBOLS, name
        assert getattr(F.lib(), name).argtypes is not None
    for cls in (F.Matcher, F.MultiMatcher):
        for name in ("match_list_top_sections_indices", "match_list_top_sections_indices_device"):
            assert callable(getattr(cls, name)), (cls, name)
        p = inspect.signature(cls.match_list_top_sections_indices).parameters
        assert list(p)[:4] == ["self", "corpus", "sections", "limit"] and p["subset"].default is None and p["capture"].default is None
        assert p["subset"].kind is inspect.Parameter.KEYWORD_ONLY and p["capture"].kind is inspect.Parameter.KEYWORD_ONLY
        p = inspect.signature(cls.match_list_top_sections_indices_device).parameters
        assert list(p)[:9] == ["self", "corpus", "sections", "limit", "dev_out_ptr", "capacity", "dev_positions_ptr", "positions_capacity", "dev_counts_ptr"]
    for mirror, names in (("include/frizbee_hip.hpp", ("match_list_top_sections_indices", "match_list_top_sections_indices_device", "SectionHeadIndices") + NEW),
                          ("rust/src/hip.rs", NEW)):
        text = read(*mirror.split("/"))
        for name in names:
            assert name in text, (mirror, name)


def test_the_header_states_the_contract_the_count_words_and_what_is_left_out():
    header = read("include", "frizbee_hip.h")
    text = " ".join(header[header.index("SECTIONED TOP-`limit` WITH MATCHED POSITIONS"):header.index("int fzb_match_list_top_sections_indices(")].replace("*", " ").split())
    for phrase in ("fzb_match_list_top_indices(corpus, limit) returns over a corpus whose scope is the corpus' own scope AND section s's predicate",
                   "ties at the cut included", "all four sort strategies", "de-duplicated union over the non-negated patterns", "ONE pass of the filter and the scorers",
                   "ONE traced pass over the heads", "ONE host wait", "exactly as in fzb_match_list_top_sections", "(0, 0) reproduces fzb_match_list_top_indices",
                   "appears in each head with its positions", "freed with fzb_match_indices_free", "dense over the whole block", "empty position lists",
                   "capacity >= n_sections min(limit, haystacks) records", "FZB_ERR_CAPACITY before any launch", "2 n_sections + 4 words",
                   "[2s] = records of head s", "[2s + 1] = matches in section s", "[2S] = records in all", "[2S + 1] unspecified", "[2S + 2] = position dwords written",
                   "[2S + 3] = 0", "Not for an empty needle"):
        assert phrase.lower() in text.lower(), phrase
    # matched positions for sectioned heads are no longer among what is not offered; sharded / RCCL forms and larger limits still are
    sections = " ".join(header[header.index("SECTIONED TOP-`limit`:"):header.index("int fzb_match_list_top_sections(")].replace("*", " ").split())
    left_out = sections[sections.index("NOT OFFERED:"):]
    assert "for sectioned heads" not in left_out.split(".")[0] and "sharded and RCCL forms" in left_out and "limits above FZB_SECTION_LIMIT_MAX" in left_out
    assert "_sections_indices forms below" in left_out
    design = read("DESIGN.md")
    assert "k_sec_items" in design and "fzb_match_list_top_sections_indices" in design and "sections_indices.txt" in read("profiles", "README.md")
    assert "match_list_top_sections_indices" in read("README.md") and "fzb_match_list_top_sections_indices" in read("INTEGRATION.md")


def test_bad_arguments_are_refused_before_any_device_is_touched():
    l = F.lib()
    fake = C.c_void_p(64)  # never dereferenced: the argument checks come first
    secs = np.zeros((9, 2), np.uint16)
    out, pos, lens, found = C.c_void_p(), C.c_void_p(), (C.c_size_t * 9)(), (C.c_uint64 * 9)()
    for fn in (l.fzb_match_list_top_sections_indices, l.fzb_multi_match_list_top_sections_indices):
        assert fn(fake, fake, secs.ctypes.data, 9, 10, None, None, C.byref(out), lens, C.byref(pos), found) == FZB_ERR_INVALID and not out.value and not pos.value
        assert b"FZB_SECTIONS_MAX" in l.fzb_last_error()
        assert fn(fake, fake, secs.ctypes.data, 8, 1025, None, None, C.byref(out), lens, C.byref(pos), found) == FZB_ERR_INVALID
        assert b"FZB_SECTION_LIMIT_MAX" in l.fzb_last_error()
        for args in ((None, fake, secs.ctypes.data, 1, 1, None, None, C.byref(out), lens, C.byref(pos), found),
                     (fake, None, secs.ctypes.data, 1, 1, None, None, C.byref(out), lens, C.byref(pos), found),
                     (fake, fake, None, 1, 1, None, None, C.byref(out), lens, C.byref(pos), found),
                     (fake, fake, secs.ctypes.data, 1, 1, None, None, None, lens, C.byref(pos), found),
                     (fake, fake, secs.ctypes.data, 1, 1, None, None, C.byref(out), None, C.byref(pos), found),
                     (fake, fake, secs.ctypes.data, 1, 1, None, None, C.byref(out), lens, None, found)):
            assert fn(*args) == FZB_ERR_INVALID and b"null" in l.fzb_last_error(), args
    for fn in (l.fzb_match_list_top_sections_indices_device, l.fzb_multi_match_list_top_sections_indices_device):
        assert fn(fake, fake, secs.ctypes.data, 9, 10, None, None, fake, 90, fake, 900, fake, None) == FZB_ERR_INVALID and b"FZB_SECTIONS_MAX" in l.fzb_last_error()
        assert fn(fake, fake, secs.ctypes.data, 8, 1025, None, None, fake, 8200, fake, 82000, fake, None) == FZB_ERR_INVALID and b"FZB_SECTION_LIMIT_MAX" in l.fzb_last_error()
        for args in ((None, fake, secs.ctypes.data, 1, 1, None, None, fake, 1, fake, 8, fake, None), (fake, None, secs.ctypes.data, 1, 1, None, None, fake, 1, fake, 8, fake, None),
                     (fake, fake, None, 1, 1, None, None, fake, 1, fake, 8, fake, None), (fake, fake, secs.ctypes.data, 1, 1, None, None, None, 1, fake, 8, fake, None),
                     (fake, fake, secs.ctypes.data, 1, 1, None, None, fake, 1, None, 8, fake, None), (fake, fake, secs.ctypes.data, 1, 1, None, None, fake, 1, fake, 8, None, None)):
            assert fn(*args) == FZB_ERR_INVALID and b"null" in l.fzb_last_error(), args


def test_the_python_mirror_refuses_what_the_library_refuses():
    class Handle:  # stands in for a Corpus: the checks come before the handle is used
        h = C.c_void_p(64)

    m = F.Matcher("abc")
    with pytest.raises(F.FrizbeeError):
        m.match_list_top_sections_indices(Handle, [(0, 0)] * 9, 5)
    with pytest.raises(F.FrizbeeError):
        m.match_list_top_sections_indices(Handle, [(0, 0)], 1025)
    with pytest.raises(ValueError):
        m.match_list_top_sections_indices(Handle, [(0x10000, 0)], 5)
    mm = F.MultiMatcher(F.parse_query("a b"))
    with pytest.raises(F.FrizbeeError):
        mm.match_list_top_sections_indices(Handle, [(0, 0)] * 9, 5)
    with pytest.raises(F.FrizbeeError):
        mm.match_list_top_sections_indices_device(Handle, [(0, 0)], 1025, 64, 2000, 64, 20000, 64)


def test_the_placement_is_in_sections_h_and_the_fused_queries_share_one_tail():
    csrc = os.path.join(ROOT, "frizbee_amd", "csrc")
    src = open(os.path.join(csrc, "sections.h")).read()
    for name in ("sections_slab_kept(", "sections_head_base(", "sections_head_dest(", "SECTIONS_NO_SLOT"):
        assert name in src, name
    assert "hipStream_t" not in src and "#include <hip" not in src and "__global__" not in src and "__shared__" not in src
    kern = open(os.path.join(csrc, "kernels_sections.hip")).read()
    for name in ("k_sec_items", "sections_head_base(", "sections_head_dest(", "fzb_launch_sections_items("):
        assert name in kern, name
    assert "hipLaunchKernelGGL" not in kern and "<<<" not in kern  # every launch goes through FZB_LAUNCH
    host = open(os.path.join(csrc, "host.hip")).read()
    # one tail per matcher type, called by the plain fused query and the sectioned one; the traced pass and the pack are launched nowhere else
    assert host.count("top_indices_tail(m, c, want, stride") == 2 and host.count("multi_top_indices_tail(mm, c, want, U") == 2
    assert host.count("fzb_launch_indices_pack(") == 2 and host.count("fzb_launch_multi_union(") == 1 and host.count("fzb_launch_top_items(") == 2
    assert host.count("fzb_launch_sections_items(") == 2 and host.count("fzb_launch_sections_select(") == 1
    assert "if (s.slabs) (void)hipFree(s.slabs)" in host


def test_cpp_facade_compiles_with_sections_indices():
    r = subprocess.run([build_facade()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_facade_sections_indices: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_sections_indices_through_the_cpp_facade():
    r = subprocess.run([build_facade(), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_facade_sections_indices: ok" in r.stdout, r.stdout + r.stderr
