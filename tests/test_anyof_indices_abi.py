"""The boundary of the grouped top + matched-positions query (fzb_multi_match_list_top_indices_groups / _groups_device,
fzb_multi_matcher_groups_positions_stride, fzb_multi_matcher_reserve_top_indices_groups), without a GPU: the symbols are declared, listed,
exported and mirrored, null arguments and capacity shortfalls - against U_g - are refused before anything touches a device, the header states
the carrier rule and U_g, and the C++ facade compiles with the new methods."""
import ctypes as C
import os
import re
import subprocess

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"fzb_multi_match_list_top_indices_groups": 9, "fzb_multi_match_list_top_indices_groups_device": 11, "fzb_multi_matcher_groups_positions_stride": 2,
       "fzb_multi_matcher_reserve_top_indices_groups": 4}
FZB_ERR_INVALID, FZB_ERR_CAPACITY = 1, 5


def header_text():
    return open(os.path.join(ROOT, "include", "frizbee_hip.h")).read()


def grouped():
    """`e (dead | deadbe | cafe) (rs$ | py$) !test`: U_g = 1 + 6 + 2"""
    pats, groups = F.parse_query_groups("e dead | deadbe | cafe rs$ | py$ !test")
    assert groups == [0, 1, 1, 1, 2, 2, 3]
    return F.MultiMatcher(pats, groups=groups)


def test_symbols_are_declared_listed_exported_and_mirrored():
    header = header_text()
    declared = set(re.findall(r"\b(fzb_[a-z0-9_]+)\s*\(", header))
    for name, nargs in NEW.items():
        assert name in declared and name in F.SYMBOLS, name
        fn = getattr(F.lib(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
    hpp = open(os.path.join(ROOT, "include", "frizbee_hip.hpp")).read()
    rs = open(os.path.join(ROOT, "rust", "src", "hip.rs")).read()
    multi = rs[rs.index("impl HipMultiMatcher"):rs.index("impl Drop for HipMultiMatcher")]
    for name in NEW:
        assert name + "(multi_.get()" in hpp, name
        assert ("fn " + name + "(") in rs and name + "(self.handle" in multi, name
    for method in ("match_list_top_indices_groups", "match_list_top_indices_groups_device", "groups_positions_stride", "reserve_top_indices_groups"):
        assert callable(getattr(F.MultiMatcher, method)), method
        assert re.search(r"\b" + method + r"\(", hpp) and ("fn " + method + "(") in multi, method
    assert not hasattr(F.Matcher, "match_list_top_indices_groups")


def test_the_header_states_the_carrier_rule_and_the_stride():
    header = header_text()
    text = " ".join(header[header.index("ANY-OF GROUPS WITH MATCHED POSITIONS"):header.index("int fzb_multi_matcher_reserve_top_indices_groups(")].replace("*", " ").split())
    for phrase in ("the head is exactly what fzb_multi_match_list_top / _top_subset return", "the carrier is chosen among the alternatives that match h",
                   "the largest key score << 1 | exact, on equal keys the first in query order", "The carrier's record is the group's record",
                   "src/matcher/multi.rs:56-82", "of each group's carrier ONLY", "Alternatives that match but do not carry contribute nothing; negated terms contribute nothing",
                   "U_g = the trace strides", "per group the maximum trace stride among its alternatives", "U_g replaces the U of the ungrouped forms in every capacity rule",
                   "A matcher WITHOUT a group takes the ungrouped path unchanged", "byte-identical", "only the top stage sees the set", "the bias is added once after the sum",
                   "four launches whatever the number of groups and alternatives", "One host wait in the host form, none in the device form",
                   "the traced passes disagree with the multi top stage", "Still REFUSED for a grouped matcher"):
        assert phrase in text, phrase
    # the refused paragraph stays and now points at the new forms
    refused = " ".join(header[header.index("REFUSED for a matcher with a group"):header.index("#define FZB_GROUP_ALTS_MAX")].replace("*", " ").split())
    assert "fzb_multi_match_list_top_indices_groups / _groups_device" in refused
    # no new refusal call site: the new entry points compose groups
    host = open(os.path.join(ROOT, "frizbee_amd", "csrc", "host.hip")).read()
    assert not re.search(r'fzb_refuse_groups\(mm, "fzb_[a-z_]*groups[a-z_]*"\)', host)


def test_the_stride_is_u_g():
    out = C.c_size_t(77)
    l = F.lib()
    assert l.fzb_multi_matcher_groups_positions_stride(None, C.byref(out)) == FZB_ERR_INVALID and l.fzb_multi_matcher_groups_positions_stride(grouped().h, None) == FZB_ERR_INVALID
    assert grouped().groups_positions_stride() == 1 + 6 + 2
    assert F.MultiMatcher(F.parse_query("e dead deadbe cafe !test")).groups_positions_stride() == 1 + 4 + 6 + 4  # without a group: U
    one = F.MultiMatcher([F.Pattern("dead"), F.Pattern(""), F.Pattern("xyzzy", negated=True)], groups=[0, 0, 1])  # a group left with one alternative is that plain pattern
    assert one.groups_positions_stride() == 4
    assert F.MultiMatcher([]).groups_positions_stride() == 0
    mm = grouped()
    mm.set_patterns(["ab", "abcde", "xyz"], groups=[0, 0, 0])
    assert mm.groups_positions_stride() == 5
    mm.set_patterns(["ab", "abcde", "xyz"])
    assert mm.groups_positions_stride() == 10


def test_null_arguments_and_capacity_shortfalls_are_refused_before_a_device_is_touched():
    l = F.lib()
    before = F.device_allocs()
    out, n, pos, found = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_uint64()
    fake = C.c_void_p(64)  # never dereferenced: the NULL checks come first
    null = C.c_void_p(None)
    for mm in (grouped(), F.MultiMatcher(F.parse_query("abc ab !d"))):
        fn = l.fzb_multi_match_list_top_indices_groups
        assert fn(null, fake, None, None, 1, C.byref(out), C.byref(n), C.byref(pos), C.byref(found)) == FZB_ERR_INVALID
        assert fn(mm.h, null, None, None, 1, C.byref(out), C.byref(n), C.byref(pos), C.byref(found)) == FZB_ERR_INVALID
        assert fn(mm.h, fake, None, None, 1, None, C.byref(n), C.byref(pos), None) == FZB_ERR_INVALID
        assert fn(mm.h, fake, None, None, 1, C.byref(out), None, C.byref(pos), None) == FZB_ERR_INVALID
        assert fn(mm.h, fake, None, None, 1, C.byref(out), C.byref(n), None, None) == FZB_ERR_INVALID
        assert b"null" in l.fzb_last_error()
        dev = l.fzb_multi_match_list_top_indices_groups_device
        assert dev(null, fake, None, None, 1, fake, 1, fake, 64, fake, None) == FZB_ERR_INVALID
        assert dev(mm.h, null, None, None, 1, fake, 1, fake, 64, fake, None) == FZB_ERR_INVALID
        assert dev(mm.h, fake, None, None, 1, fake, 1, fake, 64, null, None) == FZB_ERR_INVALID  # no count words
        assert dev(mm.h, fake, None, None, 1, null, 1, fake, 64, fake, None) == FZB_ERR_INVALID  # room for a record, no buffer
        assert dev(mm.h, fake, None, None, 1, fake, 1, null, 64, fake, None) == FZB_ERR_INVALID  # room for positions, no buffer
        assert b"null" in l.fzb_last_error()
        assert l.fzb_multi_matcher_reserve_top_indices_groups(null, fake, 1, 8) == FZB_ERR_INVALID
        assert l.fzb_multi_matcher_reserve_top_indices_groups(mm.h, null, 1, 8) == FZB_ERR_INVALID
    assert out.value is None and pos.value is None and n.value == 0
    # a corpus that borrows (fake, aligned) device memory touches no device: 100 haystacks, so min(limit, haystacks) is the limit below
    cp = C.c_void_p()
    l.fzb_corpus_from_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_uint64, C.POINTER(C.c_void_p)]
    assert l.fzb_corpus_from_device(fake, fake, 0, 100, 3200, C.byref(cp)) == 0
    dev = l.fzb_multi_match_list_top_indices_groups_device
    mm = grouped()
    ug = mm.groups_positions_stride()
    assert dev(mm.h, cp, None, None, 7, fake, 6, fake, 7 * ug, fake, None) == FZB_ERR_CAPACITY and b"6 < 7" in l.fzb_last_error()
    assert dev(mm.h, cp, None, None, 7, fake, 7, fake, 7 * ug - 1, fake, None) == FZB_ERR_CAPACITY
    assert ("%d < %d" % (7 * ug - 1, 7 * ug)).encode() in l.fzb_last_error()
    assert dev(mm.h, cp, None, None, 500, fake, 100, fake, 100 * ug - 1, fake, None) == FZB_ERR_CAPACITY  # min(limit, haystacks) = 100
    plain = F.MultiMatcher(F.parse_query("abc ab !d"))
    assert dev(plain.h, cp, None, None, 7, fake, 7, fake, 7 * 5 - 1, fake, None) == FZB_ERR_CAPACITY  # without a group: U
    l.fzb_corpus_free(cp)
    assert F.device_allocs() == before


def test_cpp_facade_compiles_with_the_grouped_calls(tmp_path):
    src = tmp_path / "facade_groups.cpp"
    src.write_text("""
#include <cstdio>
#include "frizbee_hip.hpp"
int main() {
    auto m = &frizbee::Matcher::match_list_top_indices_groups;
    auto d = &frizbee::Matcher::match_list_top_indices_groups_device;
    auto s = &frizbee::Matcher::groups_positions_stride;
    auto r = &frizbee::Matcher::reserve_top_indices_groups;
    std::printf("%d\\n", (m != nullptr) + (d != nullptr) + (s != nullptr) + (r != nullptr));
    return 0;
}
""")
    exe = tmp_path / "facade_groups"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", os.path.join(ROOT, "frizbee_amd"),
                           "-lfrizbee_hip", "-Wl,-rpath," + os.path.join(ROOT, "frizbee_amd")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "4", r.stdout + r.stderr
