"""The boundary of any-of groups (fzb_multi_matcher_create_groups, fzb_multi_matcher_set_pattern_groups, fzb_parse_query_groups), without a GPU:
the symbols are declared, listed, exported and mirrored, the header states the semantics and the refused forms, bad groupings and null
arguments are refused with FZB_ERR_INVALID before anything touches a device, the parser's table, anyof.h is HIP-free, shared by the kernels
and a build dependency, and the C++ host side compiles."""
import ctypes as C
import os
import re
import subprocess

import pytest

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_facade_anyof")
NEW = ("fzb_multi_matcher_create_groups", "fzb_multi_matcher_set_pattern_groups", "fzb_parse_query_groups", "fzb_query_groups_free")
REFUSED = ("fzb_multi_match_list_indices", "_indices_into", "_top_indices", "_top_indices_device", "_top_indices_fused", "_top_indices_subset", "_top_sections_indices",
           "_top_sections_indices_device", "fzb_multi_match_list_parallel_sharded", "_top_sharded", "_parallel_rccl")
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


def last_error():
    return F.lib().fzb_last_error().decode()


def test_symbols_are_declared_listed_exported_and_mirrored():
    header = header_text()
    declared = set(re.findall(r"\b(fzb_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in F.SYMBOLS, name
        assert getattr(F.lib(), name).argtypes is not None
    assert "#define FZB_GROUP_ALTS_MAX 8" in header
    import inspect
    assert callable(F.parse_query_groups)
    assert inspect.signature(F.MultiMatcher.__init__).parameters["groups"].default is None
    assert inspect.signature(F.MultiMatcher.set_patterns).parameters["groups"].default is None
    for mirror, names in (("include/frizbee_hip.hpp", ("from_pattern_groups", "parse_query_groups") + NEW), ("rust/src/hip.rs", NEW + ("build_groups", "set_pattern_groups"))):
        text = open(os.path.join(ROOT, mirror)).read()
        for name in names:
            assert name in text, (mirror, name)


def test_the_header_states_the_semantics_and_the_refused_forms():
    header = header_text()
    text = " ".join(header[header.index("ANY-OF GROUPS"):header.index("void fzb_query_groups_free(")].replace("*", " ").split())
    for phrase in ("a group matches a haystack iff at least one alternative matches it; the group's score is the maximum of the matching alternatives' scores and its exact flag the OR "
                   "of the exact flags of the alternatives whose score equals that maximum",
                   "a plain max over the key score << 1 | exact", "does not depend on the order of the alternatives", "exactly like ONE non-negated pattern",
                   "score = saturating sum, exact = OR", "Alternatives with an empty needle are dropped", "IS that plain pattern", "FZB_ERR_INVALID before anything touches the device",
                   "k pipelines, k accumulates, one clear, one flag, one compact", "allocated only by a matcher that has a group", "fzb_multi_matcher_reserve covers them",
                   "REFUSED for a matcher with a group", "says \"any-of group\"", "group_of == NULL is fzb_multi_matcher_create", "equal ids must be adjacent",
                   "skipped when the patterns AND the grouping are unchanged", "makes every pattern a single term again", "fzb_multi_matcher_clone carries the grouping",
                   "An atom that is exactly `|` joins the atom before it and the atom after it", "neither is negated and neither is itself `|`", "The atom `\\|` is the literal needle `|`",
                   "fzb_parse_query's patterns with all-distinct ids"):
        assert phrase in text, phrase
    refused = text[text.index("REFUSED for a matcher with a group"):text.index("#define FZB_GROUP_ALTS_MAX")]
    for name in REFUSED:
        assert name in refused, name
    served = text[text.index("SERVED for a matcher with a group"):text.index("REFUSED for a matcher with a group")]
    for name in ("fzb_multi_match_list", "_into", "_device", "_top", "_subset", "_top_subset", "_top_subset_device", "_top_sections", "_top_sections_device", "facet sink"):
        assert name in served, name
    # the library's messages name what the header names
    host = open(os.path.join(ROOT, "frizbee_amd", "csrc", "host.hip")).read() + open(os.path.join(ROOT, "frizbee_amd", "csrc", "host_shard.hip")).read() + \
        open(os.path.join(ROOT, "frizbee_amd", "csrc", "host_rccl.hip")).read()
    calls = set(re.findall(r'fzb_refuse_groups\(mm, "(fzb_[a-z_]+)"\)', host))
    assert calls == {"fzb_multi_match_list" + n if n.startswith("_") else n for n in REFUSED}, calls
    assert "the matcher has an any-of group" in host


def c_patterns(specs):
    return F._c_patterns([F.Pattern(n, negated=neg) for n, neg in specs])


def test_bad_groupings_and_null_arguments_are_refused_before_a_device_is_touched():
    l = F.lib()
    cfg = F._c_config(F.Config())
    out = C.c_void_p()
    ids = lambda *v: (C.c_uint32 * len(v))(*v)  # noqa: E731
    before = F.device_allocs()
    arr, keep = c_patterns([("a", False), ("b", True)])
    assert l.fzb_multi_matcher_create_groups(C.byref(cfg), arr, 2, ids(0, 0), C.byref(out)) == FZB_ERR_INVALID and not out.value
    assert "negated alternative" in last_error()
    assert l.fzb_multi_matcher_create_groups(C.byref(cfg), arr, 2, ids(0, 1), C.byref(out)) == 0 and out.value  # apart, the same two are an AND and a NOT
    mm = C.c_void_p(out.value)
    arr9, keep9 = c_patterns([(chr(ord("a") + i), False) for i in range(9)])
    out = C.c_void_p()
    assert l.fzb_multi_matcher_create_groups(C.byref(cfg), arr9, 9, ids(*[3] * 9), C.byref(out)) == FZB_ERR_INVALID and not out.value
    assert "9 alternatives" in last_error() and "FZB_GROUP_ALTS_MAX" in last_error()
    assert l.fzb_multi_matcher_create_groups(C.byref(cfg), arr9, 3, ids(0, 1, 0), C.byref(out)) == FZB_ERR_INVALID and "adjacent" in last_error()
    for args in ((None, arr9, 2, ids(0, 0), C.byref(out)), (C.byref(cfg), None, 2, ids(0, 0), C.byref(out)), (C.byref(cfg), arr9, 2, ids(0, 0), None)):
        assert l.fzb_multi_matcher_create_groups(*args) == FZB_ERR_INVALID and "null" in last_error(), args
    # the in-place form: the same refusals, and the matcher answers as before
    assert l.fzb_multi_matcher_set_pattern_groups(None, arr9, 2, ids(0, 0)) == FZB_ERR_INVALID and "null" in last_error()
    assert l.fzb_multi_matcher_set_pattern_groups(mm, None, 2, ids(0, 0)) == FZB_ERR_INVALID and "null" in last_error()
    assert l.fzb_multi_matcher_set_pattern_groups(mm, arr9, 9, ids(*[0] * 9)) == FZB_ERR_INVALID and l.fzb_multi_matcher_len(mm) == 2
    assert l.fzb_multi_matcher_set_pattern_groups(mm, arr9, 3, ids(7, 2, 7)) == FZB_ERR_INVALID and l.fzb_multi_matcher_len(mm) == 2
    assert l.fzb_multi_matcher_set_pattern_groups(mm, arr, 2, ids(4, 4)) == FZB_ERR_INVALID and l.fzb_multi_matcher_len(mm) == 2
    assert l.fzb_multi_matcher_set_pattern_groups(mm, arr9, 8, ids(*[0] * 8)) == 0 and l.fzb_multi_matcher_len(mm) == 8
    assert l.fzb_multi_matcher_set_pattern_groups(mm, arr9, 8, None) == 0 and l.fzb_multi_matcher_len(mm) == 8  # NULL: single terms
    # alternatives with an empty needle are dropped before the count and the negation are judged
    arr_e, keep_e = c_patterns([("a", False), ("", True)] + [("", False)] * 8 + [("b", False)])
    assert l.fzb_multi_matcher_set_pattern_groups(mm, arr_e, 11, ids(*[0] * 11)) == 0 and l.fzb_multi_matcher_len(mm) == 2
    l.fzb_multi_matcher_free(mm)
    assert F.device_allocs() == before
    with pytest.raises(ValueError):
        F.MultiMatcher(["a", "b"], groups=[0])
    with pytest.raises(F.FrizbeeError):
        F.MultiMatcher([F.Pattern("a"), F.Pattern("b", negated=True)], groups=[1, 1])
    m = F.MultiMatcher(["a", "b", "c"], groups=[0, 0, 1])
    assert m.groups == [0, 0, 1] and m.clone().groups == [0, 0, 1] and len(m.clone()) == 3
    m.set_patterns(["a", "b"])
    assert m.groups is None
    p = C.POINTER(F._CPattern)()
    g = C.POINTER(C.c_uint32)()
    n = C.c_size_t()
    for args in ((b"a", 1, None, C.byref(g), C.byref(n)), (b"a", 1, C.byref(p), None, C.byref(n)), (b"a", 1, C.byref(p), C.byref(g), None), (None, 1, C.byref(p), C.byref(g), C.byref(n))):
        assert l.fzb_parse_query_groups(*args) == FZB_ERR_INVALID and "null" in last_error(), args
    assert l.fzb_parse_query_groups(b"\xff", 1, C.byref(p), C.byref(g), C.byref(n)) == FZB_ERR_INVALID and "UTF-8" in last_error()
    l.fzb_query_groups_free(None, None, 0)


TABLE = [
    ("a | b", ["a", "b"], [0, 0]),
    ("a | b | c", ["a", "b", "c"], [0, 0, 0]),
    ("a | !b", ["a", "|", "b"], [0, 1, 2]),  # three plain atoms, the last negated
    ("!a | b", ["a", "|", "b"], [0, 1, 2]),
    ("| a", ["|", "a"], [0, 1]),
    ("a |", ["a", "|"], [0, 1]),
    ("a | | b", ["a", "|", "|", "b"], [0, 1, 2, 3]),
    ("|", ["|"], [0]),
    ("\\|", ["|"], [0]),
    ("a \\| b", ["a", "|", "b"], [0, 1, 2]),  # the escaped atom is a needle, never the operator
    ("a|b", ["a|b"], [0]),
    ("a\\ | b", ["a |", "b"], [0, 1]),  # the escaped blank keeps `|` inside the first atom
    ("a\\  | b", ["a ", "b"], [0, 0]),  # ... and here the atom ends behind it
    ("^src rs$ | py$ | go$ !test", ["src", "rs", "py", "go", "test"], [0, 1, 1, 1, 2]),
    ("x a | b y c | d", ["x", "a", "b", "y", "c", "d"], [0, 1, 1, 2, 3, 3]),
    ("a | ^$ | b", ["a", "|", "|", "b"], [0, 1, 2, 3]),  # an atom with an empty needle is dropped first: the two `|` are then doubled
    ("", [], []),
]


@pytest.mark.parametrize("query,needles,ids", TABLE)
def test_the_parser_table(query, needles, ids):
    pats, group_of = F.parse_query_groups(query)
    assert [p.needle for p in pats] == needles and group_of == ids, (query, pats, group_of)


def test_a_query_without_a_joining_bar_is_parse_query():
    def fields(pats):
        return [(p.needle, p.negated, p.matching) for p in pats]

    for query in ("dead be !x", "^dead 'ea f$", "!^a$ b\\ c 'd e$", "| a", "a |", "a | !b", "a || b", "a|b |c d|", "  إن  !ما ", "a\\\\ b", "!", "^$ a"):
        pats, group_of = F.parse_query_groups(query)
        assert fields(pats) == fields(F.parse_query(query)), query
        assert group_of == list(range(len(pats))), query
    pats, group_of = F.parse_query_groups("^a | b$ | 'c !d")
    assert fields(pats) == fields(F.parse_query("^a b$ 'c !d")) and group_of == [0, 0, 0, 1]


def test_anyof_header_is_a_build_dependency_hip_free_and_shared_by_the_kernels():
    csrc = os.path.join(ROOT, "frizbee_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert " anyof.h " in mk and "kernels_multi.o" in mk
    src = open(os.path.join(csrc, "anyof.h")).read()
    assert "FZB_ANYOF_FN" in src and "hipStream_t" not in src and "#include <hip" not in src and "__global__" not in src and "__shared__" not in src and "atomic" not in src.replace("no atomics", "").replace("no\n// atomics", "")
    for name in ("anyof_pack(", "anyof_combine(", "anyof_hit(", "anyof_score(", "anyof_exact(", "anyof_fold(", "anyof_join(", "anyof_find(", "ANYOF_ALTS_MAX 8", "0x80000000u"):
        assert name in src, name
    kern = open(os.path.join(csrc, "kernels_multi.hip")).read()
    for name in ("k_anyof_clear", "k_anyof_accumulate", "k_anyof_flag", "k_anyof_compact", "anyof_fold(", "anyof_hit(", "anyof_join(", "anyof_find(", "tc_flag_pass(", "tc_compact_items(",
                 "FZB_LAUNCH(", "tc_grid("):
        assert name in kern, name
    assert "hipLaunchKernelGGL" not in kern and "<<<" not in kern and "atomic" not in kern.replace("no atomics", "")  # every launch through FZB_LAUNCH; plain read-max-write
    host = open(os.path.join(csrc, "host.hip")).read()
    assert host.count("fzb_launch_anyof_keep(") == 1 and host.count("fzb_launch_anyof_clear(") == 1 and host.count("fzb_launch_anyof_accumulate(") == 1
    assert "if (mm->grouped && (rc = multi_ensure_group_buffers(mm))) return rc;" in host  # reserve covers them, only for a matcher that has a group


def test_cpp_facade_compiles_with_groups():
    r = subprocess.run([build_facade()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_facade_anyof: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_groups_through_the_cpp_facade():
    r = subprocess.run([build_facade(), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_facade_anyof: ok" in r.stdout, r.stdout + r.stderr
