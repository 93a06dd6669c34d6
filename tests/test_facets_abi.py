"""The boundary of the tag facets (fzb_facets_create / _free / _read / _device, fzb_matcher_set_facets, fzb_multi_matcher_set_facets), without
a GPU: the symbols are declared, listed and exported, the header states the layout, which entry points fill a sink and which refuse it,
bad arguments are refused before anything touches a device, facets.h is HIP-free and a build dependency, the kernels call its functions,
and the C++ host side compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_facade_facets")
NEW = ("fzb_facets_create", "fzb_facets_free", "fzb_facets_read", "fzb_facets_device", "fzb_matcher_set_facets", "fzb_multi_matcher_set_facets")
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
    assert "#define FZB_FACET_WORDS 34" in header and F.FACET_WORDS == 34 and F.FACET_BITS == 16
    assert header.index("int fzb_facets_create(") > header.index("typedef struct fzb_facets fzb_facets;") > header.index("fzb_multi_matcher_shard_report(")
    for cls, names in ((F.Facets, ("read", "read_words", "device_ptr")), (F.Matcher, ("set_facets",)), (F.MultiMatcher, ("set_facets",))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    import inspect
    assert inspect.signature(F.NarrowingQuery.__init__).parameters["facets"].default is None
    for cls in (F.NarrowingMatcher, F.NarrowingQuery):  # (NarrowingMatcher's constructor is positional and pinned: it takes the sink through set_facets)
        assert callable(cls.set_facets), cls
    for mirror, names in (("include/frizbee_hip.hpp", ("class Facets", "set_facets", "fzb_facets_read", "visible_by_bit")), ("rust/src/hip.rs", NEW)):
        text = open(os.path.join(ROOT, mirror)).read()
        for name in names:
            assert name in text, (mirror, name)


def test_the_header_states_the_layout_and_the_fill_or_refuse_rule():
    header = header_text()
    text = " ".join(header[header.index("TAG FACETS"):header.index("int fzb_facets_create(")].replace("*", " ").split())
    for phrase in ("[0] matched", "[1] visible", "[2 + b] all_by_bit[b]", "[18 + b] visible_by_bit[b]", "BEFORE scope, bias, selection, `limit` and ordering",
                   "a chip for an excluded bit shows what it hides", "the call's `found`", "counts 10 000", "none ignores the sink", "set_facets(NULL)",
                   "refused on another", "leaves both by_bit rows zero", "makes no second one", "allocates"):
        assert phrase.lower() in text.lower(), phrase
    filled = text[text.index("FILLED BY:"):text.index("REFUSED:")]
    for name in ("fzb_match_list,", "fzb_match_list_device", "fzb_match_list_sorted_device", "fzb_match_list_top,", "fzb_match_list_top_device", "fzb_match_list_top_indices,",
                 "fzb_match_list_top_indices_device", "_subset forms", "fzb_prompt_list_device", "fzb_prompt_top_device", "fzb_multi_match_list,", "fzb_multi_match_list_device",
                 "fzb_multi_match_list_top,", "fzb_multi_match_list_top_indices_fused"):
        assert name in filled, name
    refused = text[text.index("REFUSED:"):]
    for name in ("fzb_match_list_parallel,", "fzb_match_list_parallel_sharded", "fzb_match_list_top_sharded", "fzb_match_list_parallel_rccl", "fzb_match_list_indices,",
                 "fzb_match_list_indices_into", "fzb_multi_match_list_top_indices."):
        assert name in refused, name


def test_bad_arguments_are_refused_before_any_device_is_touched():
    l = F.lib()
    out = C.c_void_p()
    words = (C.c_uint32 * F.FACET_WORDS)()
    fake = C.c_void_p(64)  # never dereferenced: the argument checks come first
    assert l.fzb_facets_create(None, C.byref(out)) == FZB_ERR_INVALID and not out.value
    assert l.fzb_facets_create(fake, None) == FZB_ERR_INVALID
    assert l.fzb_facets_read(None, words) == FZB_ERR_INVALID
    assert l.fzb_facets_read(fake, None) == FZB_ERR_INVALID
    assert l.fzb_facets_device(None) is None
    assert l.fzb_matcher_set_facets(None, fake) == FZB_ERR_INVALID
    assert l.fzb_multi_matcher_set_facets(None, None) == FZB_ERR_INVALID
    assert b"null" in l.fzb_last_error()
    l.fzb_facets_free(None)
    # detaching a sink that was never attached is fine, for either matcher
    F.Matcher("abc").set_facets(None)
    F.MultiMatcher(F.parse_query("a b")).set_facets(None)


def test_a_sink_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(F.FrizbeeError):
        F.Facets(F.Corpus(["a"]))


def test_facets_header_is_a_build_dependency_hip_free_and_shared_by_the_kernels():
    csrc = os.path.join(ROOT, "frizbee_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "facets.h" in mk and "kernels_facets.o" in mk
    src = open(os.path.join(csrc, "facets.h")).read()
    assert "FZB_FACET_FN" in src and "hipStream_t" not in src and "#include <hip" not in src
    for name in ("scope_tag_of(", "scope_visible(", "facets_wave_step", "facets_lane_step", "facets_publish", "FZB_FACET_WORDS"):
        assert name in src, name
    assert len(re.findall(r"\bscope_visible\(", src)) == 1  # the predicate is called, not restated
    kern = open(os.path.join(csrc, "kernels_facets.hip")).read()
    for name in ("k_facets_records", "k_facets_column", "facets_wave_step(", "facets_publish(", "scope_tag_of(", "facet_item_tag(", "FZB_LAUNCH(", "tc_grid("):
        assert name in kern, name
    topk = open(os.path.join(csrc, "kernels_topk.hip")).read()
    assert "k_scope_flag_facets" in topk and "facets_wave_step(" in topk and '#include "facets.h"' in topk
    host = open(os.path.join(csrc, "host.hip")).read()
    assert host.count("fzb_launch_facets_records(") == 1 and host.count("fzb_launch_facets_column(") == 1  # one helper launches each


def test_the_python_mirror_names_the_four_fields():
    class Canned(F.Facets):  # read() over a canned block: no handle is used
        def __init__(self, words):
            self.h = None
            self._w = words

        def read_words(self):
            return self._w

    w = np.arange(34, dtype=np.uint32)
    r = Canned(w).read()
    assert r["matched"] == 0 and r["visible"] == 1
    assert isinstance(r["all_by_bit"], np.ndarray) and r["all_by_bit"].tolist() == list(range(2, 18)) and r["visible_by_bit"].tolist() == list(range(18, 34))


def test_cpp_facade_compiles_with_facets():
    r = subprocess.run([build_facade()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_facade_facets: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_facets_through_the_cpp_facade():
    r = subprocess.run([build_facade(), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_facade_facets: ok" in r.stdout, r.stdout + r.stderr
