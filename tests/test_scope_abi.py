"""The boundary of the per-haystack tags and the visibility scope (fzb_corpus_set_tags / _update_tags / _clear_tags / _set_scope /
_scope_info), without a GPU: the symbols are declared, listed and exported, the header states the contract sentence and the
honour-or-refuse rule, bad arguments are refused before anything touches a device, setting tags without a device fails loudly, scope.h is
HIP-free and a build dependency, and the C++ host side compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_facade_scope")
NEW = ("fzb_corpus_set_tags", "fzb_corpus_update_tags", "fzb_corpus_clear_tags", "fzb_corpus_set_scope", "fzb_corpus_scope_info")
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
        assert name in declared and name in F.SYMBOLS
        assert getattr(F.lib(), name).argtypes is not None
    # declared next to the bias block, ahead of the queries
    assert header.index("int fzb_corpus_set_tags(") > header.index("int fzb_corpus_bias_info(")
    assert header.index("int fzb_corpus_scope_info(") < header.index("int fzb_match_list(")
    for name in ("set_tags", "update_tags", "clear_tags", "set_scope", "scope_info"):
        assert callable(getattr(F.Corpus, name))
    assert F.Corpus.DEBUG_ARRAYS["tags"] == (10, np.uint16)
    assert "10 = the tags" in header
    for mirror, names in (("include/frizbee_hip.hpp", ("set_tags", "update_tags", "clear_tags", "set_scope", "scope_info")), ("rust/src/hip.rs", NEW)):
        text = open(os.path.join(ROOT, mirror)).read()
        for name in names:
            assert name in text, (mirror, name)


def test_the_header_states_the_contract_and_the_honour_or_refuse_rule():
    header = header_text()
    text = " ".join(header[header.index("PER-HAYSTACK TAGS AND A VISIBILITY SCOPE"):header.index("int fzb_corpus_set_tags(")].replace("*", " ").split())
    assert ("A query over a scoped corpus returns what the same query returns over a fzb_corpus_upload of the visible haystacks alone, in their order, with every `index` mapped back "
            "to the haystack's index in the full list.") in text
    assert "(tags[i] & require) == require && (tags[i] & exclude) == 0" in text
    assert "either HONOURS an active scope or REFUSES it with FZB_ERR_INVALID" in text and "none ignores the scope" in text
    for phrase in ("`found` counts visible matches only", "index = index_offset + (i - first)", "fzb_sharded_corpus", "borrowed one gets FZB_ERR_INVALID",
                   "wait for the device's outstanding work", "concurrently", "an error leaves the corpus as it was", "fzb_multi_match_list_top_indices_fused",
                   "fzb_match_list_parallel_rccl", "fzb_match_list_indices", "src/matcher/mod.rs:215-221", "src/sort.rs:6-40", "empty needle", "no allocation",
                   "dev_count[1] = visible matches"):
        assert phrase.lower() in text.lower(), phrase
    refused = text[text.index("Refused:"):]
    for name in ("fzb_match_list_indices", "fzb_multi_match_list_indices", "fzb_multi_match_list_top_indices", "fzb_match_list_parallel_rccl", "fzb_multi_match_list_parallel_rccl",
                 "ShardExchange"):
        assert name in refused, name


def test_bad_arguments_are_refused_before_any_device_is_touched():
    l = F.lib()
    null = C.c_void_p(None)
    idx, val, info = (C.c_uint32 * 1)(0), (C.c_uint16 * 1)(5), (C.c_uint64 * 4)()
    fake = C.c_void_p(64)  # never dereferenced: the argument checks come first
    assert l.fzb_corpus_set_tags(null, val, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_set_tags(fake, None, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_update_tags(null, idx, val, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_update_tags(fake, None, val, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_update_tags(fake, idx, None, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_clear_tags(null) == FZB_ERR_INVALID
    assert l.fzb_corpus_set_scope(null, 1, 2) == FZB_ERR_INVALID
    assert l.fzb_corpus_scope_info(null, info) == FZB_ERR_INVALID
    assert l.fzb_corpus_scope_info(fake, None) == FZB_ERR_INVALID
    assert b"null" in l.fzb_last_error()


def test_mismatched_arguments_are_refused_by_the_python_mirror():
    class NoHandle(F.Corpus):  # the checks below come before the handle is used
        def __init__(self):
            self.h = None

    c = NoHandle()
    with pytest.raises(F.FrizbeeError):
        c.update_tags([1, 2], [3])
    with pytest.raises(F.FrizbeeError):
        c.set_tags([70000])
    with pytest.raises(F.FrizbeeError):
        c.set_tags([-1])
    with pytest.raises(F.FrizbeeError):
        c.update_tags([1], [65536])
    with pytest.raises(F.FrizbeeError):
        c.update_tags([-1], [1])
    with pytest.raises(F.FrizbeeError):
        c.set_scope(require=65536)
    with pytest.raises(F.FrizbeeError):
        c.set_scope(exclude=-1)


def test_set_tags_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(F.FrizbeeError):
        F.Corpus(["a"]).set_tags([1])


def test_scope_header_is_a_build_dependency_and_hip_free():
    mk = open(os.path.join(ROOT, "frizbee_amd", "csrc", "Makefile")).read()
    assert "scope.h" in mk
    src = open(os.path.join(ROOT, "frizbee_amd", "csrc", "scope.h")).read()
    assert "FZB_SCOPE_FN" in src and "hipStream_t" not in src and "#include <hip" not in src
    for name in ("scope_visible", "scope_tile_keeps"):
        assert name in src
    topk = open(os.path.join(ROOT, "frizbee_amd", "csrc", "kernels_topk.hip")).read()
    assert "k_scope_flag" in topk and "scope_tile_keeps(" in topk and '#include "scope.h"' in topk


def test_cpp_facade_compiles_with_scope():
    r = subprocess.run([build_facade()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_facade_scope: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_scope_through_the_cpp_facade():
    r = subprocess.run([build_facade(), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_facade_scope: ok" in r.stdout, r.stdout + r.stderr
