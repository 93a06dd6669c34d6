"""The boundary of the candidate sets (fzb_subset, the *_subset queries, fzb_corpus_generation), without a GPU: the symbols are declared,
listed and exported with the documented signatures, the header states the contract sentence, the staleness rule and what is out of scope,
bad arguments are refused before anything touches a device, items_filter.h is HIP-free and a build dependency, the Python mirror has the
classes and keyword arguments, and `subset=None, capture=None` calls exactly the entry points it called before."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fzb_corpus_generation", "fzb_subset_create", "fzb_subset_free", "fzb_subset_set_indices", "fzb_subset_from_scope", "fzb_subset_info", "fzb_subset_read",
       "fzb_match_list_subset", "fzb_match_list_top_subset", "fzb_match_list_top_subset_device", "fzb_match_list_top_indices_subset", "fzb_debug_set_items_dfa_min")
FZB_ERR_INVALID = 1


def header_text():
    return open(os.path.join(ROOT, "include", "frizbee_hip.h")).read()


def test_symbols_are_declared_listed_and_exported_with_the_documented_signatures():
    header = header_text()
    declared = set(re.findall(r"\b(fzb_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in F.SYMBOLS, name
        assert getattr(F.lib(), name).argtypes is not None, name
    flat = " ".join(header.split())
    for sig in ("int fzb_corpus_generation(const fzb_corpus* c, uint64_t* out);", "int fzb_subset_create(const fzb_corpus* c, fzb_subset** out);", "void fzb_subset_free(fzb_subset* s);",
                "int fzb_subset_set_indices(fzb_subset* s, const uint32_t* host_indices, size_t n);", "int fzb_subset_from_scope(fzb_subset* s, const fzb_corpus* c, uint16_t require, uint16_t exclude);",
                "int fzb_subset_info(fzb_subset* s, uint64_t out[4]);", "int fzb_subset_read(fzb_subset* s, uint32_t* host_out, size_t cap, size_t* out_n);",
                "int fzb_match_list_subset(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, fzb_match** out, size_t* out_len);",
                "int fzb_match_list_top_subset(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match** out, size_t* out_len, uint64_t* out_found);",
                "int fzb_match_list_top_subset_device(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match* dev_out, size_t capacity, uint32_t* dev_count, void* stream);",
                "int fzb_match_list_top_indices_subset(fzb_matcher* m, const fzb_corpus* c, const fzb_subset* in, fzb_subset* capture, size_t limit, fzb_match_indices** out, size_t* out_len, uint32_t** out_positions, uint64_t* out_found);",
                "int fzb_corpus_info(const fzb_corpus* c, uint64_t out[12]);"):
        assert sig in flat, sig
    # declared behind the top-`limit` forms they extend
    assert header.index("typedef struct fzb_subset fzb_subset;") > header.index("int fzb_matcher_reserve_top_indices(")
    for mirror in ("include/frizbee_hip.hpp", "rust/src/hip.rs"):
        text = open(os.path.join(ROOT, mirror)).read()
        for name in NEW[:-1]:
            assert name in text, (mirror, name)


def test_the_header_states_the_contract_staleness_and_scope_of_the_feature():
    header = header_text()
    text = " ".join(header[header.index("CANDIDATE SETS"):header.index("int fzb_match_list_top_indices_subset(")].replace("*", " ").split())
    assert ("A query over subset S returns what the same query returns over a fzb_corpus_upload of the haystacks of S alone, in their order, with every `index` mapped back to the "
            "full list's.") in text
    for phrase in ("strictly ascending", "`found` counts the matches inside S", "src/matcher/mod.rs:215-221", "The reference has no such call", "borrowed one: FZB_ERR_INVALID",
                   "wait for the device's outstanding work", "an error leaves the subset as it was", "generation", "fzb_corpus_append", "_remove_device", "_replace", "\"stale\"",
                   "OUT OF SCOPE", "fzb_multi_matcher", "sharded and RCCL", "fzb_match_list_indices", "density switch", "capture == in", "BEFORE the list's terms", "EMPTY NEEDLE",
                   "no subset query allocates device memory", "unknown until fzb_subset_info is asked"):
        assert phrase.lower() in text.lower(), phrase


def test_null_arguments_are_refused_before_any_device_is_touched():
    l = F.lib()
    null, fake = C.c_void_p(None), C.c_void_p(64)  # `fake` is never dereferenced: the argument checks come first
    out, n, pos, found, gen, info = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_uint64(), C.c_uint64(), (C.c_uint64 * 4)()
    idx = (C.c_uint32 * 1)(0)
    assert l.fzb_corpus_generation(null, C.byref(gen)) == FZB_ERR_INVALID
    assert l.fzb_corpus_generation(fake, None) == FZB_ERR_INVALID
    assert l.fzb_subset_create(null, C.byref(out)) == FZB_ERR_INVALID
    assert l.fzb_subset_create(fake, None) == FZB_ERR_INVALID
    assert l.fzb_subset_set_indices(null, idx, 1) == FZB_ERR_INVALID
    assert l.fzb_subset_set_indices(fake, None, 1) == FZB_ERR_INVALID
    assert l.fzb_subset_from_scope(null, fake, 0, 0) == FZB_ERR_INVALID
    assert l.fzb_subset_from_scope(fake, null, 0, 0) == FZB_ERR_INVALID
    assert l.fzb_subset_info(null, info) == FZB_ERR_INVALID
    assert l.fzb_subset_info(fake, None) == FZB_ERR_INVALID
    assert l.fzb_subset_read(null, idx, 1, C.byref(n)) == FZB_ERR_INVALID
    assert l.fzb_subset_read(fake, idx, 1, None) == FZB_ERR_INVALID
    assert l.fzb_subset_read(fake, None, 1, C.byref(n)) == FZB_ERR_INVALID
    l.fzb_subset_free(null)  # a no-op
    for m, c in ((null, fake), (fake, null)):
        assert l.fzb_match_list_subset(m, c, null, null, C.byref(out), C.byref(n)) == FZB_ERR_INVALID
        assert l.fzb_match_list_top_subset(m, c, null, null, 5, C.byref(out), C.byref(n), C.byref(found)) == FZB_ERR_INVALID
        assert l.fzb_match_list_top_subset_device(m, c, null, null, 5, fake, 5, fake, None) == FZB_ERR_INVALID
        assert l.fzb_match_list_top_indices_subset(m, c, null, null, 5, C.byref(out), C.byref(n), C.byref(pos), C.byref(found)) == FZB_ERR_INVALID
    assert l.fzb_match_list_subset(fake, fake, null, null, None, C.byref(n)) == FZB_ERR_INVALID
    assert l.fzb_match_list_top_subset(fake, fake, null, null, 5, C.byref(out), None, None) == FZB_ERR_INVALID
    assert l.fzb_match_list_top_subset_device(fake, fake, null, null, 5, fake, 5, None, None) == FZB_ERR_INVALID
    assert l.fzb_match_list_top_indices_subset(fake, fake, null, null, 5, C.byref(out), C.byref(n), None, None) == FZB_ERR_INVALID
    assert b"null" in l.fzb_last_error()


def test_the_python_mirror():
    for name in ("set_indices", "from_scope", "info", "read", "__len__"):
        assert callable(getattr(F.Subset, name))
    for name in ("match_list", "match_list_top", "match_list_top_device", "match_list_top_indices"):
        params = inspect.signature(getattr(F.Matcher, name)).parameters
        for kw in ("subset", "capture"):
            assert params[kw].kind is inspect.Parameter.KEYWORD_ONLY and params[kw].default is None, (name, kw)
    params = inspect.signature(F.NarrowingMatcher.__init__).parameters
    assert list(params)[1:] == ["corpus", "config", "max_fraction"] and params["max_fraction"].default is None
    assert callable(F.NarrowingMatcher.query) and 0.0 <= F.NarrowingMatcher.DEFAULT_MAX_FRACTION <= 1.0
    assert callable(F.Corpus.generation)

    class NoHandle(F.Subset):  # the check below comes before the handle is used
        def __init__(self):
            self.h = None

    with pytest.raises(ValueError):
        NoHandle().set_indices([-1])
    with pytest.raises(ValueError):
        NoHandle().set_indices(np.array([0.5]))


def test_without_a_subset_the_calls_are_the_ones_they_were():
    """subset=None, capture=None: fzb_match_list / _top / _top_device / _top_indices themselves, never the *_subset entry points"""
    src = inspect.getsource(F.Matcher)
    for plain, sub in (("fzb_match_list(", "fzb_match_list_subset("), ("fzb_match_list_top,", "fzb_match_list_top_subset("), ("fzb_match_list_top_device(", "fzb_match_list_top_subset_device("),
                       ("fzb_match_list_top_indices,", "fzb_match_list_top_indices_subset(")):
        assert src.index("if subset is None and capture is None:") < src.index(plain) and plain in src and sub in src, plain
    assert src.count("if subset is None and capture is None:") == 4


def test_creating_a_subset_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(F.FrizbeeError):
        F.Subset(F.Corpus(["a"]))


def test_items_filter_header_is_a_build_dependency_and_hip_free():
    mk = open(os.path.join(ROOT, "frizbee_amd", "csrc", "Makefile")).read()
    assert "items_filter.h" in mk and "kernels_subset.o" in mk
    src = open(os.path.join(ROOT, "frizbee_amd", "csrc", "items_filter.h")).read()
    assert "FZB_ITEMS_FN" in src and "hipStream_t" not in src and "#include <hip" not in src and '#include "sig_filter.h"' in src
    assert "sig_passes(" in src and "(sig & " not in src  # the signature predicate is sig_filter.h's, not a second copy
    filt = open(os.path.join(ROOT, "frizbee_amd", "csrc", "kernels_filter.hip")).read()
    assert "k1_items_dfa" in filt and '#include "items_filter.h"' in filt and "items_wants_row(" in filt and "items_chain_vec(" in filt
    sub = open(os.path.join(ROOT, "frizbee_amd", "csrc", "kernels_subset.hip")).read()
    assert "scope_visible(" in sub and '#include "scope.h"' in sub  # from_scope's predicate is scope.h's
    knobs = open(os.path.join(ROOT, "frizbee_amd", "csrc", "knobs.h")).read()
    assert "FZB_NO_ITEMS_DFA" in knobs
