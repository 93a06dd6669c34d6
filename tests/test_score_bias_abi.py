"""The boundary of the per-haystack score bias (fzb_corpus_set_bias / _update_bias / _clear_bias / _bias_info), without a GPU: the symbols
are declared, listed and exported, the header states the contract, bad arguments are refused before anything touches a device, setting a
bias without a device fails loudly, and the C++ host side compiles."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_facade_bias")
NEW = ("fzb_corpus_set_bias", "fzb_corpus_update_bias", "fzb_corpus_clear_bias", "fzb_corpus_bias_info")
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
    # declared beside the editing family, behind fzb_corpus_edit_info
    assert header.index("int fzb_corpus_set_bias(") > header.index("int fzb_corpus_edit_info(")
    assert header.index("int fzb_corpus_bias_info(") < header.index("int fzb_match_list(")
    for name in ("set_bias", "update_bias", "bias_info"):
        assert callable(getattr(F.Corpus, name))
    assert F.Corpus.DEBUG_ARRAYS["bias"] == (9, np.int16)
    assert "9 = the score bias" in header


def test_the_header_states_the_contract():
    header = header_text()
    text = " ".join(header[header.index("A PER-HAYSTACK SCORE BIAS"):header.index("int fzb_corpus_set_bias(")].replace("*", " ").split())
    assert "Every entry point that takes an fzb_corpus either returns biased scores or refuses a biased corpus with FZB_ERR_INVALID" in text
    for phrase in ("clamp(score + bias[i], 0, 65535)", "ONCE per record", "A score biased down to 0 stays in the result".lower(), "fzb_sharded_corpus", "borrowed one gets FZB_ERR_INVALID",
                   "wait for the device's outstanding work", "concurrently", "an error leaves the corpus as it was", "DEPARTURE from the reference", "fzb_multi_match_list_top_indices_fused",
                   "fzb_match_list_parallel_rccl", "src/matcher/mod.rs:215-221", "src/sort.rs:6-40"):
        assert phrase.lower() in text.lower(), phrase
    info = header[header.index("int fzb_corpus_clear_bias("):header.index("int fzb_corpus_bias_info(")]
    for phrase in ("bias_hi", "never lowered by an edit", "< 256"):
        assert phrase in info, phrase


def test_bad_arguments_are_refused_before_any_device_is_touched():
    l = F.lib()
    null = C.c_void_p(None)
    idx, val, info = (C.c_uint32 * 1)(0), (C.c_int16 * 1)(5), (C.c_uint64 * 4)()
    fake = C.c_void_p(64)  # never dereferenced: the argument checks come first
    assert l.fzb_corpus_set_bias(null, val, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_set_bias(fake, None, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_update_bias(null, idx, val, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_update_bias(fake, None, val, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_update_bias(fake, idx, None, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_clear_bias(null) == FZB_ERR_INVALID
    assert l.fzb_corpus_bias_info(null, info) == FZB_ERR_INVALID
    assert l.fzb_corpus_bias_info(fake, None) == FZB_ERR_INVALID
    assert b"null" in l.fzb_last_error()


def test_mismatched_arguments_are_refused_by_the_python_mirror():
    class NoHandle(F.Corpus):  # the checks below come before the handle is used
        def __init__(self):
            self.h = None

    c = NoHandle()
    with pytest.raises(F.FrizbeeError):
        c.update_bias([1, 2], [3])
    with pytest.raises(F.FrizbeeError):
        c.set_bias([40000])
    with pytest.raises(F.FrizbeeError):
        c.update_bias([1], [-40000])


def test_set_bias_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(F.FrizbeeError):
        F.Corpus(["a"]).set_bias([1])


def test_score_bias_header_is_a_build_dependency_and_hip_free():
    mk = open(os.path.join(ROOT, "frizbee_amd", "csrc", "Makefile")).read()
    assert "score_bias.h" in mk
    src = open(os.path.join(ROOT, "frizbee_amd", "csrc", "score_bias.h")).read()
    assert "FZB_SBIAS_FN" in src and "hipStream_t" not in src and "#include <hip" not in src


def test_cpp_facade_compiles_with_score_bias():
    r = subprocess.run([build_facade()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_facade_bias: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_score_bias_through_the_cpp_facade():
    r = subprocess.run([build_facade(), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_facade_bias: ok" in r.stdout, r.stdout + r.stderr
