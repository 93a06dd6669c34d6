"""The boundary of a corpus that is edited (fzb_corpus_remove / _remove_device / _replace / _edit_info), without a GPU: the symbols are
declared, listed and exported, the header states the rules, bad arguments are refused before anything touches a device, editing without
a device fails loudly, and the C++ host side compiles."""
import ctypes as C
import os
import re
import subprocess

import pytest

import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_facade_edit")
NEW = ("fzb_corpus_remove", "fzb_corpus_remove_device", "fzb_corpus_replace", "fzb_corpus_edit_info")
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
    for name in NEW:
        assert name in declared and name in F.SYMBOLS
        assert getattr(F.lib(), name).argtypes is not None
    # declared behind fzb_corpus_info; the block states the scope, the synchronisation, the concurrency rule and what happens at 4 GiB
    at = header.index("int fzb_corpus_info(")
    text = header[header.index("A corpus that is EDITED"):header.index("int fzb_corpus_edit_info(")]
    assert header.index("A corpus that is EDITED") > at
    for phrase in ("fzb_sharded_corpus", "wait for the device's outstanding work", "concurrently", "FZB_ERR_CAPACITY", "fzb_match_list_device", "fzb_multi_match_list_device",
                   "Temporary device memory", "An error leaves the corpus exactly as it was"):
        assert phrase in text, phrase
    for name in ("remove", "remove_device", "replace", "edit_info"):
        assert callable(getattr(F.Corpus, name))


def test_bad_arguments_are_refused_before_any_device_is_touched():
    l = F.lib()
    null = C.c_void_p(None)
    idx, byte, end, info = (C.c_uint32 * 1)(0), (C.c_uint8 * 1)(97), (C.c_uint64 * 1)(1), (C.c_uint64 * 4)()
    fake = C.c_void_p(64)  # never dereferenced: the argument checks come first
    assert l.fzb_corpus_remove(null, idx, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_remove(fake, None, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_remove_device(null, idx, 4, idx, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_remove_device(fake, None, 4, idx, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_remove_device(fake, idx, 4, None, 1) == FZB_ERR_INVALID
    assert b"null" in l.fzb_last_error()
    for stride in (0, 6):
        assert l.fzb_corpus_remove_device(fake, idx, stride, idx, 1) == FZB_ERR_INVALID
        assert b"stride_bytes" in l.fzb_last_error()
    assert l.fzb_corpus_replace(null, idx, 1, byte, end) == FZB_ERR_INVALID
    assert l.fzb_corpus_replace(fake, None, 1, byte, end) == FZB_ERR_INVALID
    assert l.fzb_corpus_replace(fake, idx, 1, byte, None) == FZB_ERR_INVALID
    assert l.fzb_corpus_edit_info(null, info) == FZB_ERR_INVALID
    assert l.fzb_corpus_edit_info(fake, None) == FZB_ERR_INVALID
    assert b"null" in l.fzb_last_error()


def test_remove_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(F.FrizbeeError):
        F.Corpus(["a"]).remove([0])


def test_the_chunk_knob_is_documented():
    knobs = open(os.path.join(ROOT, "frizbee_amd", "csrc", "knobs.h")).read()
    assert "FZB_EDIT_CHUNK_ITEMS" in knobs


def test_cpp_facade_compiles_with_corpus_edit():
    r = subprocess.run([build_facade()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_facade_edit: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_corpus_edit_through_the_cpp_facade():
    r = subprocess.run([build_facade(), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_facade_edit: ok" in r.stdout, r.stdout + r.stderr
