"""The boundary of a corpus that grows, without a GPU: the new symbols are declared, listed and exported, NULL arguments are refused
before anything touches a device, appending without a device fails loudly, the C++ host side compiles - and the numpy model of the
device layout that the GPU tests measure against (corpus_layout_model.py) is pinned against a hand-built two-tile list."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import corpus_layout_model as L
import frizbee_amd as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_facade_append")
NEW = ("fzb_corpus_reserve", "fzb_corpus_append", "fzb_corpus_truncate", "fzb_corpus_info", "fzb_debug_corpus_read")
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
    # the header states the scope, the synchronisation and what happens at 4 GiB
    text = header[header.index("A corpus that GROWS"):header.index("int fzb_corpus_info(")]
    for phrase in ("fzb_sharded_corpus", "wait for the device's outstanding work", "concurrently", "FZB_ERR_CAPACITY"):
        assert phrase in text, phrase
    for name in ("append", "reserve", "truncate", "info"):
        assert callable(getattr(F.Corpus, name))


def test_null_arguments_are_refused():
    l = F.lib()
    null = C.c_void_p(None)
    byte, end, info, got = (C.c_uint8 * 1)(97), (C.c_uint64 * 1)(1), (C.c_uint64 * 12)(), C.c_size_t()
    fake = C.c_void_p(64)  # never dereferenced: the NULL checks come first
    assert l.fzb_corpus_append(null, byte, end, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_append(fake, byte, None, 1) == FZB_ERR_INVALID
    assert l.fzb_corpus_reserve(null, 1, 16) == FZB_ERR_INVALID
    assert l.fzb_corpus_truncate(null, 0) == FZB_ERR_INVALID
    assert l.fzb_corpus_info(null, info) == FZB_ERR_INVALID
    assert l.fzb_corpus_info(fake, None) == FZB_ERR_INVALID
    assert l.fzb_debug_corpus_read(null, 0, None, 0, C.byref(got)) == FZB_ERR_INVALID
    assert l.fzb_debug_corpus_read(fake, 0, None, 0, None) == FZB_ERR_INVALID
    assert b"null" in l.fzb_last_error()


def test_append_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(F.FrizbeeError):
        F.Corpus(["a"]).append(["b"])


def test_cpp_facade_compiles_with_corpus_append():
    r = subprocess.run([build_facade()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_facade_append: ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_corpus_append_through_the_cpp_facade():
    r = subprocess.run([build_facade(), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_facade_append: ok" in r.stdout, r.stdout + r.stderr


# ---- the layout model, pinned ------------------------------------------------------------------------------------------------------
def two_tiles():
    """1024 haystacks of 1 + (i % 50) bytes, then the hand-checked second tile: 40, 300 (an outlier), 0, 17 and 33 bytes"""
    first = [bytes([65 + i % 26]) * (1 + i % 50) for i in range(1024)]
    second = [b"a" * 40, b"b" * 300, b"", b"c" * 17, b"d" * 33]
    return first + second


def test_canonical_model_on_a_hand_built_list():
    data, ends = L.canonical([b"abc", b"", b"x" * 16, b"y" * 17])
    assert ends.tolist() == [3, 16, 32, 49]  # starts 0, 16, 16, 32; the empty haystack "ends" where it starts
    assert len(data) == 64 + 96
    assert data[:3].tobytes() == b"abc" and not data[3:16].any() and data[16:32].tobytes() == b"x" * 16 and data[32:49].tobytes() == b"y" * 17 and not data[49:].any()


def test_view_model_on_a_hand_built_two_tile_list():
    hs = two_tiles()
    assert L.wants_view(hs)
    v = L.build_view(hs)
    # second tile by hand: sorted 40 (item 0), 33 (item 4), 17 (item 3), then the key-0 pair - the outlier (item 1) and the empty one (item 2)
    assert v["vperm"][1024:].tolist() == [0, 4, 3, 1, 2] and v["vlen"][1024:].tolist() == [40, 33, 17, 0xFFFF, 0]
    assert v["vlong"].tolist() == [1025]
    # its group 0: longest member 40 bytes = 3 vectors, 8 tail bytes per member -> code 3 | (8/4 - 1) << 5, 2 rows of 64 units + 64 * 8 bytes
    assert int(v["vgnv"][16]) == (3 | (1 << 5)) and v["vgnv"][17:].tolist() == [0] * 15
    assert L.group_code(40) == (35, 160) and L.group_code(0) == (0, 0) and L.group_code(256) == (16 | (3 << 5), 15 * 64 + 64) and L.group_code(16) == (1 | (3 << 5), 64)
    # first tile by hand: 1 + i % 50 for 1024 items, sorted descending: group 0 starts with 50 bytes = 4 vectors, tail 2 -> 4 bytes per member
    assert int(v["vgnv"][0]) == (4 | (0 << 5)) and int(v["vgofs"][0]) == 0 and int(v["vgofs"][1]) == 3 * 64 + 16
    base = int(v["vgofs"][16]) * 16
    assert len(v["vbytes"]) == base + 160 * 16
    blk = v["vbytes"][base:]
    assert blk[0:16].tobytes() == b"a" * 16 and blk[16:32].tobytes() == b"d" * 16 and blk[32:48].tobytes() == b"c" * 16 and not blk[48:1024].any()
    assert blk[1024:1040].tobytes() == b"a" * 16 and blk[1040:1056].tobytes() == b"d" * 16 and blk[1056:1057].tobytes() == b"c" and not blk[1057:2048].any()
    assert blk[2048:2056].tobytes() == b"a" * 8 and blk[2056:2064].tobytes() == b"d" + b"\0" * 7 and not blk[2064:].any()
    decoded = L.check_view(hs, v)
    assert decoded[1025] is None and [d for i, d in enumerate(decoded) if i != 1025] == [h for i, h in enumerate(hs) if i != 1025]
    # the order of equal lengths is free: any shuffle of the ties decodes to the same list
    assert L.check_view(hs, L.build_view(hs, random.Random(5))) == decoded


def test_view_decoder_refuses_broken_views():
    hs = two_tiles()

    def broken(change):
        v = {k: a.copy() for k, a in L.build_view(hs).items()}
        change(v)
        with pytest.raises(L.ViewError):
            L.check_view(hs, v)

    broken(lambda v: v["vperm"].__setitem__(5, v["vperm"][6]))                      # not a permutation
    broken(lambda v: v["vperm"].__setitem__(slice(0, 1024), v["vperm"][:1024][::-1].copy()))  # ascending
    broken(lambda v: v["vgnv"].__setitem__(3, v["vgnv"][3] ^ 0x20))                 # a group's tail width
    broken(lambda v: v["vgofs"].__setitem__(7, v["vgofs"][7] + 1))                  # a group's block
    broken(lambda v: v["vlen"].__setitem__(1024, 41))                              # a length
    broken(lambda v: v.__setitem__("vlong", np.array([1025, 1025], np.uint32)))    # an outlier listed twice
    broken(lambda v: v.__setitem__("vlong", np.zeros(0, np.uint32)))               # ... or not at all
    broken(lambda v: v["vbytes"].__setitem__(3, 0))                                # a haystack's byte
    broken(lambda v: v["vbytes"].__setitem__(len(v["vbytes"]) - 1, 1))             # a byte where zeros belong
    broken(lambda v: v.__setitem__("vbytes", np.concatenate([v["vbytes"], np.zeros(16, np.uint8)])))  # more bytes than the groups take


def test_wants_view_follows_the_upload_criteria():
    assert not L.wants_view([]) and not L.wants_view([b"x" * 40] * 10)            # empty, uniform
    assert not L.wants_view([b"x" * 32, b"y" * 5])                                 # nothing beyond 32 bytes
    assert L.wants_view([b"x" * 33, b"y" * 5])
    assert not L.wants_view([b"x" * 300, b"y" * 5])                                # the only long one is an outlier
    assert L.wants_view([b"x" * 300] * 64 + [b"y" * 40]) and not L.wants_view([b"x" * 300] * 65 + [b"y" * 40])  # outliers <= n / 256 + 64
