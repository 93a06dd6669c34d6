"""The signatures' bit-planes (frizbee_amd/csrc/sig_filter.h), compiled for the host: the reference transposition and the index function
against a plain Python transposition, zero bits at and beyond the item count, and the AND of a needle's planes against sig_passes row by
row.  No GPU."""
import os
import random

import numpy as np
import pytest

import frizbee_amd as F
import sig_planes_host_lib as P

pytestmark = pytest.mark.skipif(not P.available(), reason="needs ROCm's clang++")

COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 5 * 1024 + 7)


def transpose(sig):
    l = P.lib()
    sig = np.ascontiguousarray(sig, dtype=np.uint32)
    out = np.full(int(l.sp_words(len(sig))), 0xA5A5A5A5A5A5A5A5, np.uint64)  # (the function writes every word)
    l.sp_transpose(sig.ctypes.data, len(sig), out.ctypes.data)
    return out


def random_sigs(rng, n):
    s = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    s[rng.random(n) < 0.1] = 0xFFFFFFFF  # rows that pass every needle
    s[rng.random(n) < 0.1] = 0
    return s


@pytest.mark.parametrize("n", COUNTS)
def test_the_transposition_equals_the_plain_one_and_is_zero_beyond_the_count(n):
    l = P.lib()
    rng = np.random.default_rng(n)
    sig = random_sigs(rng, n)
    sig[-1] = 0xFFFFFFFF  # the last item sets every plane's last valid bit
    got = transpose(sig)
    tiles = (n + 1023) // 1024
    assert l.sp_tiles(n) == tiles and len(got) == tiles * 32 * 16 == l.sp_words(n)
    assert got.tolist() == P.py_planes(sig).tolist()
    # the definition itself, item by item, through the index function
    pr = random.Random(n)
    for i in sorted(set([0, n - 1] + [pr.randrange(n) for _ in range(200)])):
        for b in range(32):
            k = int(l.sp_index(i // 1024, b, (i % 1024) // 64))
            assert (int(got[k]) >> (i % 64)) & 1 == (int(sig[i]) >> b) & 1, (i, b)
    # bits at and beyond the count are zero, and the mask function says which are valid
    for t in range(tiles):
        for w in range(16):
            valid = int(l.sp_valid(t, w, n))
            lo = t * 1024 + w * 64
            assert valid == (1 << max(0, min(64, n - lo))) - 1
            for b in range(32):
                assert int(got[int(l.sp_index(t, b, w))]) & ~valid == 0


def test_the_index_function_is_tile_major_with_one_line_per_tile_and_bit():
    l = P.lib()
    seen = set()
    for t in range(3):
        for b in range(32):
            assert l.sp_index(t, b, 0) % 16 == 0  # 16 x 8 bytes: a 128-byte line
            for w in range(16):
                k = int(l.sp_index(t, b, w))
                assert k == (t * 32 + b) * 16 + w and k not in seen
                seen.add(k)
    assert seen == set(range(3 * 512))
    assert l.sp_index(4_000_000, 31, 15) == (4_000_000 * 32 + 31) * 16 + 15  # beyond 2^31 words
    assert 5 <= l.sp_batch_tiles() <= 8


def test_the_and_of_the_needles_planes_equals_sig_passes_per_row():
    l = P.lib()
    rng = np.random.default_rng(77)
    pr = random.Random(77)
    n = 2 * 1024 + 301
    alphabet = "abcdeDEADBEzq" + "0126<_/5-. ~{"
    hays = ["".join(pr.choice(alphabet) for _ in range(pr.randint(0, 32))).encode() for _ in range(n)]
    sig = np.array([l.sp_needle_sig(h, len(h)) for h in hays], np.uint32)
    planes = transpose(sig)
    needles = [b"deadbe", b"a_b-1", b"abcdeqz0", b"abcde012<_", b"~", b"z", b"-./", b"AbCdE_5{"] + \
              ["".join(pr.choice(alphabet) for _ in range(pr.randint(1, 12))).encode() for _ in range(12)]
    some_pass = some_fail = 0
    for nd in needles:
        ns = l.sp_needle_sig(nd, len(nd))
        assert ns != 0
        want = (sig & np.uint32(ns)) == np.uint32(ns)
        for t in range(3):
            for w in range(16):
                c = int(l.sp_candidates(planes.ctypes.data, t, w, ns))
                for i in range(64):
                    item = t * 1024 + w * 64 + i
                    exp = bool(want[item]) if item < n else False
                    assert (c >> i) & 1 == exp, (nd, item)
                    if item < n:
                        assert exp == bool(l.sp_passes(int(sig[item]), ns))
        some_pass += int(want.sum())
        some_fail += int((~want).sum())
    assert bin(l.sp_needle_sig(b"abcdeqz0", 8)).count("1") >= 8 and l.sp_needle_sig(b"a_b-1", 5) >> 26  # 8 distinct bits; non-letter bits
    assert some_pass > 1000 and some_fail > 1000


def test_the_knob_the_entry_point_and_the_selector_are_declared():
    root = P.ROOT
    assert "FZB_NO_SIG_PLANES" in open(os.path.join(root, "frizbee_amd", "csrc", "knobs.h")).read()
    assert 'on("FZB_NO_SIG_PLANES")' in open(os.path.join(root, "frizbee_amd", "csrc", "host.hip")).read()
    hdr = open(os.path.join(root, "include", "frizbee_hip.h")).read()
    assert "fzb_corpus_signature_planes_info" in hdr and "fzb_corpus_signature_planes_info" in F.SYMBOLS
    assert "fzb_corpus_signature_planes_info" in open(os.path.join(root, "include", "frizbee_hip.hpp")).read()
    assert "fzb_corpus_signature_planes_info" in open(os.path.join(root, "rust", "src", "hip.rs")).read()
    assert F.Corpus.DEBUG_ARRAYS["sig_planes"] == (11, np.uint64)
    assert F.lib().fzb_corpus_signature_planes_info(None, None, None) == 1
