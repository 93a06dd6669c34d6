"""The REPEAT signature (frizbee_amd/csrc/sig_filter.h), compiled for the host: which signature bits a haystack and a needle hold at least
twice against a plain Python count, the property the filter rests on (accepted => passes the signature test AND the repeat test) over
random pairs against a case-folded subsequence check, the repeat planes' transposition and the candidates under both tests.  No GPU."""
import os
import random

import numpy as np
import pytest

import frizbee_amd as F
import sig_repeat_host_lib as R
from sig_host_lib import py_sig, py_sig_bit
from sig_planes_host_lib import py_planes

pytestmark = pytest.mark.skipif(not R.available(), reason="needs ROCm's clang++")


def bits(*chars):
    return sum(1 << py_sig_bit(ord(c)) for c in set(chars))


def test_the_repeat_signature_of_random_byte_strings_equals_a_plain_count():
    l = R.lib()
    pr = random.Random(3)
    # letters of both cases (a case pair shares a bit), zero bytes (count for nothing), digits and signs that share an other-byte class
    # ('1' and '7': 49 % 6 == 55 % 6; '0' and '6'; '_' and '/'), and every byte value
    alphabets = [bytes(b"abAB"), bytes(b"a\x00b\x00"), bytes(b"17_06/-"), bytes(b"dDeEaAbB\x00_1"), bytes(range(256))]
    seen_case_pair = seen_class_pair = seen_zero = 0
    for k in range(4000):
        al = alphabets[k % len(alphabets)]
        h = bytes(pr.choice(al) for _ in range(pr.randint(0, 32)))
        want = R.py_sig2(h)
        assert l.sr_sig2_of_bytes(h, len(h)) == want, h
        assert l.sr_sig_of_bytes(h, len(h)) == py_sig(h)
        assert want & ~py_sig(h) == 0  # twice implies once
        padded = np.frombuffer(h + b"\x00" * (-len(h) % 4), np.uint32).copy()  # the device's way: words, zero behind the length
        assert l.sr_sig2_of_words(padded.ctypes.data, len(padded)) == want, h
        seen_case_pair += h.count(b"a") == 1 and h.count(b"A") == 1 and bool(want & 1)
        seen_class_pair += h.count(b"1") == 1 and h.count(b"7") == 1 and bool(want >> py_sig_bit(ord("1")) & 1)
        seen_zero += h.count(0) >= 2
    assert seen_case_pair > 50 and seen_class_pair > 10 and seen_zero > 100
    assert l.sr_sig2_of_bytes(b"\x00\x00\x00", 3) == 0 and l.sr_sig2_of_bytes(b"", 0) == 0
    assert l.sr_sig2_of_bytes(b"aXa", 2) == 0 and l.sr_sig2_of_bytes(b"aXa", 3) == bits("a")  # within the length only


@pytest.mark.parametrize("needle,want", [
    (b"deadbe", bits("d", "e")),     # doubled letters
    (b"deadbeef", bits("d", "e")),   # three e: counts cap at two
    (b"aaa", bits("a")),             # caps at two
    (b"dD", bits("d")),              # a letter and its case flip
    (b"17", bits("1")),              # two bytes in one other-byte class
    (b"a_b-1", 0),                   # no repeat
    (b"abc", 0),
])
def test_the_needles_repeat_signature(needle, want):
    l = R.lib()
    assert l.sr_needle_sig2(needle, len(needle)) == want == R.py_sig2(needle)
    assert want & ~l.sr_needle_sig(needle, len(needle)) == 0
    if needle == b"17":
        assert py_sig_bit(ord("1")) == py_sig_bit(ord("7")) >= 26


def accepted(needle, hay):
    """the ordered-subsequence automaton of an eligible needle, restated: every needle byte or its ASCII case flip, in order"""
    i = 0
    for b in hay:
        if i < len(needle) and b != 0 and (b == needle[i] or (chr(needle[i]).isalpha() and b == needle[i] ^ 0x20)):
            i += 1
    return i == len(needle)


def test_accepted_implies_both_tests_and_the_repeat_test_rejects_more():
    l = R.lib()
    pr = random.Random(11)
    alphabet = b"adeDE17_b"
    n_acc = n_rej_by_repeat = n_rej_by_sig = n_pass_both_rejected = 0
    for _ in range(40000):
        needle = bytes(pr.choice(alphabet) for _ in range(pr.randint(1, 5)))
        hay = bytes(pr.choice(alphabet + b"\x00xy") for _ in range(pr.randint(0, 12)))
        ns, ns2 = l.sr_needle_sig(needle, len(needle)), l.sr_needle_sig2(needle, len(needle))
        s, s2 = l.sr_sig_of_bytes(hay, len(hay)), l.sr_sig2_of_bytes(hay, len(hay))
        one = (s & ns) == ns
        both = bool(l.sr_passes(s, s2, ns, ns2))
        assert both == (one and (s2 & ns2) == ns2)
        if accepted(needle, hay):
            n_acc += 1
            assert one and both, (needle, hay)
        else:
            n_rej_by_sig += not one
            n_rej_by_repeat += one and not both
            n_pass_both_rejected += both
    assert n_acc > 2000 and n_rej_by_sig > 2000 and n_rej_by_repeat > 1000 and n_pass_both_rejected > 1000, (n_acc, n_rej_by_sig, n_rej_by_repeat, n_pass_both_rejected)


def test_the_transposition_and_the_candidates_under_both_tests():
    l = R.lib()
    pr = random.Random(21)
    n = 2 * 1024 + 301
    alphabet = "abdeDEABzq" + "017_/-"
    hays = ["".join(pr.choice(alphabet) for _ in range(pr.randint(0, 14))).encode() for _ in range(n)]
    sig = np.array([py_sig(h) for h in hays], np.uint32)
    sig2 = R.want_sig2(hays)
    planes = py_planes(sig)
    planes2 = np.full(len(planes), 0xA5A5A5A5A5A5A5A5, np.uint64)  # (the function writes every word)
    l.sr_transpose(sig2.ctypes.data, n, planes2.ctypes.data)
    assert planes2.tolist() == py_planes(sig2).tolist()
    fewer = 0
    for nd in (b"deadbe", b"aaa", b"dD", b"17", b"a_b-1", b"abc", b"17x71", b"zz", b"ae//"):
        ns, ns2 = l.sr_needle_sig(nd, len(nd)), l.sr_needle_sig2(nd, len(nd))
        one = (sig & np.uint32(ns)) == np.uint32(ns)
        want = one & ((sig2 & np.uint32(ns2)) == np.uint32(ns2))
        for t in range(3):
            for w in range(16):
                c = int(l.sr_candidates(planes.ctypes.data, planes2.ctypes.data, t, w, ns, ns2))
                lo = t * 1024 + w * 64
                exp = sum(1 << i for i in range(64) if lo + i < n and want[lo + i])
                assert c == exp, (nd, t, w)
        if ns2 == 0:
            assert (want == one).all()
        fewer += int(one.sum() - want.sum())
    assert fewer > 300


def test_the_entry_point_and_the_array_are_declared():
    root = R.ROOT
    name = "fzb_corpus_signature_repeat_planes_info"
    for path in (("include", "frizbee_hip.h"), ("include", "frizbee_hip.hpp"), ("rust", "src", "hip.rs")):
        assert name in open(os.path.join(root, *path)).read(), path
    assert name in F.SYMBOLS
    assert F.Corpus.DEBUG_ARRAYS["sig_planes2"] == (12, np.uint64) and F.Corpus.DEBUG_ARRAYS["sig_planes"] == (11, np.uint64)
    assert "At least three" in open(os.path.join(root, "frizbee_amd", "csrc", "sig_filter.h")).read()
