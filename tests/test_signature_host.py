"""The letter signatures of the streaming filter (frizbee_amd/csrc/sig_filter.h), compiled for the host: the two pure functions against a
plain Python restatement, the one invariant the filter relies on - whatever the 0-typo prefilter accepts has every needle bit in its
signature - against the oracle, and which needles are eligible.  No GPU."""
import ctypes as C
import random

import pytest

import frizbee_amd as F
import oracle_lib as O
import sig_host_lib as S

pytestmark = pytest.mark.skipif(not S.available(), reason="needs ROCm's clang++")


def test_sig_bit_and_signatures_equal_the_python_restatement_on_every_byte():
    l = S.lib()
    for b in range(256):
        if b:
            assert l.sh_sig_bit(b) == S.py_sig_bit(b), b
            assert 0 <= l.sh_sig_bit(b) < 32
        assert l.sh_sig_of_byte(b) == S.py_sig(bytes([b])), b
        assert l.sh_sig_of_bytes(bytes([b]), 1) == S.py_sig(bytes([b]))
        assert l.sh_needle_sig(bytes([b]), 1) == S.py_sig(bytes([b]))
    assert l.sh_sig_of_byte(0) == 0 and l.sh_sig_of_bytes(b"", 0) == 0 and l.sh_sig_of_bytes(bytes(32), 32) == 0
    # either case of a letter: the same bit; the six classes of the other bytes: '0' (48) and '6' (54) share one, '0' and '1' do not
    for c in range(26):
        assert l.sh_sig_bit(ord("a") + c) == l.sh_sig_bit(ord("A") + c) == c
    assert l.sh_sig_bit(ord("0")) == l.sh_sig_bit(ord("6")) == 26 and l.sh_sig_bit(ord("1")) == 27
    rng = random.Random(5)
    for _ in range(3000):
        bs = bytes(rng.randrange(256) for _ in range(rng.randint(0, 40)))
        assert l.sh_sig_of_bytes(bs, len(bs)) == S.py_sig(bs) == l.sh_needle_sig(bs, len(bs))
        w = rng.getrandbits(32)
        assert l.sh_sig_of_word(w) == S.py_sig(w.to_bytes(4, "little"))


def test_whatever_the_zero_typo_prefilter_accepts_has_every_needle_bit():
    l = S.lib()
    rng = random.Random(20)
    # cases, digits, punctuation, and bytes that share a bit: '0' / '6' / '<' / 'B'-6.., '_' (95 % 6 = 5) / '/' (47 % 6 = 5) / '5'
    alphabet = "abcdeABCDE" + "zZ" + "0126<" + "_/5-. " + "~{"
    accepted = rejected_by_sig = passed_sig_not_accepted = 0
    for it in range(20000):
        needle = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, 6)))
        L = rng.randint(0, 32)
        hay = [rng.choice(alphabet) for _ in range(L)]
        if rng.random() < 0.5 and L >= len(needle):  # plant the needle as a subsequence, case flipped here and there
            for q, ch in zip(sorted(rng.sample(range(L), len(needle))), needle):
                hay[q] = ch if rng.random() < 0.7 else ch.swapcase()
        hay = "".join(hay).encode()
        nb = needle.encode()
        cs = rng.random() < 0.3
        ok = O.prefilter(needle, hay, 0, cs, False, 64)[0]
        ns, hsig = l.sh_needle_sig(nb, len(nb)), l.sh_sig_of_bytes(hay, len(hay))
        assert l.sh_eligible(nb, len(nb), 0, 0) == 1
        if ok:
            accepted += 1
            assert hsig & ns == ns, (needle, hay, cs)
        elif hsig & ns != ns:
            rejected_by_sig += 1
        else:
            passed_sig_not_accepted += 1
    # the test is not vacuous in any direction: the signature rejects, the automaton still has work, and plenty is accepted
    assert accepted > 3000 and rejected_by_sig > 3000 and passed_sig_not_accepted > 500, (accepted, rejected_by_sig, passed_sig_not_accepted)


def test_eligibility():
    l = S.lib()
    assert l.sh_eligible(b"deadbe", 6, 0, 0) == 1 and l.sh_eligible(b"a_1", 3, 0, 0) == 1 and l.sh_eligible(b"x" * 32, 32, 0, 0) == 1
    assert l.sh_eligible(b"de\0d", 4, 0, 0) == 0          # a NUL byte
    assert l.sh_eligible("dé".encode(), 3, 0, 0) == 0      # a byte >= 0x80
    assert l.sh_eligible(b"a\x80", 2, 0, 0) == 0 and l.sh_eligible(b"\xff", 1, 0, 0) == 0 and l.sh_eligible(b"\x7f", 1, 0, 0) == 1
    for k in (1, 2, -1):                                   # max_typos != 0 (-1 = None)
        assert l.sh_eligible(b"deadbe", 6, k, 0) == 0
    for mode in (1, 2, 3, 4):                              # exact / prefix / suffix / substring
        assert l.sh_eligible(b"deadbe", 6, 0, mode) == 0
    assert l.sh_eligible(b"", 0, 0, 0) == 0


def test_the_matcher_computes_the_needle_signature_when_it_is_created_and_on_set_pattern():
    def sig_of(m):
        mask, el = C.c_uint32(), C.c_int()
        assert F.lib().fzb_debug_needle_signature(m.h, C.byref(mask), C.byref(el)) == 0
        return mask.value, bool(el.value)

    m = F.Matcher("DeadBe")
    assert sig_of(m) == (S.py_sig(b"DeadBe"), True) and S.py_sig(b"DeadBe") == S.py_sig(b"abde")
    m.set_pattern("a_1")
    assert sig_of(m) == (S.py_sig(b"a_1"), True)
    m.set_pattern("dé")
    assert sig_of(m) == (0, False)
    m.set_pattern("zz")
    m.set_config(F.Config(max_typos=1))
    assert sig_of(m) == (0, False)
    for cfg in (F.Config(max_typos=None), F.Config(max_typos=2), F.Config(unicode=F.UnicodeMatching.Always), F.Config(matching=F.Matching.Substring),
                F.Config(matching=F.Matching.Exact), F.Config(matching=F.Matching.Prefix), F.Config(matching=F.Matching.Suffix)):
        assert sig_of(F.Matcher("deadbe", cfg)) == (0, False), cfg
    assert sig_of(F.Matcher(b"de\0d")) == (0, False)
    assert sig_of(F.Matcher("é", F.Config(unicode=F.UnicodeMatching.Ignore))) == (0, False)
    assert sig_of(F.Matcher("a" * 70)) == (0, False)       # a long needle keeps k1_dfa
    assert sig_of(F.Matcher("")) == (0, False)
    assert sig_of(F.Matcher("x" * 32, F.Config(casing=F.CaseMatching.Respect))) == (S.py_sig(b"x"), True)
    assert F.lib().fzb_debug_needle_signature(None, None, None) == 1
    assert F.lib().fzb_debug_signature_threshold() == S.lib().sh_gather_max()


def test_the_knob_and_the_entry_points_are_declared():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "FZB_NO_SIGNATURE" in open(os.path.join(root, "frizbee_amd", "csrc", "knobs.h")).read()
    hdr = open(os.path.join(root, "include", "frizbee_hip.h")).read()
    for name in ("fzb_corpus_signature_info", "fzb_debug_needle_signature", "fzb_debug_signature_threshold"):
        assert name in hdr and name in F.SYMBOLS
    assert F.lib().fzb_corpus_signature_info(None, None, None) == 1
