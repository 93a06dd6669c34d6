"""The per-item decision of the item-list filter for large candidate sets (frizbee_amd/csrc/items_filter.h), compiled for the host: the
signature pre-test, the length test and the chain over a row's 16-byte vectors with the tail's byte count, fuzzed against the ORACLE's
0-typo prefilter and against sig_filter.h's own signature builder.  Lengths around every vector edge (0, 1, 15, 16, 17, 31, 32, 33,
255 - 257), needles of 1, 2 and 63 rows, rows that contain a NUL byte, and poison behind every row: the bytes after a row's end must not
reach the automaton.  No GPU."""
import ctypes as C
import os
import random

import pytest

import items_filter_host_lib as I
import oracle_lib as O

pytestmark = pytest.mark.skipif(not I.available(), reason="needs ROCm's clang++")
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257)
ALPHABET = "abcdeABCDE" + "zZ" + "0126<" + "_/5-. " + "~{"


def rows_of(needle, case_sensitive):
    c = needle.encode()
    f = c if case_sensitive else c.swapcase()
    return c, f


def plant(rng, L, needle, with_nul):
    hay = [rng.choice(ALPHABET) for _ in range(L)]
    if with_nul and L:
        for q in rng.sample(range(L), min(L, rng.randint(1, 3))):
            hay[q] = "\0"
    if rng.random() < 0.6 and L >= len(needle):
        for q, ch in zip(sorted(rng.sample(range(L), len(needle))), needle):
            hay[q] = ch if rng.random() < 0.7 else ch.swapcase()
    return "".join(hay).encode()


def test_vector_arithmetic():
    l = I.lib()
    for L in range(0, 600):
        nv = l.ifh_vecs(L)
        assert nv == (L + 15) // 16
        got = [l.ifh_vec_bytes(L, v) for v in range(nv + 2)]
        assert sum(got) == L and all(g == 16 for g in got[: max(nv - 1, 0)]) and got[nv:] == [0, 0], (L, got)
        if nv:
            assert got[nv - 1] == (L - 16 * (nv - 1))


def test_wants_row_is_the_length_test_and_the_signature_predicate():
    l = I.lib()
    rng = random.Random(3)
    for _ in range(5000):
        sig, nsig, L, ml = rng.getrandbits(32), rng.getrandbits(32) & rng.getrandbits(32), rng.randint(0, 40), rng.randint(0, 40)
        passes = (sig & nsig) == nsig
        assert l.ifh_sig_passes(sig, nsig) == int(passes)
        assert l.ifh_wants_row(1, sig, nsig, L, ml) == int(L >= ml and passes)
        assert l.ifh_wants_row(0, sig, nsig, L, ml) == int(L >= ml)


@pytest.mark.parametrize("rows", (1, 2, 63))
@pytest.mark.parametrize("with_nul", (False, True))
def test_decision_equals_the_oracle_prefilter(rows, with_nul):
    l = I.lib()
    rng = random.Random(100 * rows + with_nul)
    accepted = rejected = sig_rejected = 0
    for it in range(1500):
        needle = "".join(rng.choice(ALPHABET) for _ in range(rows))
        cs = rng.random() < 0.3
        c, f = rows_of(needle, cs)
        dfa = I.subsequence_dfa(c, f)
        nsig = l.ifh_needle_sig(c, len(c))
        for L in LENGTHS + (rng.randint(0, 300),):
            hay = plant(rng, L, needle, with_nul)
            want = bool(O.prefilter(needle, hay, 0, cs, False, 64)[0])
            # poison behind the row: the needle itself, which the automaton would happily consume
            buf = hay + (c * 40)[: 64 + (-len(hay)) % 16]
            got = l.ifh_decide(0, 0, 0, buf, L, rows, rows, dfa)
            assert got == int(want), (needle, hay, cs, L)
            # with the signature pre-test (rows of up to 32 bytes have signatures; the signature is the library's own builder's)
            hsig = l.ifh_sig_of_bytes(hay, len(hay))
            assert l.ifh_decide(1, hsig, nsig, buf, L, rows, rows, dfa) == int(want), (needle, hay, cs, L, "sig")
            # a row the signature rejects is rejected whatever its bytes hold (they are never requested)
            if (hsig & nsig) != nsig:
                sig_rejected += 1
                assert not want
                assert l.ifh_decide(1, hsig, nsig, c + bytes(64), len(c), rows, rows, dfa) == 0
            accepted += want
            rejected += not want
    assert accepted > (100 if rows == 63 else 1000) and rejected > 1000 and sig_rejected > 500, (accepted, rejected, sig_rejected)


def test_min_len_rejects_short_rows_and_chain_vec_counts_bytes():
    l = I.lib()
    c, f = rows_of("ab", False)
    dfa = I.subsequence_dfa(c, f)
    assert l.ifh_decide(0, 0, 0, b"ab" + bytes(30), 2, 2, 2, dfa) == 1
    assert l.ifh_decide(0, 0, 0, b"ab" + bytes(30), 2, 3, 2, dfa) == 0  # shorter than min_len
    assert l.ifh_decide(0, 0, 0, b"ab" + bytes(30), 1, 1, 2, dfa) == 0  # only the first byte belongs to the row
    w = (C.c_uint32 * 4)(int.from_bytes(b"xaxb", "little"), int.from_bytes(b"abab", "little"), 0, 0)
    assert [l.ifh_chain_vec(0, w, n, dfa) for n in range(0, 9)] == [0, 0, 1, 1, 2, 2, 2, 2, 2]
    assert l.ifh_chain_vec(1, w, 3, dfa) == 1 and l.ifh_chain_vec(1, w, 4, dfa) == 2
