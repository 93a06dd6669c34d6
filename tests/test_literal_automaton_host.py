"""The Knuth-Morris-Pratt table of a literal Substring matcher on the ASCII path (build_filter_tables, frizbee_amd/csrc/host.hip), on the
host: both forms the streaming filter kernels run - the class-composite table (fzb_debug_cdfa_state) and the byte table
(fzb_debug_kmp_dfa_accepts, also behind the haystack's end) - against Python's `in` on case-folded text, for needles whose restart state is
not 0: periodic needles, needles with long borders, mixed-case needles under every casing.  The haystacks are glued needle prefixes with
case flips, so that the automaton falls back from deep states.  No GPU."""
import ctypes as C

import numpy as np

import frizbee_amd as F

CASINGS = ("Ignore", "Smart", "Respect")


def needles(rng):
    """generated needles of 1..63 bytes, by family"""
    out = []
    pick = lambda alpha, n: "".join(alpha[int(x)] for x in rng.integers(0, len(alpha), n))
    for alpha in ("ab", "abc", "aA", "abA"):  # random needles over 2- and 3-letter alphabets, mixed case included
        for _ in range(70):
            out.append(("random " + alpha, pick(alpha, int(rng.integers(1, 64)))))
    for plen in (1, 2, 3, 4):  # a period repeated and cut at any length
        for _ in range(40):
            p = pick("abA_", plen)
            out.append(("period %d" % plen, (p * 64)[: int(rng.integers(1, 64))]))
    for _ in range(120):  # p^i c p^j
        p = pick("abc", int(rng.integers(1, 5)))
        i, j = int(rng.integers(1, 8)), int(rng.integers(1, 8))
        out.append(("p^i c p^j", (p * i + pick("abcd", 1) + p * j)[:63]))
    for n in range(1, 64):  # a^n
        out.append(("a^n", "a" * n))
    for k in range(1, 9):  # (a^k b)^j
        for j in range(1, 9):
            if (k + 1) * j <= 63:
                out.append(("(a^k b)^j", ("a" * k + "b") * j))
    for _ in range(120):  # letters with `_` and `/`
        p = pick("ab_/", int(rng.integers(1, 6)))
        out.append(("delimiters", (p * 64)[: int(rng.integers(1, 64))]))
    wide = "abcdefghijklmnopqrstuvwxyz"
    for nletters in range(13, 27):  # many byte classes: two transitions per composite lookup, or no composite table at all
        for cut in (nletters + 3, 2 * nletters + 1, 40, 63):
            out.append(("wide %d" % nletters, (wide[:nletters] * 5)[:cut]))
            out.append(("wide %d" % nletters, (wide[:nletters] * 5)[:cut].capitalize()))
    return out


def haystacks(rng, needle, count):
    """glued needle prefixes (the full needle and its near-misses among them), suffixes and filler, letters flipped in case now and then"""
    n = len(needle)
    out = []
    for _ in range(count):
        target = int(rng.integers(0, min(3 * n + 12, 220)))
        flip = float(rng.choice([0.0, 0.03, 0.15]))
        whole = rng.random() < 0.45  # this row may hold the full needle
        s = ""
        while len(s) < target:
            r = rng.random()
            if r < 0.55:
                k = n if whole and rng.random() < 0.3 else int(rng.integers(max(1, n - 3), n)) if rng.random() < 0.5 and n > 1 else int(rng.integers(1, n + 1))
                if k == n and not whole:
                    k = n - 1
                s += needle[:k]
            elif r < 0.75:
                s += needle[int(rng.integers(0, n)) :] if whole else needle[int(rng.integers(0, n)) :][: max(0, n - 2)]
            else:
                s += "q_ /x0Z"[int(rng.integers(0, 7))]
        s = "".join(c.swapcase() if rng.random() < flip else c for c in s[: max(target, 0)])
        out.append(s.encode())
    return out


def test_the_kmp_tables_decide_like_python_in():
    l = F.lib()
    rng = np.random.default_rng(20260)
    kg = (C.c_int32 * 2)()
    decisions = accepts = 0
    widths = {0: 0, 2: 0, 4: 0}
    by_family = {}
    for family, needle in needles(rng):
        assert 1 <= len(needle) <= 63
        for casing in CASINGS:
            m = F.Matcher(needle, F.Config(matching=F.Matching.Substring, casing=F.CaseMatching[casing]))
            cs = casing == "Respect" or (casing == "Smart" and needle != needle.lower())
            assert m.info()["case_sensitive"] == cs and not m.info()["unicode"]
            nb = needle.encode()
            composite = None
            for h in haystacks(rng, needle, 24):
                want = int(nb in h) if cs else int(nb.lower() in h.lower())
                got_c = l.fzb_debug_cdfa_state(m.h, h, len(h), kg)
                got_b = l.fzb_debug_kmp_dfa_accepts(m.h, h, len(h), 0)
                got_f = l.fzb_debug_kmp_dfa_accepts(m.h, h, len(h), int(rng.integers(1, 70)))  # the kernels read on behind the end: nothing changes
                assert got_b == want and got_f == want, (needle, casing, h, got_b, got_f, want)
                assert got_c in (-1, want), (needle, casing, h, got_c, want)
                assert composite in (None, got_c >= 0)
                composite = got_c >= 0
                assert (kg[1] in (2, 4)) == composite
                decisions += 1
                accepts += want
            widths[kg[1] if composite else 0] += 1
            f = by_family.setdefault(family, [0, 0])
            f[0] += 1
            f[1] += composite
    print("decisions", decisions, "accepted", accepts, "matchers by composition width (0 = byte table only)", widths, "by family (matchers, with a composite table)", by_family)
    assert decisions >= 50_000
    assert 5 * accepts >= decisions and 5 * (decisions - accepts) >= decisions, (accepts, decisions)
    assert widths[4] >= 100 and widths[2] >= 100 and widths[0] >= 20, widths


def test_the_byte_table_hook_is_only_for_ascii_substring_needles_of_up_to_63_bytes():
    l = F.lib()
    sub = lambda needle, **kw: F.Matcher(needle, F.Config(matching=F.Matching.Substring, **kw))
    assert l.fzb_debug_kmp_dfa_accepts(None, b"", 0, 0) == -1
    assert l.fzb_debug_kmp_dfa_accepts(F.Matcher("abab").h, b"abab", 4, 0) == -1  # fuzzy: the ordered-subsequence table
    assert l.fzb_debug_kmp_dfa_accepts(F.Matcher("abab", F.Config(matching=F.Matching.Prefix)).h, b"abab", 4, 0) == -1
    assert l.fzb_debug_kmp_dfa_accepts(sub("éaéa").h, "éaéa".encode(), 6, 0) == -1
    assert l.fzb_debug_kmp_dfa_accepts(sub("ab" * 32).h, b"ab" * 32, 64, 0) == -1  # 64 rows: beyond the by-value needle, no streaming automaton
    m = sub("ab" * 31 + "a")
    assert l.fzb_debug_kmp_dfa_accepts(m.h, b"b" + b"ab" * 31 + b"a", 64, 0) == 1 and l.fzb_debug_kmp_dfa_accepts(m.h, b"ab" * 30 + b"aab" + b"ab", 65, 3) == 0
    # a needle that holds a NUL byte: the zero fill behind a haystack could complete it, the kernels feed the dead byte instead - and so does the hook
    m = sub("a\0a\0")
    for h, want in ((b"a\0a", 0), (b"a\0a\0", 1), (b"xa\0a\0a", 1), (b"a\0a\0"[:3] + b"x", 0), (b"", 0), (b"a", 0)):
        for fill in (0, 1, 2, 17):
            assert l.fzb_debug_kmp_dfa_accepts(m.h, h, len(h), fill) == want, (h, fill)
        assert l.fzb_debug_cdfa_state(m.h, h, len(h), None) == want, h
