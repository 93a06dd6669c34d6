"""A SECOND, independent transcription of the reference's literal matcher (src/literal/algo.rs:98-313; case_needle and
case_needle_unicode, src/prefilter/mod.rs:49-96; respects_case_for / respects_unicode_for, src/lib.rs:370-400), haystacks as bytes, the
lane count of the seed scan as a parameter.  Written from the reference alone, not from the oracle or the device kernels.  Test
infrastructure: tests/test_oracle_literal_second.py holds the C++ oracle to it, tests/test_gpu_literal_forms.py takes the occurrence
statistics of its lists from it.

One departure, on purpose: the reference seeds its substring scan with the two RAREST needle bytes (src/literal/rank.rs, a frequency
table); the table is not reproduced here.  `seeds` defaults to the first and the last needle byte and may be any two distinct offsets -
both seeds hit at every occurrence whichever they are, every hit but those of a 1- or 2-byte ASCII needle is verified by matches_at, and
for those the offsets are (0, 0) and (0, 1) whatever the table says (rank.rs:271-305)."""

DEFAULT_SCORING = dict(match_score=12, mismatch_penalty=6, gap_open_penalty=5, gap_extend_penalty=1, prefix_bonus=12, capitalization_bonus=4,
                       matching_case_bonus=4, exact_match_bonus=8, delimiter_bonus=4)
SCORING_FIELDS = tuple(DEFAULT_SCORING)


def scoring_of(values=None):
    """a scoring as the dict the functions below read: None = the defaults, else the nine values in the order of src/lib.rs:439-478"""
    return dict(DEFAULT_SCORING) if values is None else dict(zip(SCORING_FIELDS, values))


def respects_case_for(casing, needle):  # src/lib.rs:370-376
    return casing == "Respect" or (casing == "Smart" and any(c.isupper() for c in needle))


def respects_unicode_for(unicode, needle):  # src/lib.rs:394-400
    return unicode == "Always" or (unicode == "Smart" and not needle.isascii())


def case_needle(needle, case_sensitive):  # src/prefilter/mod.rs:49-65: (original, opposite case) per byte
    out = []
    for c in needle:
        if case_sensitive:
            out.append((c, c))
        elif 97 <= c <= 122:
            out.append((c, c - 32))
        elif 65 <= c <= 90:
            out.append((c, c + 32))
        else:
            out.append((c, c))
    return out


def case_needle_unicode(needle, case_sensitive):  # src/prefilter/mod.rs:71-96: (utf8 bytes, opposite-case utf8 bytes) per scalar
    out = []
    for c in needle:
        b = c.encode()
        other = c
        if not case_sensitive and c.isupper():
            low = c.lower()
            if len(low) == 1 and len(low.encode()) == len(b):
                other = low
        elif not case_sensitive and c.islower():
            up = c.upper()
            if len(up) == 1 and len(up.encode()) == len(b):
                other = up
        out.append((b, other.encode()))
    return out


def is_delimiter(byte):  # algo.rs:327-330
    return byte <= 127 and not (48 <= byte <= 57 or 65 <= byte <= 90 or 97 <= byte <= 122)


class Literal:
    """`LiteralImpl::new` (algo.rs:33-78) and what `Matcher` makes of its result (match_one_impl :99-116, match_one_indices_impl :135-155)"""

    def __init__(self, needle, mode, casing="Smart", unicode="Smart", scoring=None, lanes=16, seeds=None):
        assert isinstance(needle, str) and needle
        self.mode = mode
        self.s = scoring_of(scoring)
        self.lanes = lanes
        raw = needle.encode()
        self.needle_len = len(raw)
        case_sensitive = respects_case_for(casing, needle)
        self.unicode = respects_unicode_for(unicode, needle)
        self.needle_ascii = case_needle(raw, case_sensitive)
        self.needle_unicode = case_needle_unicode(needle, case_sensitive)
        if self.unicode:  # :43-50: the seeds' (original, opposite-case) bytes
            seed_bytes = [(c[i], f[i]) for c, f in self.needle_unicode for i in range(len(c))]
        else:
            seed_bytes = list(self.needle_ascii)
        if len(seed_bytes) >= 2:
            a, b = seeds if seeds is not None else (0, len(seed_bytes) - 1)
            assert 0 <= a < b < len(seed_bytes)
            if len(seed_bytes) == 2:
                assert (a, b) == (0, 1)
        else:
            a, b = 0, 0
        self.seed_a_off, self.seed_b_off = a, b
        self.seed_a, self.seed_b = seed_bytes[a], seed_bytes[b]

    # ---- matches_at, :157-178 ----
    def matches_at(self, hay, pos):
        if self.unicode:
            k = pos
            for c, f in self.needle_unicode:
                got = hay[k : k + len(c)]
                assert len(got) == len(c)  # (a Rust slice out of range panics: the callers never ask beyond the end)
                if got != c and got != f:
                    return False
                k += len(c)
        else:
            for k, (orig, flipped) in enumerate(self.needle_ascii):
                byte = hay[pos + k]
                if byte != orig and byte != flipped:
                    return False
        return True

    # ---- score_scalar, :180-202 ----
    def score_scalar(self, hay, start, matched_exact_case):
        s = self.s
        score = s["match_score"]
        if matched_exact_case:
            score += s["matching_case_bonus"]
        if start == 0:
            score += s["prefix_bonus"]
        else:
            byte, prev = hay[start], hay[start - 1]
            if 65 <= byte <= 90 and 97 <= prev <= 122:
                score += s["capitalization_bonus"]
            if is_delimiter(prev) and not is_delimiter(byte):
                score += s["delimiter_bonus"]
        return score

    # ---- score_at, :204-227 ----
    def score_at(self, hay, pos):
        score = 0
        if self.unicode:
            start = pos
            for c, _ in self.needle_unicode:
                score += self.score_scalar(hay, start, hay[start : start + len(c)] == c)
                start += len(c)
        else:
            for k, (orig, _) in enumerate(self.needle_ascii):
                start = pos + k
                score += self.score_scalar(hay, start, hay[start] == orig)
        if pos == 0 and self.needle_len == len(hay):
            score += self.s["exact_match_bonus"]
        assert score <= 0xFFFF  # u16 arithmetic under the overflow guard (:314-324)
        return score

    # ---- find, :229-255 ----
    def find(self, hay):
        n = self.needle_len
        if len(hay) < n:
            return None
        if self.mode == "Exact":
            return (0, self.score_at(hay, 0)) if len(hay) == n and self.matches_at(hay, 0) else None
        if self.mode == "Prefix":
            return (0, self.score_at(hay, 0)) if self.matches_at(hay, 0) else None
        if self.mode == "Suffix":
            pos = len(hay) - n
            return (pos, self.score_at(hay, pos)) if self.matches_at(hay, pos) else None
        assert self.mode == "Substring"
        return self.find_substring(hay)

    def _window(self, hay, start):  # load_window: the lanes behind the end never reach a result (zero here)
        chunk = list(hay[start : start + self.lanes])
        return chunk + [0] * (self.lanes - len(chunk))

    @staticmethod
    def _occ(chunk, pair):
        m = 0
        for i, b in enumerate(chunk):
            if b == pair[0] or b == pair[1]:
                m |= 1 << i
        return m

    # ---- find_substring, :257-313 ----
    def find_substring(self, hay):
        ln, n, L = len(hay), self.needle_len, self.lanes
        last_start = ln - n + 1
        best = None
        start = 0
        while start < last_start:
            usable = last_start - start
            valid = (1 << L) - 1 if usable >= L else (1 << usable) - 1
            hits_a = self._occ(self._window(hay, start + self.seed_a_off), self.seed_a) & valid
            if hits_a == 0:
                start += L
                continue
            if self.seed_a_off != self.seed_b_off:
                hits = hits_a & self._occ(self._window(hay, start + self.seed_b_off), self.seed_b)
            else:
                hits = hits_a
            while hits:
                low = hits & -hits
                pos = start + low.bit_length() - 1
                hits &= ~((low << 1) - 1)
                if (not self.unicode and n <= 2) or self.matches_at(hay, pos):
                    score = self.score_at(hay, pos)
                    if best is None or score > best[1]:  # strictly greater: the earliest of the best-scoring occurrences stays
                        best = (pos, score)
            start += L
        return best

    # ---- match_one_impl :99-116, match_one_indices_impl :135-155 ----
    def match_one(self, hay):
        """None, or (score, exact, indices): the matched run's byte offsets, last byte first"""
        found = self.find(hay)
        if found is None:
            return None
        pos, score = found
        exact = pos == 0 and self.needle_len == len(hay)
        return score, exact, list(range(pos + self.needle_len - 1, pos - 1, -1))

    def occurrences(self, hay):
        """every byte offset at which the needle occurs (Substring's candidates), ascending - for the statistics of the test lists"""
        return [p for p in range(len(hay) - self.needle_len + 1) if self.matches_at(hay, p)]
