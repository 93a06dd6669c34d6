"""Needles, list shapes and the haystack generator of the literal-mode parity tests (tests/test_gpu_literal_forms.py on the device,
tests/test_oracle_literal_second.py on the host).  Needles with borders - periodic ones above all - so that the Knuth-Morris-Pratt automaton
of a Substring needle restarts from deep states and most accepted haystacks hold several, overlapping, occurrences; haystacks glued from
needle prefixes, near-misses that an occurrence restarts inside, case flips and filler, with occurrences planted so that they end on or
straddle the byte offsets at which a filter kernel changes what it does.  No GPU, no library call: plain Python over bytes."""
import random

from lit_second_transcription import Literal

N_ROWS = 3 * 1024 + 517  # three full tiles; the last one ends inside a tile and inside a 64-row group (517 = 8 * 64 + 5)

# shape -> (longest haystack, rows beyond 256 bytes).  s32: the two pre-requested vectors of k1_dfa; v128 / v256: the filter view's 8 and 16
# vectors per row; out: the same with as many rows beyond 256 bytes as a list of N_ROWS keeps its view with (n / 256 + 64), decided one vector per lane
SHAPES = {"s32": (32, 0), "v128": (128, 0), "v256": (256, 0), "out": (256, 70)}
OUT_MAX = 700
EDGES = (4, 16, 32, 128, 256)  # an occurrence ends on, or straddles, each of these (and the haystack's last byte)

SCORINGS = {
    "default": [12, 6, 5, 1, 12, 4, 4, 8, 4],
    # pairwise different bonuses: an occurrence at offset 0 (+20), behind a delimiter (+9), on a capital after a lowercase letter (+5) and a plain
    # one score differently, and so do a letter in the needle's case (+3) and its flip; the exact bonus (+17) is no sum of two others
    "distinct": [11, 6, 5, 1, 20, 5, 3, 17, 9],
}
CASINGS = ("Smart", "Ignore", "Respect")
MODES = ("Exact", "Prefix", "Suffix", "Substring")

_L40 = "abcdefghijklmnopqrstuvwxyz0123456789_/-."  # 40 byte classes
# name -> (needle, shapes it is run on, composition width of its class-composite table: 4, 2, 0 = none, None = no streaming automaton)
NEEDLES = {
    "aa": ("aa", ("s32", "v128", "v256", "out"), 4),
    "aab": ("aab", ("s32", "v128", "v256", "out"), 4),
    "abab": ("abab", ("s32", "v128", "v256", "out"), 4),
    "aaaa": ("aaaa", ("s32", "v128", "v256", "out"), 4),
    "a_a_a": ("a_a_a", ("s32", "v128", "v256", "out"), 4),
    "aabaaab": ("aabaaab", ("s32", "v128", "v256", "out"), 4),
    "abcabcab": ("abcabcab", ("s32", "v128", "v256", "out"), 4),
    "Ab/Ab": ("Ab/Ab", ("s32", "v128", "v256", "out"), 4),
    "ab*16": ("ab" * 16, ("v128", "v256", "out"), 4),
    "a*31+b": ("a" * 31 + "b", ("v128", "v256", "out"), 4),
    "aab*21": ("aab" * 21, ("v128", "v256", "out"), 4),  # 63 bytes: the longest needle passed by value
    "abc*64": (("abc" * 22)[:64], ("v128", "v256", "out"), None),  # 64 rows: the needle's arrays in device memory from here on
    "aab*65": (("aab" * 22)[:65], ("v128", "v256", "out"), None),
    "ab*40": ("ab" * 40, ("v128", "v256", "out"), None),
    "13 letters": ("abcdefghijklm" * 2 + "abc", ("v128", "v256", "out"), 2),  # 14 byte classes: two transitions per composite lookup
    # 41 byte classes: no composite table, the byte table in the burst kernel (48 bytes of period 40: two occurrences take 88, so not on v128)
    "40 letters": (_L40 + _L40[:8], ("v256", "out"), 0),
    "NUL": ("a\0a\0a", ("s32", "v128", "v256", "out"), 4),  # the zero fill behind a haystack is a needle byte: the sanitising forms
    "éaéa": ("éaéa", ("s32", "v128", "v256", "out"), None),
    "жжж": ("жжж", ("s32", "v128", "v256", "out"), None),
    "다a다a": ("다a다a", ("s32", "v128", "v256", "out"), None),
}


def units_of(needle):
    """the needle as its scalars' byte strings (bytes, on the ASCII path)"""
    return [c.encode() for c in needle]


def longest_border(units):
    n = len(units)
    for b in range(n - 1, 0, -1):
        if units[:b] == units[n - b :]:
            return b
    return 0


def make_list(name, shape, n_rows=N_ROWS, seed=0):
    """the list of one (needle, shape) pair: n_rows haystacks as bytes"""
    needle = NEEDLES[name][0]
    units = units_of(needle)
    nu, nb = len(units), len(needle.encode())
    max_len, n_out = SHAPES[shape]
    rng = random.Random(f"{name}/{shape}/{seed}")
    folded = needle.lower()
    breakers = [c.encode() for c in "qxzwv0179,:+~=" if c not in folded]
    if not needle.isascii():  # bytes that are no scalar: a stray continuation byte, a scalar that lost its last byte, a lead byte alone
        breakers += [b"\x80", b"\xbf", units[0][:-1] if len(units[0]) > 1 else b"\xc3", "다".encode()[:2], b"\xd0"]
    delims = [b"_", b"/", b" ", b"-", b"."]
    border = longest_border(units)
    prefix = lambda k: b"".join(units[:k])
    whole = prefix(nu)

    def near_miss():
        r = rng.random()
        if r < 0.4 and nu > 1:  # one unit short, then something else
            return prefix(nu - 1) + rng.choice(breakers)
        if r < 0.7 and nu > 1:  # one unit replaced (the breaker behind it: the rest of the needle starts nothing)
            k = rng.randrange(nu)
            return prefix(k) + rng.choice(breakers) + b"".join(units[k + 1 :]) + rng.choice(breakers)
        return prefix(rng.randint(0, nu - 1)) + rng.choice(breakers)  # a prefix, cut by a breaker

    def occurrence():
        """one occurrence or a run of overlapping ones, in one of the contexts that score differently, some letters flipped in case"""
        r = rng.random()
        body = whole
        if r < 0.35:  # the needle continued by its period: occurrences that overlap
            body = whole + b"".join(units[border:]) * rng.randint(1, 2)
        elif r < 0.55 and nu > 1:  # one unit short of an occurrence, and the occurrence restarts inside the near-miss
            k = rng.randint(max(1, nu - 3), nu - 1)
            body = prefix(k) + whole
        if len(body) > nb and rng.random() < 0.4:  # a letter near the front in the other case: it costs the first occurrence its case bonus, a later one scores higher
            chars = list(body.decode())
            j = rng.randrange(nu - border)
            if len(chars[j].swapcase().encode()) == len(chars[j].encode()):
                chars[j] = chars[j].swapcase()
            body = "".join(chars).encode()
        ctx = rng.random()
        lead = rng.choice(delims) if ctx < 0.3 else rng.choice([b"k", b"m", b"t"]) if ctx < 0.5 else rng.choice([b"0", b"7", b"K"]) if ctx < 0.8 else b""
        return lead + body

    def flips(piece, p):
        if p == 0:
            return piece
        try:
            chars = piece.decode()
        except UnicodeDecodeError:
            return piece
        return "".join(c.swapcase() if rng.random() < p and len(c.swapcase().encode()) == len(c.encode()) else c for c in chars).encode()

    def body_of(target, accept):
        parts, size = [], 0
        while size < target:
            r = rng.random()
            if accept and r < 0.12:
                p = flips(occurrence(), rng.choice([0.0, 0.0, 0.1, 0.3]))
            elif r < 0.45:
                p = near_miss()
            elif r < 0.6 and accept:
                p = prefix(rng.randint(1, max(1, nu - 1))) if nu > 1 else rng.choice(breakers)  # glued on, no breaker: may complete an occurrence
            elif r < 0.8:
                p = rng.choice(breakers) * rng.randint(1, 3)
            else:
                p = rng.choice(delims) + rng.choice([b"", b"Q", b"k"])
            parts.append(p)
            size += len(p)
        return b"".join(parts)[:target]

    def plant(row, end):
        """the needle (letters flipped now and then) written over the row so that the occurrence ends at byte `end`"""
        if end < nb or end > len(row):
            return row
        occ = flips(whole, rng.choice([0.0, 0.0, 0.2]))
        return row[: end - nb] + occ + row[end:]

    def one_row(max_len):
        r = rng.random()
        if r < 0.012:
            return b""
        if r < 0.06:  # lengths around the needle's: the needle itself (an exact match), flipped, one unit short, one byte more on either side
            k = rng.randrange(6)
            return (whole, flips(whole, 0.5), prefix(nu - 1), whole + rng.choice(breakers), rng.choice(delims) + whole, prefix(nu - 1) + rng.choice(breakers))[k][:max_len]
        target = max_len if r < 0.09 else max_len - 1 if r < 0.1 else rng.randint(1, max_len)
        accept = rng.random() < 0.5
        row = body_of(target, accept)
        if accept and rng.random() < 0.55:  # an occurrence that ends on an edge, or straddles it by 1 .. needle - 1 bytes
            edge = rng.choice([e for e in EDGES if e <= len(row) + nb] + [len(row)] * 2)
            end = edge if edge == len(row) or rng.random() < 0.4 else edge + rng.randint(1, max(1, nb - 1))
            row = plant(row, min(end, len(row)) if edge == len(row) else end)
            if rng.random() < 0.5:  # and a second one in another context, before or behind it
                row = plant(row, rng.randint(nb, len(row)) if len(row) >= nb else 0)
        elif accept and len(row) >= 2 * nb + 2 and rng.random() < 0.5:  # two that do not overlap, anywhere
            cut = rng.randint(nb, len(row) - nb - 1)
            row = plant(plant(row, rng.randint(nb, cut)), rng.randint(cut + 1 + nb, len(row)))
        return row

    rows = [one_row(max_len) for _ in range(n_rows)]
    rows[rng.randrange(n_rows)] = body_of(max_len, True)[:max_len].ljust(max_len, b"q")  # the longest haystack decides the view's vector count
    if n_out:
        n_out = min(n_out, max(5, n_rows // 50))  # (a shorter list of the same kind keeps the share)
        for i in rng.sample(range(n_rows), n_out - 5) + [i for i in (0, 1023, 1024, 2047 + 64, n_rows - 1) if i < n_rows]:  # rows beyond 256 bytes, at tile and group boundaries too
            L = rng.choice([257, 258, 272, 300, 511, 512, 513, OUT_MAX]) if rng.random() < 0.4 else rng.randint(257, OUT_MAX)
            row = body_of(L, rng.random() < 0.6)
            if rng.random() < 0.5:  # an occurrence beyond byte 256, at a vector boundary of the outlier kernel or at the row's end
                row = plant(row, rng.choice([len(row), 272, 288 + rng.randint(0, 15), rng.randint(257 + nb, max(257 + nb, len(row)))]))
            rows[i] = row.ljust(257, b"q")
    return rows


def statistics(name, rows, scoring="default", casing="Smart"):
    """what the second transcription says of a list under Substring: (accepted, accepted with two or more occurrences, of those: the reported
    occurrence is not the first) and the per-row result [(score, exact, indices) or None]"""
    lit = Literal(NEEDLES[name][0], "Substring", casing=casing, scoring=SCORINGS[scoring])
    accepted = multi = later = 0
    out = []
    for h in rows:
        got = lit.match_one(h)
        out.append(got)
        if got is None:
            continue
        accepted += 1
        occ = lit.occurrences(h)
        assert occ and got[2][-1] in occ
        if len(occ) >= 2:
            multi += 1
            later += got[2][-1] != occ[0]
    return (accepted, multi, later), out


def conditions_hold(stats, n_rows):
    """the issue's conditions on a list: 10 % .. 80 % accepted; a quarter of those with several occurrences; in 5 % of those not the first reported"""
    accepted, multi, later = stats
    return 0.10 * n_rows <= accepted <= 0.80 * n_rows and 4 * multi >= accepted and 20 * later >= multi
