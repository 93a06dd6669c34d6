"""TEST INFRASTRUCTURE: the inputs of the form-gate tests (tests/test_form_gates_host.py, tests/test_gpu_form_gates.py) - haystacks that push a
scorer's operands as high as a needle and a scoring allow, and the seeded search for the largest score the oracle gives under a scoring.  Plain
Python over the oracle; nothing here imports the library."""
import random

import numpy as np

import form_gates as G
import oracle_lib as O

LETTERS = b"ABCDEFGHIJKLMNOPQRSTUVWXYZ"
LANES = {64: (64, 64, 32), 32: (32, 32, 16), 16: (16, 16, 8)}


def capital_needle(rows):
    """`rows` capital letters: smart case respects them, so every matched letter earns the matching-case bonus"""
    return bytes(LETTERS[i % 26] for i in range(rows))


def windows_of(swl):
    """one, 3/2, two and three chunks, each also plus one byte, and the widest window a thread scores"""
    return sorted({swl, swl + 1, 3 * swl // 2, 3 * swl // 2 + 1, 2 * swl, 2 * swl + 1, 3 * swl, 3 * swl + 1, 1024})


def adversarial(needle, width, lanes, fill=b"_"):
    """windows of exactly `width` bytes (>= len(needle)) whose first byte is the needle's first and whose last byte is its last:
      * the needle in full at the first bytes (prefix bonus, and in the biased domain the largest lane bias) and in full at the last bytes;
      * every needle letter behind a `fill` byte: a delimiter ("_": delimiter bonus) or a lowercase letter ("a": capitalisation bonus);
      * 1, lanes - 1, lanes and lanes + 1 fill bytes between matched letters, the needle in full at the last bytes again.
    width == len(needle) gives the needle itself: the exact match."""
    n = len(needle)
    assert width >= n
    if width == n:
        return [needle]
    out = []

    def fit(body):
        body = (body + fill * width)[:width]
        return body[:width - n] + needle if width >= 2 * n else body[:width - 1] + needle[-1:]

    out.append(fit(needle))
    out.append(fit(fill.join(needle[i:i + 1] for i in range(n))))          # A_B_C: the first letter at byte 0, the others behind a fill byte
    out.append(fit(needle[:1] + b"".join(fill + needle[i:i + 1] for i in range(n))))  # the same after a first match of the prefix
    for gap in (1, lanes - 1, lanes, lanes + 1):
        out.append(fit((fill * gap).join(needle[i:i + 1] for i in range(n))))
    return [h for i, h in enumerate(out) if h not in out[:i]]


def random_windows(rng, needle, width, count):
    """a seeded search on top: windows over aA, aA_ and abAB_/ + the needle's own letters, most of them carrying the needle in order"""
    out = []
    for _ in range(count):
        alpha = rng.choice([b"aA", b"aA_", b"abAB_/ "]) + needle[: rng.randint(0, 3)]
        h = bytearray(rng.choice(alpha) for _ in range(width))
        if rng.random() < 0.8 and width >= len(needle):
            at = sorted(rng.sample(range(width), len(needle)))
            if rng.random() < 0.5:
                at[0] = 0
            for q, c in zip(at, needle):
                h[q] = c
        out.append(bytes(h))
    return out


def random_needle(rng, rows):
    alpha = rng.choice([b"aA", b"aA_", b"abAB_/ "])
    return bytes(rng.choice(alpha) for _ in range(rows))


# ---- the largest score the oracle gives: what fzb_order_flags' bound (score ceiling + exact_match_bonus) must never be below ---------------------------------
_BEST = {}


def best_score_search(sc, rows, seed=7, needles=24, per_needle=160):
    """(best score, needle, haystack) over a seeded search: needles of `rows` bytes and haystacks over aA_ / and space, every haystack scored
    (max_typos=None).  Among the needles are the ones that realise the bound where a scoring allows it: one repeated lowercase letter
    (haystack == needle: match + case per row, prefix, exact) and letters alternating with delimiters."""
    key = (tuple(sc), rows, seed)
    if key in _BEST:
        return _BEST[key]
    rng = random.Random(seed * 1000 + rows)
    alpha = b"aA_ /"
    fixed = [b"a" * rows, b"A" * rows, (b"a_" * rows)[:rows], (b"aA" * rows)[:rows], (b"_a" * rows)[:rows], (b"a/A " * rows)[:rows]]
    best = (-1, b"", b"")
    for k in range(needles):
        needle = fixed[k] if k < len(fixed) else bytes(rng.choice(alpha) for _ in range(rows))
        hs = [needle, b"_" + needle, needle + b"_", b"_".join(needle[i:i + 1] for i in range(rows)), b"a".join(needle[i:i + 1] for i in range(rows))]
        for _ in range(per_needle):
            width = rng.randint(rows, 2 * rows + 6)
            h = bytearray(rng.choice(alpha) for _ in range(width))
            if rng.random() < 0.8:
                for q, c in zip(sorted(rng.sample(range(width), rows)), needle):
                    h[q] = c
            hs.append(bytes(h))
        recs = O.Matcher(needle, scoring=list(sc), max_typos=None, sort="IndexAsc").match_list(hs)
        if len(recs):
            i = int(np.argmax(recs["score"]))
            if int(recs["score"][i]) > best[0]:
                best = (int(recs["score"][i]), needle, hs[int(recs["index"][i])])
    _BEST[key] = best
    return best


def oracle_accepts(needle, sc):
    """the oracle refuses needle and scoring as the reference's overflow guard does; form_gates.overflow_guard_ok must say the same"""
    try:
        O.Matcher(needle, scoring=list(sc))
        ok = True
    except RuntimeError:
        ok = False
    assert ok == G.overflow_guard_ok(sc, len(needle)), (needle, sc, ok)
    return ok


# ---- haystack lists of the GPU tests: the built windows among seeded random ones -----------------------------------------------------------------
def gate_list(kind, needle, sw_lanes, seed, n=1200):
    """`kind`: "short" - every haystack at most sw_lanes / 2 bytes (the short-haystack scorer); "ragged" - single-chunk windows, 65..200 bytes, a few
    of 1024 bytes and one beyond (classes, multi-chunk scorers, the greedy hand-over); "long" - len(needle)..700 bytes with 256 and 257 (long needles)"""
    rng = random.Random(seed)
    rows = len(needle)
    if kind == "short":
        widths = [w for w in range(1, sw_lanes // 2 + 1)]
        special = []
    elif kind == "ragged":
        widths = [w for w in (rows, sw_lanes // 2, sw_lanes - 1, sw_lanes, sw_lanes + 1, 65, 3 * sw_lanes // 2 + 1, 2 * sw_lanes + 1, 3 * sw_lanes + 1, 100, 127, 128, 129, 200) if w >= 1]
        special = [1024, 1024, 1024, 1500]
    else:
        widths = [rows, rows + 1, 200, 255, 256, 257, 300, 511, 513, 700]
        special = []
    hs = []
    for w in widths + special:
        if w >= rows:
            for fill in (b"_", b"a"):
                hs += adversarial(needle, w, sw_lanes, fill)
    while len(hs) < n:
        w = rng.choice(widths)
        hs += random_windows(rng, needle, w, 1) if w >= rows or rng.random() < 0.3 else [bytes(rng.choice(b"aA_/ z") for _ in range(w))]
    rng.shuffle(hs)
    return hs


def ordering_list(needle, best_hay, seed, n=9000):
    """~9000 short haystacks for the ordering gate: long tie groups at the best score (copies of `best_hay`) and at the scores just below it
    (the needle with a suffix, behind a prefix, with one letter's case flipped), spaced letters and seeded random windows"""
    rng = random.Random(seed)
    rows = len(needle)
    flipped = bytes([needle[0] ^ 0x20]) + needle[1:] if needle[:1].isalpha() else needle + b"A"
    variants = [best_hay, needle, needle + b"_z", b"z_" + needle, flipped, b"_".join(needle[i:i + 1] for i in range(rows)), needle[: max(rows - 1, 1)] + b"q" + needle[-1:]]
    hs = []
    for _ in range(n):
        r = rng.random()
        if r < 0.6:
            hs.append(variants[min(int(r * 10), len(variants) - 1)] if r < 0.45 else rng.choice(variants))
        else:
            hs += random_windows(rng, needle, rng.randint(rows, rows + 12), 1)
    return hs
