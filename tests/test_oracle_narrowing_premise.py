"""The premise `frizbee_amd.NarrowingMatcher` rests on, held to the oracle on the CPU: with fuzzy matching and max_typos = 0, every haystack
that matches `needle + suffix` also matches `needle` - the accept decision is "the needle's rows occur in order" (src/prefilter/algo/mod.rs)
and the haystack is long enough, and both only get stricter as the needle grows - so the match set a query captured may be the candidate
set of the next keystroke.  Held for every lane pair, all three casings (Smart going from insensitive to sensitive included), ASCII
needles, and all-unicode needles under unicode=Always.  The class the helper must NOT admit - an ASCII needle extended by a non-ASCII
scalar under unicode=Smart, which moves the matcher from the ASCII automaton to the unicode kernels and their case folding - is shown to
be excluded by the helper's own condition (the two needles report different unicode paths)."""
import json
import os

import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from ref_generators import SwCursor, api_cases
from test_gpu_parity import LANES, _expand

G = os.path.join(os.path.dirname(__file__), "golden")
MT = json.load(open(os.path.join(G, "matcher.json")))
CASINGS = ("Ignore", "Smart", "Respect")


def match_set(needle, hs, lanes, **cfg):
    return set(O.Matcher(needle, lanes=lanes, max_typos=0, sort="IndexAsc", **cfg).match_list(hs)["index"].tolist())


def assert_chain(needle, hs, lanes, **cfg):
    """every prefix chain needle[:1] -> needle[:2] -> .. -> needle: the match sets only shrink; returns how many non-trivial steps there were"""
    steps = 0
    prev = None
    for k in range(1, len(needle) + 1):
        cur = match_set(needle[:k], hs, lanes, **cfg)
        if prev is not None:
            assert cur <= prev, (needle[:k - 1], needle[:k], lanes, cfg, sorted(cur - prev)[:5], [hs[i] for i in sorted(cur - prev)[:3]])
            steps += bool(prev)
        prev = cur
    return steps


def ascii_needles(rng, hs, n):
    """needles drawn as subsequences of the haystacks (so that chains stay non-empty for a while), some letters case-flipped"""
    out = []
    pool = [h for h in hs if 0 < len(h) and all(0 < ord(c) < 128 for c in h)]
    for _ in range(n):
        if not pool:
            break
        h = pool[int(rng.integers(len(pool)))]
        keep = sorted(rng.choice(len(h), size=min(len(h), int(rng.integers(1, 9))), replace=False).tolist())
        s = "".join(h[i] for i in keep)
        out.append("".join(c.swapcase() if rng.random() < 0.2 else c for c in s))
    return out


@pytest.mark.parametrize("pf", sorted(LANES))
@pytest.mark.parametrize("casing", CASINGS)
def test_ascii_needles_over_the_reference_generators(pf, casing):
    rng = np.random.default_rng(pf)
    steps = 0
    for _, hs, _ in api_cases(60, seed=100 + pf):
        if not hs:
            continue
        for needle in ascii_needles(rng, hs, 3):
            steps += assert_chain(needle, hs, LANES[pf], casing=casing)
    assert steps > 100  # (chains whose shorter needle matched something: the property had something to say)


@pytest.mark.parametrize("pf", sorted(LANES))
@pytest.mark.parametrize("casing", CASINGS)
def test_ascii_needles_over_the_golden_lists(pf, casing):
    steps = 0
    for case in MT["cases"]:
        needle = case["needle"]
        if not needle or any(ord(c) >= 128 or ord(c) == 0 for c in needle):
            continue
        steps += assert_chain(needle, _expand(case["haystacks"]), LANES[pf], casing=casing)
    assert steps > 10


@pytest.mark.parametrize("pf", sorted(LANES))
@pytest.mark.parametrize("casing", CASINGS)
def test_unicode_needles_with_unicode_always(pf, casing):
    rng = np.random.default_rng(7 * pf)
    steps = 0
    for k in range(40):
        c = SwCursor(rng.integers(0, 256, 512).tolist())
        hs = ["".join(c.unicode_char() for _ in range(c.len(48, [0, 1, 2, 7, 8, 15, 16, 31, 32, 48]))) for _ in range(24)]
        pool = [h for h in hs if h and "\0" not in h]
        for _ in range(3):
            h = pool[int(rng.integers(len(pool)))]
            keep = sorted(rng.choice(len(h), size=min(len(h), int(rng.integers(1, 7))), replace=False).tolist())
            needle = "".join(h[i] for i in keep)
            steps += assert_chain(needle, hs, LANES[pf], casing=casing, unicode="Always")
    assert steps > 100


def test_the_excluded_class_changes_the_unicode_path():
    """ASCII needle + a non-ASCII scalar under unicode=Smart: the helper compares fzb_matcher_info's unicode path (and lane pair) of the two
    needles and refuses to narrow - shown here on the info alone (host work, no device)."""
    for pf in sorted(LANES):
        cfg = F.Config(pf_lanes=pf, sw_lanes=0, unicode=F.UnicodeMatching.Smart)
        for a, b in (("k", "ké"), ("dead", "deadK"), ("src", "srcß")):
            ia, ib = F.Matcher(a, cfg).info(), F.Matcher(b, cfg).info()
            assert not ia["unicode"] and ib["unicode"], (a, b, ia, ib)
    # and the helper's own decision, without a device: the condition is evaluated before anything is launched
    nm = F.NarrowingMatcher.__new__(F.NarrowingMatcher)
    nm.config = F.Config()
    nm.max_fraction = 1.0
    nm._cur, nm._prev = 0, (b"dead", (False, 64, 64), 0)

    class Gen:
        def generation(self):
            return 0

        def __len__(self):
            return 10

    nm.corpus = Gen()
    assert nm._may_narrow("deadK".encode(), (True, 64, 64)) is False   # another unicode path
    assert nm._may_narrow(b"deadb", (False, 64, 32)) is False               # another lane pair
    assert nm._may_narrow(b"dea", (False, 64, 64)) is False                 # not an extension
    assert nm._may_narrow(b"dead", (False, 64, 64)) is False                # an empty suffix
    nm.config = F.Config(max_typos=1)
    assert nm._may_narrow(b"deadb", (False, 64, 64)) is False               # typos
    nm.config = F.Config(matching=F.Matching.Substring)
    assert nm._may_narrow(b"deadb", (False, 64, 64)) is False               # a literal mode
