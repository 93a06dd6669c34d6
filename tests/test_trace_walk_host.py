"""frizbee_amd/csrc/trace_walk.h - the walk back through the score / match matrices that lane 0 of the traced scorer runs for
`match_list_indices` - compiled for the host and held to the oracle's walk.  Three independent pieces meet here: the matrices come from the
second transcription's forward pass (tests/sw_second_transcription.py), packed into the kernel's cells layout; the walk under test is the
device header's; the expected positions are `fzo_sw_indices`', the oracle's restatement of score_haystack[_unicode]_indices
(src/smith_waterman/algo/mod.rs:49-152, alignment_iter.rs:35-181).  The walk's decisions are tie-breaks and typo counts, and whether a
tie occurs depends on the scoring constants - hence every scoring of the ISA fuzz and random ones, at every lane width of both classes."""
import numpy as np
import pytest

import oracle_lib as O
import sw_second_transcription as T2
import trace_host_lib as TW
from test_gpu_fuzz_isa import SCORINGS as ISA_SCORINGS  # definitions only: nothing there touches the GPU at import

pytestmark = pytest.mark.skipif(not TW.available(), reason="ROCm clang++ not installed")

DEFAULT = list(O.DEFAULT_SCORING)
SCORINGS = [list(sc) for sc, _ in ISA_SCORINGS]  # the default, then the nine others
assert SCORINGS[0] == DEFAULT and len(SCORINGS) == 10
WIDTHS = [(8, False), (16, False), (32, False), (16, True), (32, True), (64, True)]  # (lanes, u8 class): what the three backend pairs select
TYPOS = [None, 0, 1, 3]


def random_scoring(rng):
    return [int(rng.integers(1, 17)), int(rng.integers(0, 9)), int(rng.integers(0, 9)), int(rng.integers(0, 4)), int(rng.integers(0, 17)),
            int(rng.integers(0, 9)), int(rng.integers(0, 9)), int(rng.integers(0, 17)), int(rng.integers(0, 9))]


def pick_scoring(rng, it):
    """default : the nine others : random = 1 : 2 : 1"""
    k = it % 4
    if k == 0:
        return DEFAULT
    if k == 3:
        return random_scoring(rng)
    return SCORINGS[1 + (it // 4 * 2 + k - 1) % 9]


def widths_for(it, nrows, scoring):
    """two of the six (lanes, class) pairs per input, rotating; the u8 class only where the reference would select it"""
    out = []
    for k in range(6):
        lanes, u8 = WIDTHS[(it + k) % 6]
        if u8 and not O.score_fits_in_u8(nrows, scoring):
            continue
        out.append((lanes, u8))
        if len(out) == 2:
            break
    return out


def run_window(needle, window, scoring, cs, start_pos, lanes, u8, unicode, stats):
    """one forward pass, then the device header's walk at every typo budget against the oracle's -> whether the window scored"""
    bits = 8 if u8 else 16
    mats = {}
    if unicode:
        score = T2.score_haystack_unicode(needle, window, scoring, cs, start_pos == 0, lanes, bits, mats)
        rows, ulen = len(needle), [len(c.encode()) for c in needle]
    else:
        score = T2.score_haystack(needle, window, scoring, cs, start_pos == 0, lanes, bits, mats)
        rows, ulen = len(needle), None
    nbytes = len(O._b(needle))
    cells = nchunks = None
    for mt in TYPOS:
        ctx = (needle, window, scoring, cs, start_pos, lanes, u8, mt)
        wscore, want = O.sw_indices(needle, window, start_pos=start_pos, unicode=unicode, max_typos=mt, scoring=scoring, case_sensitive=cs, lanes=lanes, is_u8=u8)
        assert wscore == score, ctx
        if score == 0:  # the kernel does not walk a window that did not score
            assert want == [], ctx
            continue
        if cells is None:
            cells, nchunks = TW.pack_cells(mats, rows, lanes)
        got, guard = TW.walk(cells, nchunks, rows, lanes, unicode, score, mt, window, start_pos, ulen, stride=nbytes)  # the kernel's stride: the needle's bytes
        assert got == want, ctx + (got, want)
        assert all(g == 0xA5A5A5A5 for g in guard), ctx
        assert TW.POISON not in got, ctx
        if mt is None:
            stats["full" if len(want) == nbytes else "partial" if want else "empty"] += 1
    if score:
        stats["windows"] += 1
        stats["multi_chunk"] += nchunks > 1
        stats[(lanes, u8)] = stats.get((lanes, u8), 0) + 1
    return score != 0


def new_stats():
    return dict(windows=0, multi_chunk=0, full=0, partial=0, empty=0)


def test_ascii_walk_against_the_oracle():
    rng = np.random.default_rng(20_000)
    alpha = b"abcABC_-/ 01xyz"
    lengths = [1, 3, 7, 8, 9, 12, 15, 16, 17, 24, 31, 32, 33, 40, 64, 65, 100]
    stats = new_stats()
    it = 0
    while stats["windows"] < 20_000:
        asz = int(rng.integers(2, len(alpha) + 1))
        needle = bytes(alpha[int(x)] for x in rng.integers(0, asz, int(rng.integers(1, 9))))
        hay = bytearray(alpha[int(x)] for x in rng.integers(0, asz, int(rng.choice(lengths))))
        if rng.random() < 0.7 and len(hay) >= len(needle):
            for q, c in zip(np.sort(rng.choice(len(hay), len(needle), replace=False)), needle):
                hay[q] = c
        scoring = pick_scoring(rng, it)
        cs = bool(rng.integers(0, 2))
        start_pos = int(rng.integers(0, 3))
        for lanes, u8 in widths_for(it, len(needle), scoring):
            run_window(needle, bytes(hay), scoring, cs, start_pos, lanes, u8, False, stats)
        it += 1
        assert it < 60_000, stats  # the generator, not the walk, would be at fault
    assert all(stats.get(w, 0) >= 1_500 for w in WIDTHS), stats  # every lane width of both classes
    assert stats["multi_chunk"] >= 4_000 and min(stats["full"], stats["partial"]) >= 2_000, stats


def test_unicode_walk_against_the_oracle():
    rng = np.random.default_rng(8_000)
    # one- to four-byte scalars; é / É, ж / Ж, a / A: case-folded matches of equal byte length
    alpha = ["a", "b", "A", "B", "_", " ", "/", "é", "É", "ß", "ж", "Ж", "다", "라", "😀", "1"]
    stats = new_stats()
    cont_runs = 0
    it = 0
    while stats["windows"] < 8_000:
        asz = int(rng.integers(3, len(alpha) + 1))
        needle = "".join(alpha[int(x)] for x in rng.integers(0, asz, int(rng.integers(1, 7))))
        hay = [alpha[int(x)] for x in rng.integers(0, asz, int(rng.choice([1, 3, 7, 8, 12, 15, 16, 17, 24, 30, 33, 40])))]
        if rng.random() < 0.7 and len(hay) >= len(needle):
            for q, c in zip(np.sort(rng.choice(len(hay), len(needle), replace=False)), needle):
                hay[q] = c if rng.random() < 0.8 else c.swapcase() if len(c.swapcase().encode()) == len(c.encode()) else c
        hay = [c.encode() for c in hay]
        if it % 4 == 0:  # runs of continuation bytes that belong to no scalar: the walk steps left over every one of them
            for _ in range(int(rng.integers(1, 4))):
                hay.insert(int(rng.integers(0, len(hay) + 1)), bytes(int(x) for x in rng.integers(0x80, 0xC0, int(rng.integers(1, 6)))))
            cont_runs += 1
        window = b"".join(hay)
        scoring = pick_scoring(rng, it)
        cs = bool(rng.integers(0, 2))
        start_pos = int(rng.integers(0, 3))
        for lanes, u8 in widths_for(it, len(needle), scoring):
            run_window(needle, window, scoring, cs, start_pos, lanes, u8, True, stats)
        it += 1
        assert it < 30_000, stats
    assert all(stats.get(w, 0) >= 500 for w in WIDTHS), stats
    assert stats["multi_chunk"] >= 1_500 and min(stats["full"], stats["partial"]) >= 800 and cont_runs >= 500, stats


def test_nothing_is_written_past_the_stride():
    # more positions available than the caller has room for: the first `stride` of them, the words behind untouched
    sc = DEFAULT
    for needle, window, unicode in ((b"abcdef", b"xxabc_def", False), ("é다a", "_é다a".encode(), True), ("😀😀", "😀😀".encode(), True)):
        rows = len(needle)
        ulen = [len(c.encode()) for c in needle] if unicode else None
        for lanes in (8, 16, 32, 64):
            mats = {}
            score = (T2.score_haystack_unicode if unicode else T2.score_haystack)(needle, window, sc, False, True, lanes, 16, mats)
            _, want = O.sw_indices(needle, window, unicode=unicode, lanes=lanes)
            assert len(want) == len(O._b(needle))
            cells, nchunks = TW.pack_cells(mats, rows, lanes)
            for stride in range(0, len(want) + 2):
                got, guard = TW.walk(cells, nchunks, rows, lanes, unicode, score, None, window, 0, ulen, stride=stride)
                assert got == want[:stride], (needle, lanes, stride, got, want)
                assert all(g == 0xA5A5A5A5 for g in guard), (needle, lanes, stride, guard)


# the smallest window of the runs above on which ONE decision of the walk decides the positions: each stops agreeing with the oracle when
# that decision is changed (needle, window, scoring, case_sensitive, start_pos, lanes, u8 class, unicode)
NAMED = [
    ("diagonal >= left", b"aabbbbb", b"bab", [1, 0, 6, 2, 14, 7, 5, 7, 4], False, 2, 16, True, False),
    ("diagonal >= up", b"accb", b"aab", DEFAULT, False, 1, 32, True, False),
    ("left >= up", b"abaabbc", b"aca", [5, 0, 8, 0, 13, 5, 7, 7, 7], True, 2, 64, True, False),
    ("a move up is a typo", b"--0", b"-", [9, 8, 0, 1, 8, 2, 3, 14, 4], True, 2, 64, True, False),
    ("a mismatch is a typo", b"cAb", b"A", [9, 2, 7, 0, 1, 7, 5, 12, 6], True, 0, 16, True, False),
    ("the budget is exceeded, not reached", b"-", b"-", [1, 1, 1, 0, 0, 0, 0, 0, 0], True, 0, 16, True, False),
    ("continuation bytes are stepped over", "_A_ééb", "__A_éBÉB".encode(), [1, 1, 1, 0, 0, 0, 0, 0, 0], True, 0, 16, True, True),
]


@pytest.mark.parametrize("case", NAMED, ids=[c[0] for c in NAMED])
def test_named_windows(case):
    _, needle, window, scoring, cs, start_pos, lanes, u8, unicode = case
    assert run_window(needle, window, scoring, cs, start_pos, lanes, u8, unicode, new_stats())
