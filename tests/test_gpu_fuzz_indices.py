"""Bulk differential fuzz of MATCHED POSITIONS: `Matcher.match_list_indices` - answered by one kernel, the traced instantiation
k2c_generic<SWL, UNICODE, TRACE = true, ..> (kernels_generic.hip): score / match matrices in HBM, the ballot search for the first column
of the last row that holds the score, the in-kernel 0-typo window, lane 0's walk back (trace_walk.h), the greedy positions beyond 1024
bytes - against the oracle's `match_list_indices_ordered`, record for record: (index, score, exact, positions).  The walk's decisions are
tie-breaks and typo counts, and whether a tie occurs depends on the scoring constants: under the default scoring the rarest slip of the
walk is decided by one window in two thousand, under the ten scorings of the ISA fuzz in turn by one in forty.  So: every scoring x every
needle x every typo budget per lane width, and the long-needle forms on both sides of the LDS / slab line.  tests/test_trace_walk_host.py
holds the same walk to the oracle on the host; this file is the kernel around it, as compiled for gfx950.

Every test counts, on the ORACLE's side of the comparison, what keeps it from passing vacuously: records with a position for every needle
byte, with some, with none, records from haystacks wider than one chunk and from haystacks beyond 1024 bytes."""
import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from test_gpu_fuzz_isa import DEFAULT, LANE_TRIPLES, NEEDLES, SCORINGS, make_list, make_unicode_list

pytestmark = pytest.mark.gpu

SORTS = ["ScoreThenIndexAsc", "ScoreThenIndexDesc", "IndexAsc", "IndexDesc"]
UNICODE_SCORINGS = (SCORINGS[0], SCORINGS[1], SCORINGS[2], SCORINGS[4], SCORINGS[5], SCORINGS[6])  # the six of the unicode ISA fuzz


def unpack(data, ends):
    raw = data.tobytes()
    e = [0] + [int(x) for x in ends]
    return [raw[e[i] : e[i + 1]] for i in range(len(ends))]


class Tally:
    """what the oracle's records say about the inputs (nothing here looks at the GPU's answer)"""

    def __init__(self):
        self.haystacks = self.records = self.full = self.partial = self.empty = self.multi_chunk = self.beyond_1024 = 0

    def add(self, nbytes, hs, want, sw_lanes):
        self.haystacks += len(hs)
        self.records += len(want)
        for index, _, _, ix in want:
            n = len(hs[index])
            self.full += len(ix) == nbytes
            self.partial += 0 < len(ix) < nbytes
            self.empty += not ix
            self.multi_chunk += n > sw_lanes
            self.beyond_1024 += n > 1024

    def report(self):
        r = max(self.records, 1)
        return (f"haystacks {self.haystacks} records {self.records} full {self.full} ({100 * self.full / r:.1f} %) partial {self.partial} ({100 * self.partial / r:.1f} %) "
                f"empty {self.empty} ({100 * self.empty / r:.1f} %) multi-chunk {self.multi_chunk} beyond-1024 {self.beyond_1024}")

    def assert_not_vacuous(self, tag, beyond_1024=200):
        print(tag, self.report())
        assert self.full >= 0.20 * self.records, (tag, self.report())
        assert self.partial >= 0.20 * self.records, (tag, self.report())
        assert self.empty >= 0.05 * self.records, (tag, self.report())
        assert self.multi_chunk >= 1000, (tag, self.report())
        assert self.beyond_1024 >= beyond_1024, (tag, self.report())


def oracle_side(needle, hs, lanes, tally, sub=None, **cfg):
    """-> (the oracle's ordered records over `hs` (or over the sub-list `sub` selects), the oracle's matcher)"""
    om = O.Matcher(needle, lanes=LANE_TRIPLES[lanes], **cfg)
    lst = hs if sub is None else [hs[int(i)] for i in sub]
    want = om.match_list_indices_ordered(lst)
    tally.add(len(O._b(needle)), lst, want, om.info()["sw_lanes"])
    return want, om


def gpu_matcher(needle, lanes, om, **cfg):
    fc = F.Config(max_typos=cfg.get("max_typos", 0), scoring=F.Scoring(*cfg.get("scoring", DEFAULT)), pf_lanes=LANE_TRIPLES[lanes][0], sort=F.SortStrategy[cfg.get("sort", "ScoreThenIndexAsc")],
                  unicode=F.UnicodeMatching[cfg.get("unicode", "Smart")], casing=F.CaseMatching[cfg.get("casing", "Smart")])
    fm = F.Matcher(needle, fc)
    assert fm.info()["use_u8"] == om.info()["use_u8"] and fm.info()["sw_lanes"] == om.info()["sw_lanes"], (needle, cfg)
    return fm


def report_difference(tag, got, want, lst):
    """as test_gpu_fuzz_isa.check: the tag, the first differing record from both sides, the haystack bytes"""
    bad = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    rec = want[bad] if bad < len(want) else got[bad]
    raise AssertionError((tag, "records", len(got), len(want), "first difference at", bad, "got", got[bad : bad + 1], "want", want[bad : bad + 1], "haystack", lst[rec[0]]))


def compare(tag, needle, hs, lanes, tally, corpus=None, selection=None, **cfg):
    want, om = oracle_side(needle, hs, lanes, tally, sub=selection, **cfg)
    fm = gpu_matcher(needle, lanes, om, **cfg)
    got = [(m.index, m.score, m.exact, m.indices) for m in fm.match_list_indices(corpus if corpus is not None else F.Corpus(hs), selection)]
    if got != want:
        report_difference(tag, got, want, hs if selection is None else [hs[int(i)] for i in selection])
    return fm


ASCII_POOLS = {
    "short": np.array([0, 1, 3, 6, 8, 12, 16, 20, 27, 31, 32]),
    "chunk": np.array([0, 5, 16, 31, 32, 33, 40, 47, 48, 49, 63, 64]),
    # the ISA fuzz's ragged pool + haystacks beyond 1024 bytes (whole-haystack and typo windows there: match_greedy's positions)
    "ragged": np.array([2, 9, 30, 33, 64, 65, 70, 100, 127, 128, 129, 200, 300, 1025, 1400, 2000]),
}
ASCII_PER_CONFIG = 700


def ascii_cases(lanes, per_config=ASCII_PER_CONFIG):
    """every scoring x every needle x max_typos 0 (window found in the kernel, wmode 1) / 1 / 2 (window kernel, wmode 0) / None (whole
    haystack, wmode 2); casing, the sort strategy (the ordering step runs on the host) and the length pool rotate"""
    rng = np.random.default_rng(4000 + lanes)
    k = 0
    for si, (sc, what) in enumerate(SCORINGS):
        for ni, needle in enumerate(NEEDLES):
            for typos in (0, 1, 2, None):
                if typos in (1, 2) and len(needle) <= typos:
                    continue
                pool = ("short", "chunk", "ragged")[(si + ni + (typos or 0)) % 3]
                casing = ("Smart", "Respect")[(si + ni + k) % 2]
                sort = SORTS[k % 4]
                k += 1
                data, ends = make_list(rng, needle, per_config, ASCII_POOLS[pool])
                yield (lanes, what, needle, typos, pool, casing, sort), needle, unpack(data, ends), dict(max_typos=typos, scoring=sc, casing=casing, sort=sort)


@pytest.mark.parametrize("lanes", [64, 32, 16])
def test_ascii_positions_every_scoring_every_needle(lanes):
    tally = Tally()
    for tag, needle, hs, cfg in ascii_cases(lanes):
        compare(tag, needle, hs, lanes, tally, **cfg)
    assert tally.haystacks >= 250_000, tally.report()
    tally.assert_not_vacuous(("ascii", lanes))


UNICODE_NEEDLES = ["إنما", "éa", "中文字", "aЖ", "😀é", "é", "fBr"]  # the last one ASCII: scored by the unicode kernel under UnicodeMatching.Always
UNICODE_PER_CONFIG = 520


def with_continuation_runs(rng, hs, needle):
    """every fifth row gets runs of continuation bytes that belong to no scalar, between its scalars (the walk steps left over them);
    every sixth row loses the needle's scalars, either case (under max_typos None it is still a record: one without positions)"""
    out = []
    gone = set(needle) | set(needle.upper()) | set(needle.lower())
    for i, h in enumerate(hs):
        if i % 6 == 1:
            h = "".join("-" if c in gone else c for c in h.decode()).encode()
        if i % 5 == 0:
            chars = [c.encode() for c in h.decode()]
            for _ in range(int(rng.integers(1, 4))):
                chars.insert(int(rng.integers(0, len(chars) + 1)), bytes(int(x) for x in rng.integers(0x80, 0xC0, int(rng.integers(1, 6)))))
            h = b"".join(chars)
        out.append(h)
    return out


def unicode_cases(lanes, per_config=UNICODE_PER_CONFIG):
    rng = np.random.default_rng(5000 + lanes)
    k = 0
    for sc, what in UNICODE_SCORINGS:
        for needle in UNICODE_NEEDLES:
            for typos in (0, 1, None):
                if typos and len(needle) <= typos:
                    continue
                ascii_needle = needle.isascii()
                mode = "Always" if ascii_needle or k % 2 else "Smart"
                max_chars = (14, 60, 30, 120, 600)[k % 5]  # up to 4 bytes a scalar: windows of one chunk, of several, and a few rows beyond 1024 bytes
                sort = SORTS[k % 4]
                k += 1
                data, ends = make_unicode_list(rng, needle, per_config, max_chars)
                hs = with_continuation_runs(rng, unpack(data, ends), needle)
                yield (lanes, what, needle, typos, mode, max_chars, sort), needle, hs, dict(max_typos=typos, scoring=sc, unicode=mode, sort=sort)


@pytest.mark.parametrize("lanes", [64, 32, 16])
def test_unicode_positions(lanes):
    tally = Tally()
    for tag, needle, hs, cfg in unicode_cases(lanes):
        compare(tag, needle, hs, lanes, tally, **cfg)
    assert tally.haystacks >= 60_000, tally.report()
    tally.assert_not_vacuous(("unicode", lanes))


def rand_text(rng, n, alpha):
    return bytes(alpha[int(x)] for x in rng.integers(0, len(alpha), n))


def long_haystacks(rng, needle, count, alpha):
    """100 .. 1100 bytes (a few beyond 1024) that carry most of the needle in order: all of it in half of the rows (what a 0-typo query
    keeps), 85 - 99 % in the others; + the needle itself, in other case, doubled, and embedded without gaps"""
    n = len(needle)
    hs = [needle, needle.swapcase(), needle + needle, alpha[:1] * 40 + needle + alpha[1:2] * 40, needle[: n // 2], b""]
    for i in range(count):
        L = int(rng.integers(max(100, n + 10), 1101)) if i % 12 else int(rng.integers(1025, 1600))
        body = bytearray(rand_text(rng, L, alpha))
        at = np.sort(rng.choice(L, n, replace=False))
        keep = np.ones(n, bool) if i % 2 else rng.random(n) < rng.uniform(0.85, 0.99)
        if i % 3 == 0:  # most of it without gaps: long diagonal runs, then a ragged tail
            run = int(rng.integers(n // 2, n))
            at[:run] = at[0] % (L - n) + np.arange(run)
            at[run:] = np.sort(rng.choice(np.arange(at[run - 1] + 1, L), n - run, replace=False))
        for q, ch, kp in zip(at, needle, keep):
            if kp:
                body[int(q)] = ch
        hs.append(bytes(body))
    return hs


def takes_the_slab(info):
    """fzb_launch_generic_long keeps the previous-chunk vectors in LDS while 16 x (rows + 1) x sw_lanes <= 60 KiB, in the global slab beyond"""
    return 16 * (info["rows"] + 1) * info["sw_lanes"] > 60 * 1024


def long_needle_cases():
    """(pf, needle, haystacks, scoring): needles on both sides of the LDS / slab line - 119 | 120 rows at the 32 lanes of the u16 class at
    pf 64; the u8 class (64 lanes) takes the slab from 60 rows on; at pf 16 (8 lanes) the line is at 480 rows"""
    rng = np.random.default_rng(6000)
    alpha = b"abcdefgh_/AB"
    for pf in (64, 16):
        for n in (70, 119, 120, 121, 160, 230) + ((500,) if pf == 16 else ()):
            needle = rand_text(rng, n, b"abcdefgh_/")
            yield pf, needle, long_haystacks(rng, needle, 100 if n < 500 else 40, alpha), DEFAULT
        needle = rand_text(rng, int(rng.integers(70, 101)), b"abcdef")
        yield pf, needle, long_haystacks(rng, needle, 100, b"abcdefAB_"), [1, 1, 1, 0, 0, 0, 0, 0, 0]  # u8 class whatever the length
        ualpha = list("éàüñабвгд中文字abc_ ")
        uneedle = "".join(ualpha[int(x)] for x in rng.integers(0, len(ualpha), 130))
        uhs = [uneedle, uneedle.upper(), "", "__" + uneedle + "--"]
        for i in range(60):
            out = []
            for ch in uneedle:
                r = rng.random()
                if i % 2 and r < 0.03:
                    continue
                out.append(ch if r > 0.06 or not i % 2 else ualpha[int(rng.integers(0, len(ualpha)))])
                if rng.random() < 0.3:
                    out.extend(ualpha[int(x)] for x in rng.integers(0, len(ualpha), int(rng.integers(1, 6))))
            uhs.append("".join(out))
        yield pf, uneedle, [h.encode() for h in uhs], DEFAULT


def test_long_needle_positions_on_both_sides_of_the_slab_line():
    tallies = {64: Tally(), 16: Tally()}
    sides = {64: set(), 16: set()}
    for pf, needle, hs, sc in long_needle_cases():
        cp = F.Corpus(hs)
        for typos in (0, 1, None):
            fm = compare((pf, len(needle), sc, typos), needle, hs, pf, tallies[pf], corpus=cp, max_typos=typos, scoring=sc, sort="IndexAsc")
            info = fm.info()
            assert info["rows"] > 63  # NeedleLongDev
            sides[pf].add((takes_the_slab(info), info["unicode"], info["use_u8"]))
    for pf in (64, 16):
        print(("long", pf), tallies[pf].report(), sorted(sides[pf]))
        for slab in (False, True):  # both sides of the line ran, at this lane triple
            assert any(s[0] == slab for s in sides[pf]), (pf, sides[pf])
        assert tallies[pf].full >= 200 and tallies[pf].partial >= 200 and tallies[pf].beyond_1024 >= 20, tallies[pf].report()
    s64 = sides[64]
    assert (True, False, False) in s64 and (False, False, False) in s64 and (True, False, True) in s64 and (True, True, False) in s64, s64  # ASCII u16 on both sides, u8 slab, unicode slab


@pytest.mark.parametrize("lanes", [64, 32, 16])
def test_selection_over_a_resident_corpus(lanes):
    # a permuted selection with repeats and entries that do not match, against the oracle on the selected sub-list
    rng = np.random.default_rng(7000 + lanes)
    tally = Tally()
    sc = SCORINGS[6][0]
    for needle, typos, pool in ((b"deadbe", 1, "ragged"), (b"fBr", 0, "chunk"), (b"x_y", None, "ragged")):
        data, ends = make_list(rng, needle, 6000, ASCII_POOLS[pool])
        hs = unpack(data, ends)
        cp = F.Corpus(packed=(data, ends))
        sel = rng.permutation(len(hs))[:2500]
        sel = np.concatenate([sel, sel[:300], rng.integers(0, len(hs), 200)]).astype(np.uint32)
        rng.shuffle(sel)
        compare((lanes, "selection", needle, typos), needle, hs, lanes, tally, corpus=cp, selection=sel, max_typos=typos, scoring=sc, sort=SORTS[lanes % 3])
    print(("selection", lanes), tally.report())
    assert tally.records >= 1000 and tally.full >= 200 and tally.partial >= 200 and tally.haystacks > tally.records, tally.report()


@pytest.mark.parametrize("lanes", [64, 32, 16])
def test_multi_pattern_positions_under_other_scorings(lanes):
    rng = np.random.default_rng(8000 + lanes)
    alpha = "abcAB_ /xé"
    records = with_positions = 0
    for it in range(40):
        sc = (SCORINGS[2][0], SCORINGS[6][0], SCORINGS[9][0])[it % 3]
        words = ["".join(alpha[int(x)] for x in rng.integers(0, 7, int(rng.integers(1, 4)))) for _ in range(int(rng.integers(1, 4)))]
        query = " ".join(("!" if rng.random() < 0.25 else "") + ["", "^", "'"][int(rng.integers(0, 3))] + w for w in words)
        hs = ["".join(alpha[int(x)] for x in rng.integers(0, len(alpha), int(rng.integers(0, 90)))) for _ in range(300)]
        sort, typos = SORTS[it % 4], [0, 1, None][it % 3]
        om = O.MultiMatcher(O.parse_query(query), lanes=LANE_TRIPLES[lanes], sort=sort, max_typos=typos, scoring=sc)
        fm = F.MultiMatcher(F.parse_query(query), F.Config(max_typos=typos, sort=F.SortStrategy[sort], scoring=F.Scoring(*sc), pf_lanes=LANE_TRIPLES[lanes][0]))
        want = om.match_list_indices_ordered(hs)
        got = [(m.index, m.score, m.exact, m.indices) for m in fm.match_list_indices(hs)]
        if got != want:
            report_difference((lanes, "multi", query, sc, sort, typos), got, want, hs)
        records += len(want)
        with_positions += sum(1 for w in want if w[3])
    print(("multi", lanes), "records", records, "with positions", with_positions)
    assert records >= 1000 and with_positions >= 500, (records, with_positions)
