"""frizbee_amd/csrc/sections.h on the CPU: the decisions of the sectioned top-`limit` stage, compiled for the host
(tests/kernel_host/sections_host.cpp walks the stage through the functions the kernels call) and fuzzed against numpy: membership masks,
the whole walk - histograms, cuts, tile counts, scans, destinations, ranks - and the rank function against np.lexsort."""
import subprocess

import numpy as np
import pytest

import sections_host_lib as H

pytestmark = pytest.mark.skipif(not H.available(), reason="ROCm's clang++ is not installed")

SORTS = ((True, False), (True, True), (False, False), (False, True))  # (by_score, desc): ScoreThenIndexAsc / Desc, IndexAsc / Desc
SECTIONS = [(1, 0), (2, 1), (0, 0), (0xF0, 0), (1, 1), (1, 0), (0xFFF, 0), (0, 0x8000)]  # overlapping, a duplicate, empty ones


def records(rng, n_hay, n, scores):
    idx = np.sort(rng.choice(n_hay, size=n, replace=False)).astype(np.uint32)
    recs = np.zeros(n, H.REC)
    recs["index"] = idx
    recs["score"] = scores
    recs["exact"] = rng.integers(0, 2, n)
    recs["_pad"] = 1
    return recs


def score_sets(rng, n):
    return {
        "below 256": (rng.integers(0, 256, n), True),
        "both sides of 256": (rng.integers(0, 700, n), False),
        "heavy ties": (rng.choice([96, 96, 96, 300, 0], n), False),
        "all equal, one level": (np.full(n, 96), True),
        "wide": (rng.integers(0, 65536, n), False),
        "clamped": (np.clip(rng.integers(-300, 400, n), 0, None), False),
    }


def check(recs, tags, sections, limit, by_score, desc, one_pass, what):
    heads, found, cuts = H.walk(recs, tags, sections, limit, by_score, desc, one_pass)
    rec_tags = tags[recs["index"]] if tags is not None else np.zeros(len(recs), np.uint16)
    want, want_found = H.model(recs, rec_tags, sections, limit, by_score, desc)
    assert found == want_found, (what, found, want_found)
    for s in range(len(sections)):
        assert heads[s].tolist() == want[s].tolist(), (what, s, sections[s], limit, cuts[s].tolist())
    return heads, found, cuts


def test_the_limits_are_the_headers():
    import re, os
    header = open(os.path.join(H.ROOT, "include", "frizbee_hip.h")).read()
    assert int(re.search(r"#define FZB_SECTIONS_MAX (\d+)", header).group(1)) == H.lib().sec_sections_max() == 8
    assert int(re.search(r"#define FZB_SECTION_LIMIT_MAX (\d+)", header).group(1)) == H.lib().sec_limit_max() == 1024
    assert H.lib().sec_tile() == 2048 and H.lib().sec_state_words() == 16


def test_membership_masks():
    rng = np.random.default_rng(1)
    tags = np.concatenate([rng.integers(0, 65536, 5000), [0, 0xFFFF, 0x8000, 1, 2, 3]]).astype(np.uint16)
    for trial in range(20):
        S = int(rng.integers(0, 9))
        sections = [(int(rng.integers(0, 65536)) & int(rng.integers(0, 65536)) & int(rng.integers(0, 65536)), int(rng.integers(0, 65536)) & int(rng.integers(0, 65536)) & int(rng.integers(0, 65536)))
                    for _ in range(S)]
        if S > 2:
            sections[1] = (0, 0)
            sections[2] = sections[0]
        got = H.masks(tags, sections)
        want = np.zeros(len(tags), np.uint32)
        for s, (r, e) in enumerate(sections):
            want |= H.member(tags, r, e).astype(np.uint32) << s
        assert got.tolist() == want.tolist(), sections
    assert H.masks(tags, SECTIONS)[-6:].tolist() == [0b10000100, 0b01101101, 0b00000100, 0b10100101, 0b10000110, 0b10100101]  # worked out by hand


def test_rank_against_lexsort():
    rng = np.random.default_rng(2)
    for kept in (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 1024):
        for name, (scores, _) in score_sets(rng, kept).items():
            slab = np.zeros(kept, H.REC)
            slab["index"] = np.arange(kept) * 3
            slab["score"] = scores
            pos = np.arange(kept)
            for by_score, desc in SORTS:
                got = H.ranks(slab, by_score, desc)
                keys = (-pos if desc else pos, -slab["score"].astype(np.int64) if by_score else np.zeros(kept, np.int64))
                order = np.lexsort(keys)  # order[r] = the position that goes to rank r
                want = np.empty(kept, np.int64)
                want[order] = np.arange(kept)
                assert got.tolist() == want.tolist(), (kept, name, by_score, desc)


def test_every_limit_through_the_whole_walk():
    """limit 0 .. 1024, each once, the sorts and the score sets taking turns; lists of several tiles with a ragged last one"""
    rng = np.random.default_rng(3)
    n_hay, n = 9000, 5000  # (three tiles of 2048, the last one ragged)
    tags = rng.integers(0, 65536, n_hay).astype(np.uint16)
    sets = score_sets(rng, n)
    lists = {name: (records(rng, n_hay, n, scores), one_pass) for name, (scores, one_pass) in sets.items()}
    names = sorted(lists)
    seen_cut_ties = seen_keep_all = seen_empty = seen_two_bins = 0
    for limit in range(0, 1025):
        name = names[limit % len(names)]
        by_score, desc = SORTS[(limit // len(names)) % 4]
        recs, one_pass = lists[name]
        _, found, cuts = check(recs, tags, SECTIONS, limit, by_score, desc, one_pass and by_score, (name, limit, by_score, desc))
        seen_empty += found[4] == 0
        if by_score and limit:
            live = [s for s in range(8) if not cuts[s][5]]
            seen_cut_ties += any(cuts[s][3] < cuts[s][2] for s in live)
            seen_keep_all += any(cuts[s][5] for s in range(8))
            seen_two_bins += len({int(cuts[s][0]) >> 8 for s in live}) > 1
    assert seen_cut_ties > 50 and seen_keep_all > 50 and seen_empty == 1025 and seen_two_bins > 20, (seen_cut_ties, seen_keep_all, seen_empty, seen_two_bins)


@pytest.mark.parametrize("by_score,desc", SORTS)
def test_sizes_around_tiles_and_limits(by_score, desc):
    rng = np.random.default_rng(4)
    for n in (0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 4096, 6000):
        n_hay = n + n // 2 + 3
        tags = rng.integers(0, 16, n_hay).astype(np.uint16) | (rng.integers(0, 2, n_hay).astype(np.uint16) << 15)
        for name, (scores, one_pass) in score_sets(rng, n).items():
            recs = records(rng, n_hay, n, scores)
            sections = [(0, 0), (1, 0), (2, 1), (0, 0x8000), (1, 0), (16, 0)]
            sizes = sorted({int(H.member(tags[recs["index"]], r, e).sum()) for r, e in sections})
            limits = {0, 1, 5, 100, 1024} | {k for z in sizes for k in (z - 1, z, z + 1) if 0 <= k <= 1024}
            for limit in sorted(limits):
                check(recs, tags, sections, limit, by_score, desc, one_pass and by_score, (n, name, limit))


def test_no_tags_and_no_sections():
    rng = np.random.default_rng(5)
    recs = records(rng, 3000, 2500, rng.integers(0, 500, 2500))
    for by_score, desc in SORTS:
        heads, found, _ = check(recs, None, [(0, 0), (1, 0), (0, 1)], 50, by_score, desc, False, "no tags")
        assert found == [2500, 0, 2500] and len(heads[1]) == 0
        assert H.walk(recs, None, [], 50, by_score, desc, False)[:2] == ([], [])


def test_everything_equals_the_plain_head():
    """(0, 0) is "everything": the head is the head of the whole list, record for record"""
    rng = np.random.default_rng(6)
    tags = rng.integers(0, 65536, 8000).astype(np.uint16)
    recs = records(rng, 8000, 7000, rng.choice([96, 97, 400], 7000))
    for by_score, desc in SORTS:
        for limit in (1, 20, 1024):
            heads, found, _ = H.walk(recs, tags, [(0, 0)], limit, by_score, desc, False)
            whole = recs[::-1] if desc else recs
            if by_score:
                whole = whole[np.argsort(-whole["score"].astype(np.int64), kind="stable")]
            assert heads[0].tolist() == whole[:limit].tolist() and found == [7000]


def test_the_walk_as_a_stand_alone_program_under_address_and_ub_sanitizers():
    """the same source with its own main, built with -fsanitize=address,undefined and run as a process of its own"""
    r = subprocess.run([H.build_sanitized()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith(" 0 mismatches") and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])
