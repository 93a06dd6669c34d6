"""The union step of the fused multi-pattern top + matched-positions query on the CPU: frizbee_amd/csrc/indices_union.h - what k_multi_union
calls per head record - compiled for the host (tests/union_host_lib.py) and held to numpy.  Expected union of a record's lists:
np.unique(concat)[::-1] (`match_one_indices_multi`, src/matcher/multi.rs:56-82: descending, patterns may share matched chars).  Expected
record: the saturating u16 sum, the OR of the exact flags, the patterns' common index; patterns that disagree on the index or on the record
count give values indices_pack.h's checks reject."""
import numpy as np
import pytest

import union_host_lib as U

pytestmark = pytest.mark.skipif(not U.available(), reason="ROCm clang++ not installed")


def make_lists(rng, n, stride, kind, universe):
    """n strictly descending lists of 0..stride positions each (+ npos, which may exceed the stride: the scorer counts what it found)"""
    pos = np.full((n, stride), 0xDEAD, np.uint32)  # (what lies behind a list's end must never be read)
    npos = np.zeros(n, np.uint32)
    lists = []
    for k in range(n):
        if kind == "empty":
            ln = 0
        elif kind == "full":
            ln = stride
        else:
            ln = int(rng.integers(0, stride + 1))
        ln = min(ln, len(universe[k]))
        vals = np.sort(rng.choice(universe[k], ln, replace=False))[::-1]
        pos[k, :ln] = vals
        npos[k] = ln + (int(rng.integers(0, 3)) if ln == stride else 0)
        lists.append(vals)
    return pos.reshape(-1), npos, lists


def run_case(rng, P, n, strides, overlap, kinds=None, scores_hi=300):
    head = np.zeros(n, U.REC)
    head["index"] = rng.permutation(10 * n + 5)[:n]
    sources, per_k = [], [[] for _ in range(n)]
    total = int(sum(strides))
    for p in range(P):
        if overlap == "same":      # every pattern draws from the same few bytes: fully overlapping where the lists are full
            universe = [np.arange(100, 100 + max(strides)) for _ in range(n)]
        elif overlap == "disjoint":
            universe = [np.arange(1000 * p, 1000 * p + 2 * strides[p] + 1) for _ in range(n)]
        else:                      # interleaved: a window a little wider than the lists together
            universe = [np.arange(0, 2 * total + 2) for _ in range(n)]
        pos, npos, lists = make_lists(rng, n, strides[p], kinds[p] if kinds else "random", universe)
        recs = np.zeros(n, U.REC)
        recs["index"] = head["index"]
        recs["score"] = rng.integers(0, scores_hi, n)
        recs["exact"] = rng.integers(0, 2, n)
        sources.append((recs, n, npos, pos, strides[p]))
        for k in range(n):
            per_k[k].append(lists[k])
    comb, count, npos_u, pos_u = U.union(sources, head)
    assert count == n
    for k in range(n):
        want = np.unique(np.concatenate(per_k[k] + [np.zeros(0, np.uint32)]))[::-1]
        assert npos_u[k] == len(want), (P, k, npos_u[k], want)
        assert pos_u[k, : len(want)].tolist() == want.tolist(), (P, k)
        assert (pos_u[k, len(want):] == 0xFFFFFFFF).all()  # nothing is written behind the union
    ssum = np.minimum(sum((s[0]["score"].astype(np.int64) for s in sources), np.zeros(n, np.int64)), 65535)
    eor = np.zeros(n, bool)
    for s in sources:
        eor |= s[0]["exact"] != 0
    assert comb["score"].tolist() == ssum.tolist()
    assert (comb["exact"] != 0).tolist() == eor.tolist()
    assert comb["index"].tolist() == head["index"].tolist()
    return sources, head, comb


@pytest.mark.parametrize("P", range(0, 9))
@pytest.mark.parametrize("overlap", ["same", "disjoint", "interleaved"])
def test_union_matches_numpy(P, overlap):
    rng = np.random.default_rng(100 * P + len(overlap))
    for _ in range(6):
        strides = [int(x) for x in rng.integers(1, 13, P)]
        run_case(rng, P, int(rng.integers(1, 40)), strides, overlap)


def test_no_positive_pattern():
    """only negated patterns: the head's index, score 0, exact 0, no positions, the head's count"""
    head = np.zeros(5, U.REC)
    head["index"] = [9, 3, 7, 1, 0]
    head["score"] = 77  # (the combined record does not copy the head: an all-negated head has score 0 and the pack's check shows a difference)
    comb, count, npos_u, pos_u = U.union([], head)
    assert count == 5 and comb["index"].tolist() == [9, 3, 7, 1, 0] and not comb["score"].any() and not comb["exact"].any()
    assert not npos_u.any() and pos_u.shape == (5, 0)
    head["score"] = 0
    assert U.check(head, 5, comb, count) == 0


@pytest.mark.parametrize("kinds", [("empty", "full"), ("full", "empty", "random"), ("empty", "empty"), ("full", "full", "full")])
def test_one_list_empty_and_full_lists(kinds):
    rng = np.random.default_rng(len(kinds))
    for overlap in ("same", "disjoint", "interleaved"):
        run_case(rng, len(kinds), 17, [int(x) for x in rng.integers(1, 9, len(kinds))], overlap, kinds=kinds)


def test_stride_one_and_a_long_needles_stride():
    rng = np.random.default_rng(5)
    for overlap in ("same", "disjoint", "interleaved"):
        run_case(rng, 4, 33, [1, 1, 1, 1], overlap)
        run_case(rng, 3, 9, [200, 1, 200], overlap)
        run_case(rng, 2, 5, [200, 200], overlap, kinds=("full", "full"))


def test_scores_saturate_on_both_sides_of_65535():
    rng = np.random.default_rng(6)
    n = 6
    head = np.zeros(n, U.REC)
    head["index"] = np.arange(n)
    cols = np.array([[65534, 0, 0], [65534, 1, 0], [65534, 1, 1], [20000, 20000, 20000], [40000, 40000, 40000], [65535, 65535, 65535]], np.int64)
    want = [65534, 65535, 65535, 60000, 65535, 65535]
    sources = []
    for p in range(3):
        recs = np.zeros(n, U.REC)
        recs["index"] = head["index"]
        recs["score"] = cols[:, p]
        sources.append((recs, n, np.zeros(n, np.uint32), np.zeros(n, np.uint32), 1))
    comb, count, _, _ = U.union(sources, head)
    assert comb["score"].tolist() == want and count == n
    # and through the random path with large scores
    run_case(rng, 4, 50, [3, 3, 3, 3], "interleaved", scores_hi=30000)


def test_disagreement_gives_what_the_pack_check_rejects():
    rng = np.random.default_rng(7)
    sources, head, comb = run_case(rng, 3, 12, [4, 5, 6], "interleaved")
    head = head.copy()
    head["score"], head["exact"] = comb["score"], comb["exact"]
    assert U.check(head, 12, comb, 12) == 0
    # one pattern carries another index for record 5 - whichever pattern it is, and also when it is the head's index the others miss
    for p in range(3):
        recs = [s[0].copy() for s in sources]
        recs[p]["index"][5] ^= 1
        bad_sources = [(recs[q],) + sources[q][1:] for q in range(3)]
        c2, count, _, _ = U.union(bad_sources, head)
        assert count == 12 and c2["index"][5] != head["index"][5]
        assert U.check(head, 12, c2, count) == U.BAD_RECORD
        assert np.delete(c2["index"], 5).tolist() == np.delete(head["index"], 5).tolist()
    recs = [s[0].copy() for s in sources]
    for r in recs:
        r["index"][5] ^= 1  # all patterns agree with each other but not with the head: the pack's own comparison sees it
    c2, count, _, _ = U.union([(recs[q],) + sources[q][1:] for q in range(3)], head)
    assert U.check(head, 12, c2, count) == U.BAD_RECORD
    # one pattern's traced pass produced another number of records than the head has
    for p in range(3):
        for other in (11, 13, 0):
            bad_sources = [sources[q][:1] + ((other if q == p else 12),) + sources[q][2:] for q in range(3)]
            c2, count, _, _ = U.union(bad_sources, head)
            assert count == other
            assert U.check(head, 12, c2, count) == U.BAD_COUNT


def test_head_longer_than_its_room_and_by_value_bound():
    """the walk covers min(head count, room) records (the kernel trims its grid by the device-side count); the by-value bound is the one the
    fuzz straddles"""
    assert U.lib().uh_by_value() == 8
    rng = np.random.default_rng(8)
    sources, head, comb = run_case(rng, 2, 20, [3, 4], "interleaved")
    c2, count, npos_u, pos_u = U.union(sources, head, head_count=20, max_records=7)
    assert len(c2) == 7 and c2.tolist() == comb[:7].tolist()
    assert count == 20  # the sources' counts equal the head's: what the pack compares
