"""frizbee_amd/csrc/topk_select.h - the decisions the top-`limit` selection kernels (kernels_topk.hip) take - compiled for the host and
fuzzed against numpy.  The property is the whole contract of the stage: the kept records, still in record order, reversed for the *Desc
strategies and sorted stably by descending score, ARE the first `limit` entries of the same reverse + stable sort of every record
(`match_list`'s post-step, src/matcher/mod.rs:215-221 + src/sort.rs:6-40 of the reference)."""
import numpy as np
import pytest

import topk_host_lib as TH

pytestmark = pytest.mark.skipif(not TH.available(), reason="ROCm clang++ not installed")


def ordered(idx, scores, by_score, desc):
    """`match_list`'s post-step over the records `idx` (ascending): reverse for *Desc, stable sort by descending score for Score*"""
    idx = np.asarray(idx, dtype=np.int64)
    if desc:
        idx = idx[::-1]
    if by_score:
        idx = idx[np.argsort(-scores[idx].astype(np.int64), kind="stable")]
    return idx


def score_arrays(rng, n):
    yield "uniform", rng.integers(0, 65536, n).astype(np.uint16)
    vals = rng.integers(0, 65536, int(rng.integers(1, 4)))
    yield "heavy ties", rng.choice(vals, n).astype(np.uint16)
    yield "below 256", rng.integers(0, 256, n).astype(np.uint16)
    yield "few low values", rng.choice(rng.integers(0, 256, int(rng.integers(1, 4))), n).astype(np.uint16)
    his = rng.integers(0, 256, 4)
    yield "several high bytes", ((rng.choice(his, n).astype(np.uint32) << 8) | rng.integers(0, 8, n).astype(np.uint32)).astype(np.uint16)
    yield "scorer-like", np.minimum(rng.poisson(60, n) + (rng.random(n) < 0.02) * 250, 65535).astype(np.uint16)


def check(scores, limit, by_score, desc, one_pass):
    n = len(scores)
    dest, cut, kept = TH.select(scores, limit, by_score, desc, one_pass)
    want = min(limit, n)
    assert kept == want
    kept_idx = np.nonzero(dest != TH.NOT_KEPT)[0]
    # the destinations are the compaction in record order: 0 .. kept-1, ascending with the record index
    assert np.array_equal(dest[kept_idx], np.arange(kept, dtype=np.uint32))
    full = ordered(np.arange(n), scores, by_score, desc)
    assert np.array_equal(ordered(kept_idx, scores, by_score, desc), full[:limit])
    # the cut itself, computed directly
    if n <= limit:
        assert cut["keep_all"] == 1
        return
    assert cut["keep_all"] == 0
    if not by_score:
        assert (cut["gt"], cut["ties"], cut["quota"], cut["lo"]) == (0, n, limit, n - limit if desc else 0)
        return
    if limit == 0:
        assert cut["T"] > 0xFFFF and cut["gt"] == 0 and cut["quota"] == 0
        return
    T = int(np.sort(scores)[::-1][limit - 1])  # the limit-th best score
    gt, ties = int((scores > T).sum()), int((scores == T).sum())
    assert gt < limit <= gt + ties
    assert (cut["T"], cut["gt"], cut["ties"], cut["quota"], cut["lo"]) == (T, gt, ties, limit - gt, ties - (limit - gt) if desc else 0)


@pytest.mark.parametrize("seed", range(6))
def test_selection_is_the_head_of_the_stable_sort(seed):
    rng = np.random.default_rng(1000 + seed)
    sizes = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, int(rng.integers(3000, 20001)), 20000]
    cases = 0
    for n in sizes:
        for name, scores in score_arrays(rng, n):
            below_256 = n == 0 or int(scores.max()) < 256
            for desc in (False, True):
                for by_score in (True, False):
                    limits = {0, 1, 2, max(n - 1, 0), n, n + 1, int(rng.integers(0, n + 2)), int(rng.integers(0, n + 2))}
                    for limit in sorted(limits):
                        check(scores, limit, by_score, desc, False)
                        if below_256 and by_score:
                            check(scores, limit, by_score, desc, True)
                        cases += 1
    assert cases > 1000


def test_known_small_cases():
    s = np.array([5, 9, 5, 9, 5, 1], np.uint16)
    # limit 3, ascending ties: both 9s and the FIRST 5; descending: both 9s and the LAST 5
    dest, cut, kept = TH.select(s, 3, True, False)
    assert list(np.nonzero(dest != TH.NOT_KEPT)[0]) == [0, 1, 3] and (cut["T"], cut["gt"], cut["quota"], cut["lo"]) == (5, 2, 1, 0)
    dest, cut, kept = TH.select(s, 3, True, True)
    assert list(np.nonzero(dest != TH.NOT_KEPT)[0]) == [1, 3, 4] and (cut["T"], cut["gt"], cut["quota"], cut["lo"]) == (5, 2, 1, 2)
    # by index: the first / last two records
    assert list(np.nonzero(TH.select(s, 2, False, False)[0] != TH.NOT_KEPT)[0]) == [0, 1]
    assert list(np.nonzero(TH.select(s, 2, False, True)[0] != TH.NOT_KEPT)[0]) == [4, 5]
    # a cut above 255 and one below it on the same array
    s = np.array([300, 10, 300, 299, 10, 700, 10], np.uint16)
    assert list(np.nonzero(TH.select(s, 2, True, False)[0] != TH.NOT_KEPT)[0]) == [0, 5]
    assert list(np.nonzero(TH.select(s, 2, True, True)[0] != TH.NOT_KEPT)[0]) == [2, 5]
    assert list(np.nonzero(TH.select(s, 5, True, True)[0] != TH.NOT_KEPT)[0]) == [0, 2, 3, 5, 6]
