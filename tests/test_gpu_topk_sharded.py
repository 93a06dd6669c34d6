"""Top-`limit` queries over a sharded list (fzb_match_list_top_sharded / fzb_multi_match_list_top_sharded): every shard selects its own head
on its device, only those records reach the root, the root selects and orders once more.  Equal to the ORACLE's full list cut at `limit`
(the reference's caller truncates what `match_list_parallel` returns, src/matcher/parallel.rs:18-89), `found` equal to its length - for
every arrangement of the shards one GPU can host (oversubscribed; the gather forms of test_gpu_sharded.py)."""
import os
import sys

import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu

SORTS = ("ScoreThenIndexAsc", "ScoreThenIndexDesc", "IndexAsc", "IndexDesc")


@pytest.fixture(params=["pull", "pull_workers", "copy"])
def gather_mode(request):
    """shards read in place by the root (enqueued by the calling thread, or by the per-shard workers), or - FZB_SHARD_GATHER=copy - the form
    shards on OTHER devices take: the selected slot and its count pair copied to the root"""
    if request.param == "copy":
        os.environ["FZB_SHARD_GATHER"] = "copy"
    if request.param == "pull_workers":
        os.environ["FZB_SHARD_INLINE"] = "0"
    F.lib().fzb_debug_reload_knobs()
    yield request.param
    os.environ.pop("FZB_SHARD_GATHER", None)
    os.environ.pop("FZB_SHARD_INLINE", None)
    F.lib().fzb_debug_reload_knobs()


def assert_top(got, want, limit, ctx=""):
    recs, found = got
    assert found == len(want), (ctx, limit, found, len(want))
    assert recs.tolist() == want[:limit].tolist(), (ctx, limit, len(recs))


def test_single_matcher_every_sort_shard_count_and_limit(gather_mode):
    data, ends = synth.ragged_corpus(b"deadbeef", 60_013, 4, 96, seed=7)
    odata = np.concatenate([data, np.zeros(64, np.uint8)])
    have = F.device_count()
    for ndev in (1, 2, 3, 8):
        for by_bytes in (False, True):
            sc = F.ShardedCorpus(packed=(data, ends), ndev=ndev, by_bytes=by_bytes, oversubscribe=ndev > have)
            for sort in SORTS:
                for needle, typos in (("dead", 0), ("deadbeef", 1)):
                    m = F.Matcher(needle, F.Config(max_typos=typos, sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=64))
                    want = O.Matcher(needle, lanes=(64, 64, 32), max_typos=typos, sort=sort).match_packed(odata, ends)
                    per_shard = len(want) // ndev
                    assert per_shard > 100
                    # (the last limit is larger than what a shard finds on its own - its whole run travels - and smaller than the list)
                    for limit in (0, 1, 100, 5000, per_shard + per_shard // 2, len(want) + 1):
                        assert_top(m.match_list_top_sharded(sc, limit), want, limit, (ndev, by_bytes, sort, needle, typos))
                    rep = m.shard_report()
                    assert rep.startswith("root device") and rep.count("shard ") == ndev, rep
                    assert m.match_list_parallel_sharded(sc).tolist() == want.tolist()  # the full-list form on the same matcher, afterwards
                    assert_top(m.match_list_top_sharded(sc, 100), want, 100, "again")
            del sc


def test_multi_matcher_every_sort_shard_count_and_limit(gather_mode):
    data, ends = synth.ragged_corpus(b"deadbeef", 60_013, 4, 96, seed=8)
    odata = np.concatenate([data, np.zeros(64, np.uint8)])
    have = F.device_count()
    for ndev in (1, 2, 3, 8):
        for by_bytes in (False, True):
            sc = F.ShardedCorpus(packed=(data, ends), ndev=ndev, by_bytes=by_bytes, oversubscribe=ndev > have)
            for sort in SORTS:
                for q in ("dead be !x", "deadbeef dead beef"):
                    mm = F.MultiMatcher(F.parse_query(q), F.Config(sort=F.SortStrategy[sort], pf_lanes=64))
                    want = O.MultiMatcher(O.parse_query(q), sort=sort).match_packed(odata, ends)
                    per_shard = len(want) // ndev
                    assert per_shard > 20
                    for limit in (0, 1, 100, 5000, per_shard + per_shard // 2, len(want) + 1):
                        assert_top(mm.match_list_top_sharded(sc, limit), want, limit, (ndev, by_bytes, sort, q))
                    assert mm.match_list_parallel_sharded(sc).tolist() == want.tolist()
            del sc


def test_a_shard_without_a_match_empty_patterns_and_tiny_lists(gather_mode):
    have = F.device_count()
    # every match lives in the first third: with three shards the other two find nothing
    hs = ["deadbeef_%d" % i for i in range(300)] + ["nothing-%d" % i for i in range(700)]
    sc = F.ShardedCorpus(hs, ndev=3, oversubscribe=3 > have)
    for sort in SORTS:
        want = O.Matcher("deadbeef", sort=sort).match_list(hs)
        assert len(want) == 300
        m = F.Matcher("deadbeef", F.Config(sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=64))
        mm = F.MultiMatcher(F.parse_query("dead beef"), F.Config(sort=F.SortStrategy[sort], pf_lanes=64))
        wantm = O.MultiMatcher(O.parse_query("dead beef"), sort=sort).match_list(hs)
        for limit in (0, 1, 100, 300, 301, 5000):
            assert_top(m.match_list_top_sharded(sc, limit), want, limit, sort)
            assert_top(mm.match_list_top_sharded(sc, limit), wantm, limit, sort)
        for limit in (0, 10, 2000):  # no pattern: every haystack, score 0
            e = O.Matcher("", sort=sort).match_list(hs)
            assert_top(F.Matcher("", F.Config(sort=F.SortStrategy[sort])).match_list_top_sharded(sc, limit), e, limit, ("empty", sort))
            assert_top(F.MultiMatcher([], F.Config(sort=F.SortStrategy[sort])).match_list_top_sharded(sc, limit), e, limit, ("no pattern", sort))
        recs, found = F.Matcher("@@##", F.Config(sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=64)).match_list_top_sharded(sc, 10)
        assert found == 0 and len(recs) == 0
    for hs in ([], ["deadbe"], ["x", "deadbe", "", "dead_be"]):
        for ndev in (1, 3):
            sc = F.ShardedCorpus(hs, ndev=ndev, oversubscribe=ndev > have)
            for sort in SORTS:
                want = O.Matcher("deadbe", sort=sort).match_list(hs)
                for limit in (0, 1, 5):
                    assert_top(F.Matcher("deadbe", F.Config(sort=F.SortStrategy[sort], pf_lanes=64)).match_list_top_sharded(sc, limit), want, limit, (hs, ndev, sort))


def test_sharded_top_across_a_needle_change(gather_mode):
    """set_pattern between sharded top queries: the root keeps its staging, count words, peer decisions and report, the per-shard clones
    follow the needle - every answer is the unsharded matcher's."""
    have = F.device_count()
    hs = ["deadbeef_%d" % i for i in range(300)] + ["nothing-%d" % i for i in range(700)]
    sc = F.ShardedCorpus(hs, ndev=3, oversubscribe=3 > have)
    cp = F.Corpus(hs)
    cfg = F.Config(pf_lanes=64, sw_lanes=64)
    m = F.Matcher("deadbeef", cfg)
    for needle in ("deadbeef", "nothing", "deadbeef"):
        m.set_pattern(needle)
        want, want_found = F.Matcher(needle, cfg).match_list_top(cp, 50)
        got, found = m.match_list_top_sharded(sc, 50)
        assert found == want_found and found in (300, 700), needle
        assert got.tolist() == want.tolist(), needle
    assert m.shard_report().startswith("root device") and m.shard_report().count("shard ") == 3
