"""The signature filter listing its own survivors (k1_dfa_sig<.., SEG> -> k2b_dp_short<.., SEG> over the segmented list of
frizbee_amd/csrc/seg_list.h: two launches, no k_compact1) on the GPU.  Every comparison is three-way, record for record: against the
oracle, against FZB_NO_SIGNATURE=1 (k1_dfa -> k_compact1 -> scorer) and against FZB_NO_SEG_LIST=1 (k1_dfa_sig -> k_compact1 -> scorer).
fzb_debug_set_filter_grid caps the filter's grid so that small lists get runs of several tiles per workgroup, a short last run and empty
trailing segments."""
import os
import random

import numpy as np
import pytest
import torch

import frizbee_amd as F
import oracle_lib as O
from test_gpu_signature_filter import LANES, Dev, fcfg, make_rows, oracle, tile_of

pytestmark = pytest.mark.gpu

ROUND = 8  # tiles: list sizes around it give a workgroup (grid capped to 1) one full run of that many tiles, and one tile more


class knob:
    """an environment switch of knobs.h set for the block"""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        os.environ[self.name] = "1"
        F.lib().fzb_debug_reload_knobs()

    def __exit__(self, *a):
        os.environ.pop(self.name, None)
        F.lib().fzb_debug_reload_knobs()


class filter_grid:
    """fzb_debug_set_filter_grid for the block"""

    def __init__(self, g):
        self.g = g

    def __enter__(self):
        F.lib().fzb_debug_set_filter_grid(self.g)

    def __exit__(self, *a):
        F.lib().fzb_debug_set_filter_grid(0)


@pytest.fixture(scope="module")
def dev():
    return Dev(cap=24 * 1024)


def check(dev, m, needle, cp, hs, first=0, count=None, index_offset=0, **cfg):
    """the three-way comparison of one query; returns the number of records"""
    got = dev.run(m, cp, first, count, index_offset)
    assert m.last_counters()["filter_survivors"] == len(got)
    want = oracle(needle, hs, first, count, index_offset, **cfg)
    assert got.tolist() == want.tolist(), (needle, len(hs), first, count, index_offset)
    for name in ("FZB_NO_SIGNATURE", "FZB_NO_SEG_LIST"):
        with knob(name):
            old = dev.run(m, cp, first, count, index_offset)
            assert m.last_counters()["filter_survivors"] == len(got)
        assert old.tolist() == got.tolist(), (name, needle, len(hs), first, count)
    return len(got)


@pytest.mark.parametrize("length", [32, 16, None], ids=["len32", "len16", "ragged0-32"])
def test_list_sizes_runs_and_lengths(dev, length):
    rng = random.Random(300 + (length or 0))
    m = F.Matcher("DeadBe", fcfg())
    total = 0
    for n in (1, 1023, 1024, 1025):
        hs = make_rows(rng, n, length, "DeadBe", p_match=0.2)
        total += check(dev, m, "DeadBe", F.Corpus(hs), hs)
    # one workgroup: a run of ROUND tiles less one row, exactly, and a row more (ROUND + 1 tiles); three workgroups: runs of 3 tiles;
    # 20 tiles over three workgroups: runs of 7, 7 and 6 tiles, the last tile short
    for n, grids in ((ROUND * 1024 - 1, (1, 3)), (ROUND * 1024, (1, 3)), (ROUND * 1024 + 1, (1, 3)), (19 * 1024 + 77, (3,))):
        hs = make_rows(rng, n, length, "DeadBe", p_match=0.2)
        cp = F.Corpus(hs)
        for g in grids:
            with filter_grid(g):
                total += check(dev, m, "DeadBe", cp, hs)
    assert total > 5000


def test_tile_mix_inside_one_run(dev):
    rng = random.Random(31)
    T = int(F.lib().fzb_debug_signature_threshold())
    # dense | empty | threshold - 1, threshold, threshold + 1 passing rows | every row passes the signature and fails the automaton | a short last tile
    hs = tile_of(rng, 1024, 700) + tile_of(rng, 0, 0) + tile_of(rng, T - 1, T // 2) + tile_of(rng, T, T // 2) + tile_of(rng, T + 1, T // 2) + tile_of(rng, 1024, 0)
    hs += tile_of(rng, 300, 100)[:77]
    cp = F.Corpus(hs)
    m = F.Matcher("deadbe", fcfg())
    want = 700 + 3 * (T // 2) + len(oracle("deadbe", hs[6 * 1024:]))
    for g in (1, 2, 0):
        with filter_grid(g):
            assert check(dev, m, "deadbe", cp, hs) == want


def test_all_match_no_match_and_where_the_survivors_sit(dev):
    rng = random.Random(37)
    m = F.Matcher("deadbe", fcfg())
    n = 5 * 1024 + 300
    every = make_rows(rng, n, 32, "deadbe", 1.0, 0.0)
    none = make_rows(rng, n, 32, "deadbe", 0.0, 0.5)
    last = make_rows(rng, 5 * 1024, 32, "deadbe", 0.0, 0.2) + make_rows(rng, 300, 32, "deadbe", 0.5, 0.2)
    front = make_rows(rng, 1024, 32, "deadbe", 0.5, 0.2) + make_rows(rng, n - 1024, 32, "deadbe", 0.0, 0.2)
    for hs, k in ((every, n), (none, 0), (last, None), (front, None)):
        cp = F.Corpus(hs)
        for g in (0, 2):
            with filter_grid(g):
                got = check(dev, m, "deadbe", cp, hs)
                assert k is None or got == k
    idx = dev.run(m, F.Corpus(last))["index"]
    assert len(idx) > 50 and idx.min() >= 5 * 1024
    idx = dev.run(m, F.Corpus(front))["index"]
    assert len(idx) > 200 and idx.max() < 1024
    # nothing found: both count words are written
    cp = F.Corpus(none)
    dev.cnt.fill_(77)
    torch.cuda.synchronize()
    m.match_list_device(cp, dev.out.data_ptr(), dev.cap, dev.cnt.data_ptr())
    torch.cuda.synchronize()
    assert dev.cnt[:2].tolist() == [0, 0] and m.last_counters()["filter_survivors"] == 0


def test_sub_ranges_offsets_and_capacity(dev):
    rng = random.Random(41)
    hs = make_rows(rng, 4097, 32, "deadbe", p_match=0.15)
    cp = F.Corpus(hs)
    m = F.Matcher("deadbe", fcfg())
    total = 0
    for first in (0, 1, 3, 1029):
        for count in (1500, 2900):  # both end inside a tile of the range
            for g in (0, 2):
                with filter_grid(g):
                    total += check(dev, m, "deadbe", cp, hs, first, count)
    assert total > 2000
    with filter_grid(2):
        assert check(dev, m, "deadbe", cp, hs, 3, 2500, index_offset=123456) > 100
    # capacity below the match count: the first `capacity` records, dev_count = (capacity, found)
    want = oracle("deadbe", hs)
    cap = 100
    assert len(want) > 3 * cap
    out = torch.zeros((cap + 8) * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    for g in (0, 2):
        with filter_grid(g):
            out.zero_()
            m.match_list_device(cp, out.data_ptr(), cap, cnt.data_ptr())
            torch.cuda.synchronize()
            assert cnt[:2].tolist() == [cap, len(want)]
            rec = out.cpu().numpy().view(F.MATCH_DTYPE)
            assert rec[:cap].tolist() == want[:cap].tolist() and not rec[cap:].view(np.uint8).any()


def test_borrowed_appended_and_sharded_corpora(dev):
    from test_gpu_edges import padded16
    rng = random.Random(43)
    m = F.Matcher("deadbe", fcfg())
    hs = [h.encode() for h in make_rows(rng, 3 * 1024 + 500, 32, "deadbe", p_match=0.15)]
    cp = padded16(hs, torch.device("cuda", 0), False)
    F._check(F.lib().fzb_corpus_set_uniform_len(cp.h, 32))   # the uniform-length promise: end offsets are not read
    assert cp.signature_info()[0]
    for g in (0, 2):
        with filter_grid(g):
            assert check(dev, m, "deadbe", cp, hs) > 300
    # appends inside reserved room: a reserved matcher allocates nothing, segment counts included
    rg = [h.encode() for h in make_rows(rng, 3000, None, "deadbe", p_match=0.2)]
    cq = F.Corpus([])
    cq.reserve(len(rg), 48 * len(rg))
    m.reserve(cq)
    before = F.device_allocs()
    with filter_grid(2):
        for b in range(3):
            cq.append(rg[b * 1000:(b + 1) * 1000])
            got = dev.run(m, cq)
            assert got.tolist() == oracle("deadbe", rg[:(b + 1) * 1000]).tolist() and len(got) > 100 * (b + 1)
    assert F.device_allocs() == before
    # three shards on one device
    sh = make_rows(rng, 5000, 32, "deadbe", p_match=0.15)
    sc = F.ShardedCorpus(sh, ndev=3, oversubscribe=True)
    ms = F.Matcher("deadbe", F.Config(pf_lanes=64, sw_lanes=64))
    want = O.Matcher("deadbe", lanes=LANES).match_list(sh)
    got = ms.match_list_parallel_sharded(sc)
    assert len(want) > 300 and got.tolist() == want.tolist()
    for name in ("FZB_NO_SIGNATURE", "FZB_NO_SEG_LIST"):
        with knob(name):
            assert ms.match_list_parallel_sharded(sc).tolist() == want.tolist()


def test_top_and_multi_pattern_entry_points(dev):
    rng = random.Random(47)
    hs = make_rows(rng, 6 * 1024 + 11, 32, "deadbe", p_match=0.15)
    cp = F.Corpus(hs)
    want = O.Matcher("deadbe", lanes=LANES).match_list(hs)
    m = F.Matcher("deadbe", F.Config(pf_lanes=64, sw_lanes=64))
    pats, opats = F.parse_query("deadbe !k"), O.parse_query("deadbe !k")
    mm = F.MultiMatcher(pats, F.Config(pf_lanes=64, sw_lanes=64))
    wantm = O.MultiMatcher(opats, lanes=LANES).match_list(hs)
    assert len(want) > 500 and 0 < len(wantm) < len(want)

    def both():
        head, found = m.match_list_top(cp, 10)
        return head.tolist(), int(found), mm.match_list(cp).tolist()

    for g in (0, 2):
        with filter_grid(g):
            got = both()
            assert got == (want[:10].tolist(), len(want), wantm.tolist())
            for name in ("FZB_NO_SIGNATURE", "FZB_NO_SEG_LIST"):
                with knob(name):
                    assert both() == got


def test_profiled_stages_are_still_returned(dev):
    rng = random.Random(53)
    hs = make_rows(rng, 4 * 1024, 32, "deadbe", p_match=0.1)
    cp = F.Corpus(hs)
    m = F.Matcher("deadbe", fcfg())
    m.set_profiling(True)
    for _ in range(3):
        got = dev.run(m, cp)
    t = m.last_stage_timings_ms()
    m.set_profiling(False)
    assert t["calls"] == 3 and t["filter"] > 0 and t["scorers"] > 0 and t["compaction_and_window"] >= 0 and t["total"] + 1e-4 >= t["filter"] + t["scorers"]
    assert m.last_counters()["filter_survivors"] == len(got) == len(oracle("deadbe", hs))
