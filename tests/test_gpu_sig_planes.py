"""The PLANE form of the signature filter (k1_dfa_sig<.., SEG, PLANES> over CorpusDev::sig_planes, frizbee_amd/csrc/sig_filter.h) on the
GPU.  Every query is compared three ways, record for record: against the oracle, against FZB_NO_SIG_PLANES=1 of the same build (the u32
form, tile by tile) and through the filter's survivor count; the corpus' planes are compared with the plain transposition of its u32
signatures.  Shapes: list sizes around a plane word and a tile, runs longer than one batch (fzb_debug_set_filter_grid, FZB_DEBUG_CUS=1),
dense / empty / all-pass-none-match tiles inside one batch, aligned and unaligned sub-ranges, corpus edits and reserved room.
(The bitmap words and tile counts the kernel also writes are not exposed by the Python mirror: their consumers - FZB_NO_SEG_LIST's
k_compact1 among them - are behind the u32 form only, and the survivor count and the records are what this file can see of them.)"""
import os
import random
import re

import numpy as np
import pytest
import torch

import frizbee_amd as F
from sig_host_lib import py_sig
from sig_planes_host_lib import py_planes
from test_gpu_sig_batched import filter_grid, knob
from test_gpu_signature_filter import Dev, fcfg, make_rows, oracle, tile_of, want_sig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = int(re.search(r"#define FZB_SIG_BATCH_TILES (\d+)u", open(os.path.join(ROOT, "frizbee_amd", "csrc", "sig_filter.h")).read()).group(1))
NEEDLES = ("deadbe", "a_b-1", "abcdeqz0")  # 4 letters | letters and three of the other-byte classes | 8 distinct bits


@pytest.fixture(scope="module")
def dev():
    return Dev(cap=24 * 1024)


def planes_ok(cp, n):
    """the corpus has both arrays, and the planes are the transposition of the signatures"""
    assert cp.signature_info() == (True, 4 * n)
    assert cp.signature_planes_info() == (True, 4096 * ((n + 1023) // 1024))
    sig = cp.debug_read("sig")
    assert cp.debug_read("sig_planes").tolist() == py_planes(sig).tolist()
    return sig


def check(dev, m, needle, cp, hs, first=0, count=None, index_offset=0):
    got = dev.run(m, cp, first, count, index_offset)
    assert m.last_counters()["filter_survivors"] == len(got)
    want = oracle(needle, hs, first, count, index_offset)
    assert got.tolist() == want.tolist(), (needle, len(hs), first, count)
    assert (np.diff(got["index"].astype(np.int64)) > 0).all()
    with knob("FZB_NO_SIG_PLANES"):
        old = dev.run(m, cp, first, count, index_offset)
        assert m.last_counters()["filter_survivors"] == len(got)
    assert old.tolist() == got.tolist(), (needle, len(hs), first, count)
    return len(got)


@pytest.mark.parametrize("needle", NEEDLES)
def test_list_sizes(dev, needle):
    rng = random.Random(len(needle))
    m = F.Matcher(needle, fcfg())
    total = 0
    for n in (1, 64, 65, 1023, 1024, 1025, 2 * 1024 + 1, 5 * 1024 + 7):
        hs = make_rows(rng, n, 32, needle, p_match=0.2, p_letters=0.2)
        cp = F.Corpus(hs)
        sig = planes_ok(cp, n)
        assert sig.tolist() == want_sig([h.encode() for h in hs]).tolist()
        total += check(dev, m, needle, cp, hs)
    assert total > 1500


def test_ragged_list_of_lengths_1_to_32(dev):
    rng = random.Random(5)
    hs = []
    for i in range(3 * 1024 + 77):
        hs += make_rows(rng, 1, 1 + rng.randrange(32), "deadbe", p_match=0.3, p_letters=0.2)
    assert {len(h) for h in hs} == set(range(1, 33))
    cp = F.Corpus(hs)
    planes_ok(cp, len(hs))
    assert cp.info()["uniform_len"] == 0
    m = F.Matcher("deadbe", fcfg())
    for g in (0, 1):
        with filter_grid(g):
            assert check(dev, m, "deadbe", cp, hs) > 300


def test_runs_longer_than_one_batch(dev):
    """one and two workgroups over 2 B + 1 tiles: a second (and third) batch, and the survivors listed so far carried across them"""
    rng = random.Random(9)
    n = (2 * B + 1) * 1024 - 100
    hs = make_rows(rng, n, 32, "deadbe", p_match=0.1, p_letters=0.1)
    cp = F.Corpus(hs)
    m = F.Matcher("deadbe", fcfg())
    for g in (1, 2):
        with filter_grid(g):
            assert check(dev, m, "deadbe", cp, hs) > 1000
    m2 = F.Matcher("a_b-1", fcfg())
    with filter_grid(1):
        check(dev, m2, "a_b-1", cp, hs)
    # a device of one compute unit: eight workgroups, runs of three tiles - and the record says that the plane form ran
    try:
        os.environ["FZB_DEBUG_CUS"] = "1"
        F.lib().fzb_debug_reload_knobs()
        cs, ms = F.Corpus(hs), F.Matcher("deadbe", fcfg())
        F.launch_grids()
        got = dev.run(ms, cs)
        grids = F.launch_grids()
        assert grids["k1_dfa_sig_planes"][:2] == grids["k1_dfa_sig"][:2] == (8, 8), grids
        assert got.tolist() == oracle("deadbe", hs).tolist()
        os.environ["FZB_NO_SIG_PLANES"] = "1"
        F.lib().fzb_debug_reload_knobs()
        old = dev.run(ms, cs)
        grids = F.launch_grids()
        assert "k1_dfa_sig" in grids and "k1_dfa_sig_planes" not in grids, grids
        assert old.tolist() == got.tolist()
    finally:
        os.environ.pop("FZB_DEBUG_CUS", None)
        os.environ.pop("FZB_NO_SIG_PLANES", None)
        F.lib().fzb_debug_reload_knobs()


def test_dense_all_pass_and_empty_tiles_inside_one_batch(dev):
    rng = random.Random(13)
    T = int(F.lib().fzb_debug_signature_threshold())
    m = F.Matcher("deadbe", fcfg())
    # sparse | every row passes, 700 match | sparse | every row passes, none matches (the letters in the wrong order) | threshold, threshold + 1 | empty | short
    hs = tile_of(rng, 60, 30) + tile_of(rng, 1024, 700) + tile_of(rng, 80, 40) + tile_of(rng, 1024, 0) + tile_of(rng, T, T // 2) + tile_of(rng, T + 1, T // 2) + tile_of(rng, 0, 0)
    hs += tile_of(rng, 300, 100)[:77]
    assert len(hs) <= B * 1024
    cp = F.Corpus(hs)
    sig = planes_ok(cp, len(hs))
    ns = py_sig(b"deadbe")
    assert [int(((sig[t * 1024:(t + 1) * 1024] & ns) == ns).sum()) for t in range(7)] == [60, 1024, 80, 1024, T, T + 1, 0]
    want = 30 + 700 + 40 + 2 * (T // 2) + len(oracle("deadbe", hs[7 * 1024:]))
    for g in (1, 2, 0):  # one batch holds all of it | two runs | a workgroup per tile
        with filter_grid(g):
            assert check(dev, m, "deadbe", cp, hs) == want
    # every row of two tiles passes the signature and none matches: nothing found, both count words written
    none = tile_of(rng, 1024, 0) + tile_of(rng, 1024, 0)
    cq = F.Corpus(none)
    with filter_grid(1):
        assert check(dev, m, "deadbe", cq, none) == 0
    # a batch without a single candidate
    empty = make_rows(rng, 3 * 1024 + 5, 32, "deadbe", 0.0, 0.0)
    ce = F.Corpus(empty)
    assert int(((planes_ok(ce, len(empty)) & ns) == ns).sum()) == 0
    for g in (1, 0):
        with filter_grid(g):
            dev.cnt.fill_(77)
            torch.cuda.synchronize()
            m.match_list_device(ce, dev.out.data_ptr(), dev.cap, dev.cnt.data_ptr())
            torch.cuda.synchronize()
            assert dev.cnt[:2].tolist() == [0, 0] and m.last_counters()["filter_survivors"] == 0


def test_sub_ranges_aligned_and_not(dev):
    rng = random.Random(17)
    hs = make_rows(rng, 5 * 1024 + 7, 32, "deadbe", p_match=0.15, p_letters=0.15)
    cp = F.Corpus(hs)
    m = F.Matcher("deadbe", fcfg())
    total = 0
    # first a multiple of the tile: the plane form over the tiles from first / 1024 on, the count ending inside a word, on a word and on a tile;
    # first off a tile: the u32 form
    for first in (1024, 3072, 1, 1029):
        for count in (1500, 1024, 1025, 64, len(hs) - first):
            for g in (0, 1):
                with filter_grid(g):
                    total += check(dev, m, "deadbe", cp, hs, first, count)
    assert total > 1500
    with filter_grid(1):
        assert check(dev, m, "deadbe", cp, hs, 2048, 2500, index_offset=123456) > 100
    try:  # which form took which range
        os.environ["FZB_DEBUG_CUS"] = "1"
        F.lib().fzb_debug_reload_knobs()
        cs, ms = F.Corpus(hs), F.Matcher("deadbe", fcfg())
        for first, planes in ((1024, True), (1029, False)):
            F.launch_grids()
            got = dev.run(ms, cs, first, 2000)
            grids = F.launch_grids()
            assert "k1_dfa_sig" in grids and ("k1_dfa_sig_planes" in grids) == planes, (first, grids)
            assert got.tolist() == oracle("deadbe", hs, first, 2000).tolist()
    finally:
        os.environ.pop("FZB_DEBUG_CUS", None)
        F.lib().fzb_debug_reload_knobs()


def test_corpus_edits_keep_the_planes_in_step(dev):
    rng = random.Random(19)
    hs = [h.encode() for h in make_rows(rng, 3000, None, "deadbe", p_match=0.15)]
    extra = [h.encode() for h in make_rows(rng, 700, None, "deadbe", p_match=0.3)]
    m = F.Matcher("deadbe", fcfg())
    cp = F.Corpus(hs)

    def in_step(cur):
        assert len(cp) == len(cur)
        assert planes_ok(cp, len(cur)).tolist() == want_sig(cur).tolist()
        assert check(dev, m, "deadbe", cp, cur) > 100

    in_step(hs)
    cur = hs + extra
    cp.append(extra)  # without reserve: the arrays regrow
    in_step(cur)
    idx = sorted(rng.sample(range(len(cur)), 40))
    new = [h.encode() for h in make_rows(rng, 40, None, "deadbe", p_match=0.5)]
    cp.replace(idx, new)
    for i, h in zip(idx, new):
        cur[i] = h
    in_step(cur)
    drop = set(rng.sample(range(len(cur)), 55))
    cp.remove(sorted(drop))
    cur = [h for i, h in enumerate(cur) if i not in drop]
    in_step(cur)
    for keep in (2049, 2048, 1500):  # inside a tile | on a tile's edge | inside a word
        cp.truncate(keep)
        cur = cur[:keep]
        in_step(cur)
    cp.append(extra[:600])  # behind a truncate: the cut tile's planes are rebuilt from the kept signatures
    cur = cur + extra[:600]
    in_step(cur)
    # a haystack beyond 32 bytes: signatures and planes go; removed again, both are rebuilt
    cp.append([b"d" * 40])
    assert cp.signature_info() == (False, 0) and cp.signature_planes_info() == (False, 0) and len(cp.debug_read("sig_planes")) == 0
    cp.truncate(len(cur))
    in_step(cur)
    # reserved room: after the first append, appends inside it allocate nothing - planes included
    cq = F.Corpus([])
    cq.reserve(len(hs), 48 * len(hs))
    m.reserve(cq)
    cq.append(hs[:1000])
    before = F.device_allocs()
    for b in (1, 2):
        cq.append(hs[b * 1000:(b + 1) * 1000])
        assert check(dev, m, "deadbe", cq, hs[:(b + 1) * 1000]) > 100
    assert F.device_allocs() == before
    assert planes_ok(cq, len(hs)).tolist() == want_sig(hs).tolist()


def test_the_switch_builds_the_planes_and_leaves_them_unused(dev):
    rng = random.Random(23)
    hs = make_rows(rng, 2500, 32, "deadbe", p_match=0.15)
    with knob("FZB_NO_SIG_PLANES"):
        cp = F.Corpus(hs)
        planes_ok(cp, len(hs))
    with knob("FZB_NO_SIGNATURE"):
        cn = F.Corpus(hs)
        assert cn.signature_info() == (False, 0) and cn.signature_planes_info() == (False, 0)
    m = F.Matcher("deadbe", fcfg())
    assert check(dev, m, "deadbe", cp, hs) > 100
    assert dev.run(m, cn).tolist() == oracle("deadbe", hs).tolist()
