"""The REPEAT planes (CorpusDev::sig_planes2, frizbee_amd/csrc/sig_filter.h) and the plane form of the signature filter that reads them
(k1_dfa_sig<.., SEG, PLANES> with nsig2 != 0) on the GPU.  Every query is compared three ways, record for record: against the oracle,
against FZB_NO_SIG_PLANES=1 of the same build (the u32 form never reads the repeat planes) and through the filter's survivor count; the
corpus' repeat planes are compared with the Python reference computed from the haystack bytes, bits at and beyond the count included.
Rows are built so that a good share passes the signature and fails the repeat test (every needle letter exactly once) and some pass both
tests in the wrong order.  Shapes: list sizes around a plane word and a tile, gathered / streamed / vanishing / empty tiles inside one
batch, runs longer than a batch, aligned and unaligned sub-ranges, ragged lists, borrowed memory, corpus edits, reserved room, the switch."""
import os
import random

import pytest
import torch

import frizbee_amd as F
from sig_host_lib import py_sig, py_sig_bit
from sig_planes_host_lib import py_planes
from sig_repeat_host_lib import py_sig2, want_sig2
from test_gpu_sig_batched import filter_grid, knob
from test_gpu_sig_planes import B
from test_gpu_signature_filter import Dev, fcfg, make_rows, oracle, want_sig

pytestmark = pytest.mark.gpu

NEEDLES = ("deadbe", "aaa", "dD", "17x71", "abc")  # doubled letters | caps at two | a letter and its flip | two bytes of one class, twice | no repeat
FILL = "ghijklmnopqrstuvwxyz_-/ .0123456789GHIJK"


@pytest.fixture(scope="module")
def dev():
    return Dev(cap=24 * 1024)


def enc(hs):
    return [h.encode() if isinstance(h, str) else h for h in hs]


def once_of(needle):
    """one byte per signature bit of the needle: a row that holds these passes the signature and, for a needle with a repeat, fails the repeat test"""
    seen, out = set(), []
    for ch in needle:
        if py_sig_bit(ord(ch)) not in seen:
            seen.add(py_sig_bit(ord(ch)))
            out.append(ch)
    return "".join(out)


def plant(rng, L, filler, letters):
    s = [rng.choice(filler) for _ in range(L)]
    if L >= len(letters):
        for q, ch in zip(sorted(rng.sample(range(L), len(letters))), letters):
            s[q] = ch if rng.random() < 0.9 else ch.swapcase()
    return "".join(s)


def rows(rng, n, length, needle, p_match=0.15, p_wrong=0.1, p_once=0.3):
    """n haystacks of `length` bytes (None: 1..32): filler without the needle's letters, and three planted kinds - the needle in order, the
    needle rotated by one (every letter as often as in the needle, wrong order) and every letter once"""
    filler = [c for c in FILL if c.lower() not in needle.lower()]
    out = []
    for _ in range(n):
        L = rng.randint(1, 32) if length is None else length
        r = rng.random()
        letters = needle if r < p_match else needle[1:] + needle[:1] if r < p_match + p_wrong else once_of(needle) if r < p_match + p_wrong + p_once else ""
        out.append(plant(rng, L, filler, letters))
    return out


def passing(hs, needle):
    """(rows that pass the signature, rows that pass the signature and the repeat test)"""
    ns, ns2 = py_sig(needle.encode()), py_sig2(needle.encode())
    one = [h for h in enc(hs) if py_sig(h) & ns == ns]
    return len(one), sum(py_sig2(h) & ns2 == ns2 for h in one)


def arrays_ok(cp, hs):
    """the corpus has the three arrays, and both plane arrays are what Python makes of the haystack bytes (zero at and beyond the count)"""
    hs, n = enc(hs), len(hs)
    size = 4096 * ((n + 1023) // 1024)
    assert cp.signature_info() == (True, 4 * n)
    assert cp.signature_planes_info() == (True, size) and cp.signature_repeat_planes_info() == (True, size)
    assert cp.debug_read("sig_planes").tolist() == py_planes(want_sig(hs)).tolist()
    assert cp.debug_read("sig_planes2").tolist() == py_planes(want_sig2(hs)).tolist()


def check(dev, m, needle, cp, hs, first=0, count=None, index_offset=0):
    got = dev.run(m, cp, first, count, index_offset)
    assert m.last_counters()["filter_survivors"] == len(got)
    want = oracle(needle, hs, first, count, index_offset)
    assert got.tolist() == want.tolist(), (needle, len(hs), first, count)
    with knob("FZB_NO_SIG_PLANES"):
        old = dev.run(m, cp, first, count, index_offset)
        assert m.last_counters()["filter_survivors"] == len(got)
    assert old.tolist() == got.tolist(), (needle, len(hs), first, count)
    return len(got)


class one_cu:
    """FZB_DEBUG_CUS=1 for the block: a device of one compute unit, and the launches are recorded (F.launch_grids)"""

    def __enter__(self):
        os.environ["FZB_DEBUG_CUS"] = "1"
        F.lib().fzb_debug_reload_knobs()

    def __exit__(self, *a):
        os.environ.pop("FZB_DEBUG_CUS", None)
        F.lib().fzb_debug_reload_knobs()


def forms(dev, needle, hs, first=0, count=None):
    """the grids one query records on a device of one compute unit, its records checked against the oracle"""
    with one_cu():
        cs, ms = F.Corpus(hs), F.Matcher(needle, fcfg())
        arrays_ok(cs, hs)  # (built by eight workgroups: more than one trip of the build's loop from nine tiles on)
        F.launch_grids()
        got = dev.run(ms, cs, first, count)
        grids = F.launch_grids()
        assert got.tolist() == oracle(needle, hs, first, count).tolist()
    return grids


@pytest.mark.parametrize("needle", NEEDLES)
def test_list_sizes_and_needles(dev, needle):
    rng = random.Random(len(needle) + ord(needle[0]))
    m = F.Matcher(needle, fcfg())
    total = n_one = n_both = 0
    for n in (1, 64, 65, 1023, 1024, 1025, 2 * 1024 + 1, 5 * 1024 + 7):
        hs = rows(rng, n, 32, needle)
        cp = F.Corpus(hs)
        arrays_ok(cp, hs)
        total += check(dev, m, needle, cp, hs)
        a, b = passing(hs, needle)
        n_one, n_both = n_one + a, n_both + b
    assert total > 1000
    grids = forms(dev, needle, hs)
    assert grids["k1_dfa_sig_planes"][:2] == grids["k1_dfa_sig"][:2] == (6, 6), grids
    if needle == "abc":  # no repeat: the plane form as it was, and the two tests are one
        assert "k1_dfa_sig_repeat" not in grids and n_one == n_both
    else:
        assert grids["k1_dfa_sig_repeat"] == grids["k1_dfa_sig_planes"], grids
        assert n_one - n_both > 2500 and n_both >= total, (n_one, n_both, total)  # the once rows fail the repeat test
        assert n_both > total + 500 or needle == "aaa"  # ... and some rows pass both tests and are rejected (rotating `aaa` changes nothing)


def tile_of(rng, accepted, wrong, once, needle="deadbe"):
    """one 1024-haystack tile of 32-byte rows: `accepted` hold the needle, `wrong` its letters as often in the wrong order, `once` every letter once"""
    t = rows(rng, accepted, 32, needle, 1.0, 0.0, 0.0) + rows(rng, wrong, 32, needle, 0.0, 1.0, 0.0) + rows(rng, once, 32, needle, 0.0, 0.0, 1.0)
    t += rows(rng, 1024 - len(t), 32, needle, 0.0, 0.0, 0.0)
    rng.shuffle(t)
    return t


def test_gathered_streamed_vanishing_and_empty_tiles_inside_one_batch(dev):
    rng = random.Random(31)
    T = int(F.lib().fzb_debug_signature_threshold())
    assert 200 <= T <= 700
    m = F.Matcher("deadbe", fcfg())
    # beyond the threshold under the signature, within it under both tests: gathers | beyond it under both: streams | every candidate vanishes |
    # empty | exactly the threshold under both tests, one row more under the signature | threshold + 1 under both | sparse, then a short tile
    hs = tile_of(rng, T // 2, T // 2 - 50, 150) + tile_of(rng, T // 2, T // 2 + 50, 100) + tile_of(rng, 0, 0, 500) + tile_of(rng, 0, 0, 0)
    hs += tile_of(rng, T // 2, T - T // 2, 1) + tile_of(rng, T // 2, T + 1 - T // 2, 0) + tile_of(rng, 30, 10, 60)
    hs += tile_of(rng, 100, 100, 100)[:77]
    assert len(hs) <= B * 1024
    per_tile = [passing(hs[t * 1024:(t + 1) * 1024], "deadbe") for t in range(7)]
    assert per_tile == [(T + 100 - T % 2, T - 50 - T % 2), (T + 150 - T % 2, T + 50 - T % 2), (500, 0), (0, 0), (T + 1, T), (T + 1, T + 1), (100, 40)], per_tile
    cp = F.Corpus(hs)
    arrays_ok(cp, hs)
    want = 4 * (T // 2) + 30 + len(oracle("deadbe", hs[7 * 1024:]))
    for g in (1, 2, 0):  # one batch holds all of it | two runs | a workgroup per tile
        with filter_grid(g):
            assert check(dev, m, "deadbe", cp, hs) == want
    # every row of three tiles passes the signature and none the repeat test: nothing found
    none = tile_of(rng, 0, 0, 1024) + tile_of(rng, 0, 0, 1024) + tile_of(rng, 0, 0, 1024)[:5]
    assert passing(none, "deadbe") == (2053, 0)
    cq = F.Corpus(none)
    for g in (1, 0):
        with filter_grid(g):
            assert check(dev, m, "deadbe", cq, none) == 0


def test_runs_longer_than_one_batch(dev):
    """one and two workgroups over 2 B + 1 tiles, and a device of one compute unit: eight workgroups with runs of three tiles"""
    rng = random.Random(37)
    n = (2 * B + 1) * 1024 - 100
    hs = rows(rng, n, 32, "deadbe", 0.1, 0.05, 0.25)
    cp = F.Corpus(hs)
    arrays_ok(cp, hs)
    m = F.Matcher("deadbe", fcfg())
    for g in (1, 2):
        with filter_grid(g):
            assert check(dev, m, "deadbe", cp, hs) > 1000
    m2 = F.Matcher("aaa", fcfg())
    with filter_grid(1):
        check(dev, m2, "aaa", cp, hs)
    grids = forms(dev, "deadbe", hs)
    assert grids["k1_dfa_sig_repeat"][:2] == grids["k1_dfa_sig"][:2] == (8, 8), grids


def test_sub_ranges_aligned_and_not(dev):
    rng = random.Random(41)
    hs = rows(rng, 5 * 1024 + 7, 32, "deadbe")
    cp = F.Corpus(hs)
    m = F.Matcher("deadbe", fcfg())
    total = 0
    # first on a tile: the repeat form, the count ending inside a word (1500, 1025), on a word and on a tile; first off a tile: the u32 form
    for first in (1024, 3072, 1, 1029):
        for count in (1500, 1024, 1025, 64, len(hs) - first):
            for g in (0, 1):
                with filter_grid(g):
                    total += check(dev, m, "deadbe", cp, hs, first, count)
    assert total > 1500
    with filter_grid(1):
        assert check(dev, m, "deadbe", cp, hs, 2048, 2500, index_offset=123456) > 100
    for first, repeat in ((1024, True), (1029, False)):
        grids = forms(dev, "deadbe", hs, first, 2000)
        assert "k1_dfa_sig" in grids and ("k1_dfa_sig_repeat" in grids) == ("k1_dfa_sig_planes" in grids) == repeat, (first, grids)


def test_ragged_list_of_lengths_1_to_32(dev):
    rng = random.Random(43)
    hs = rows(rng, 3 * 1024 + 77, None, "deadbe", 0.3, 0.1, 0.3)
    # rows whose second e would lie just beyond their length - behind them a row that begins with it (5, 16 and 17 bytes: the vectors' edge too)
    for k, h in ((10, "deadb"), (700, "xdeadbyyyyyyyyyy"), (2049, "xxdeadbyyyyyyyyyy")):
        hs[k], hs[k + 1] = h, "e" + hs[k + 1][1:]
        assert passing([h], "deadbe") == (1, 0)
    assert {len(h) for h in hs} == set(range(1, 33))
    cp = F.Corpus(hs)
    arrays_ok(cp, hs)
    assert cp.info()["uniform_len"] == 0
    a, b = passing(hs, "deadbe")
    assert a - b > 500
    m = F.Matcher("deadbe", fcfg())
    for g in (0, 1):
        with filter_grid(g):
            assert check(dev, m, "deadbe", cp, hs) > 300
    assert "k1_dfa_sig_repeat" in forms(dev, "deadbe", hs)


def test_borrowed_device_memory(dev):
    from test_gpu_edges import padded16
    rng = random.Random(47)
    hs = enc(rows(rng, 2500, 32, "deadbe"))
    m = F.Matcher("deadbe", fcfg())
    want = oracle("deadbe", hs).tolist()
    for u64 in (False, True):
        cp = padded16(hs, torch.device("cuda", 0), u64)
        assert cp.signature_repeat_planes_info() == (False, 0) and len(cp.debug_read("sig_planes2")) == 0
        assert dev.run(m, cp).tolist() == want
        F._check(F.lib().fzb_corpus_set_uniform_len(cp.h, 32))  # the uniform-length promise: no end offsets read
        arrays_ok(cp, hs)
        assert check(dev, m, "deadbe", cp, hs) == len(want)
        F._check(F.lib().fzb_corpus_set_uniform_len(cp.h, 0))   # cleared: the three arrays go, the query still agrees
        assert cp.signature_info() == cp.signature_planes_info() == cp.signature_repeat_planes_info() == (False, 0)
        assert dev.run(m, cp).tolist() == want
        F._check(F.lib().fzb_corpus_set_max_len(cp.h, 32))      # the bound alone (end offsets are read)
        arrays_ok(cp, hs)
        assert check(dev, m, "deadbe", cp, hs) == len(want)
        F._check(F.lib().fzb_corpus_set_max_len(cp.h, 64))      # loosened beyond 32
        assert cp.signature_repeat_planes_info() == (False, 0) and dev.run(m, cp).tolist() == want
    rg = enc(rows(rng, 1500, None, "deadbe", 0.3, 0.1, 0.3))
    cr = padded16(rg, torch.device("cuda", 0), True)
    F._check(F.lib().fzb_corpus_set_max_len(cr.h, 32))
    arrays_ok(cr, rg)
    assert check(dev, m, "deadbe", cr, rg) > 100


def test_corpus_edits_keep_the_repeat_planes_in_step(dev):
    rng = random.Random(53)
    hs = enc(rows(rng, 3000, None, "deadbe"))
    extra = enc(rows(rng, 700, None, "deadbe", 0.3, 0.1, 0.3))
    m = F.Matcher("deadbe", fcfg())
    cp = F.Corpus(hs)

    def in_step(cur):
        assert len(cp) == len(cur)
        arrays_ok(cp, cur)
        assert check(dev, m, "deadbe", cp, cur) > 100

    in_step(hs)
    cur = hs + extra
    cp.append(extra)  # without reserve: the arrays regrow
    in_step(cur)
    idx = sorted(rng.sample(range(len(cur)), 40))
    new = enc(rows(rng, 40, None, "deadbe", 0.4, 0.1, 0.4))
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
    cp.append(extra[:600])  # behind a truncate: the cut tile is rebuilt from the bytes
    cur = cur + extra[:600]
    in_step(cur)
    # a haystack beyond 32 bytes: the three arrays go; removed again, they are rebuilt
    cp.append([b"d" * 40])
    assert cp.signature_info() == cp.signature_planes_info() == cp.signature_repeat_planes_info() == (False, 0) and len(cp.debug_read("sig_planes2")) == 0
    assert dev.run(m, cp).tolist() == oracle("deadbe", cur + [b"d" * 40]).tolist()
    cp.truncate(len(cur))
    in_step(cur)
    # reserved room: after the first append, appends inside it allocate nothing - repeat planes included
    cq = F.Corpus([])
    cq.reserve(len(hs), 48 * len(hs))
    m.reserve(cq)
    cq.append(hs[:1000])
    before = F.device_allocs()
    for b in (1, 2):
        cq.append(hs[b * 1000:(b + 1) * 1000])
        assert check(dev, m, "deadbe", cq, hs[:(b + 1) * 1000]) > 100
    assert F.device_allocs() == before
    arrays_ok(cq, hs)


def test_the_switches(dev):
    rng = random.Random(59)
    hs = rows(rng, 2500, 32, "deadbe")
    with knob("FZB_NO_SIGNATURE"):
        cn = F.Corpus(hs)
        assert cn.signature_info() == cn.signature_planes_info() == cn.signature_repeat_planes_info() == (False, 0)
        assert len(cn.debug_read("sig")) == len(cn.debug_read("sig_planes")) == len(cn.debug_read("sig_planes2")) == 0
    with knob("FZB_NO_SIG_PLANES"):  # the arrays are built and left unused
        cp = F.Corpus(hs)
        arrays_ok(cp, hs)
    m = F.Matcher("deadbe", fcfg())
    assert check(dev, m, "deadbe", cp, hs) > 100
    assert dev.run(m, cn).tolist() == oracle("deadbe", hs).tolist()
