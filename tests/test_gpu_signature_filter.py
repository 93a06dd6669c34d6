"""The signature form of the streaming filter (k1_dfa_sig behind CorpusDev::sig, frizbee_amd/csrc/sig_filter.h) on the GPU: records of
match_list_device record for record against the oracle, against the same query under FZB_NO_SIGNATURE=1 (k1_dfa), and the corpus'
signature array against numpy - at the smallest shapes where each piece can go wrong: list sizes around a bitmap word and a tile, both
tile branches and the threshold between them, sub-ranges that start off a 16-byte signature vector, corpus edits, shards, borrowed memory."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import frizbee_amd as F
import oracle_lib as O
from sig_host_lib import py_sig

pytestmark = pytest.mark.gpu

LANES = (64, 64, 32)
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4097)


def want_sig(hs):
    return np.array([py_sig(h) for h in hs], np.uint32)


def fcfg(**kw):
    return F.Config(sort=F.SortStrategy.IndexAsc, pf_lanes=64, sw_lanes=64, **kw)


class Dev:
    """match_list_device into one reused buffer: records in index order, straight from HBM"""

    def __init__(self, cap=8192):
        self.cap = cap
        self.out = torch.zeros(cap * 8 + 64, dtype=torch.uint8, device="cuda")
        self.cnt = torch.zeros(4, dtype=torch.int32, device="cuda")

    def run(self, m, cp, first=0, count=None, index_offset=0):
        self.cnt.zero_()
        torch.cuda.synchronize()
        m.match_list_device(cp, self.out.data_ptr(), self.cap, self.cnt.data_ptr(), first=first, count=count, index_offset=index_offset)
        torch.cuda.synchronize()
        k = int(self.cnt[0].item())
        return self.out[: k * 8].cpu().numpy().view(F.MATCH_DTYPE).copy()


@pytest.fixture(scope="module")
def dev():
    return Dev()


class no_signature:
    """FZB_NO_SIGNATURE=1 for the block: the filter takes k1_dfa over the same corpus"""

    def __enter__(self):
        os.environ["FZB_NO_SIGNATURE"] = "1"
        F.lib().fzb_debug_reload_knobs()

    def __exit__(self, *a):
        os.environ.pop("FZB_NO_SIGNATURE", None)
        F.lib().fzb_debug_reload_knobs()


def oracle(needle, hs, first=0, count=None, index_offset=0, **cfg):
    count = len(hs) - first if count is None else count
    w = O.Matcher(needle, lanes=LANES, sort="IndexAsc", **cfg).match_list(hs[first:first + count])
    w["index"] += index_offset
    return w


def check(dev, m, needle, cp, hs, first=0, count=None, index_offset=0, **cfg):
    """the three-way comparison of one query; returns the number of records"""
    got = dev.run(m, cp, first, count, index_offset)
    want = oracle(needle, hs, first, count, index_offset, **cfg)
    assert got.tolist() == want.tolist(), (needle, len(hs), first, count, index_offset)
    with no_signature():
        old = dev.run(m, cp, first, count, index_offset)
    assert old.tolist() == got.tolist(), (needle, len(hs), first, count)
    return len(got)


def make_rows(rng, n, length, needle, p_match=0.1, p_letters=0.15):
    """n haystacks of `length` bytes (None: 0..32, empty ones included): filler that excludes the needle's letters, a share with the needle
    planted in order (accepted) and a share with its letters in the wrong order (pass the signature, fail the automaton)"""
    filler = [c for c in "ghijklmnopqrstuvwxyz_-/ .0123456789GHIJK" if c.lower() not in needle.lower()]
    out = []
    for _ in range(n):
        L = rng.randint(0, 32) if length is None else length
        s = [rng.choice(filler) for _ in range(L)]
        r = rng.random()
        if L >= len(needle) and r < p_match + p_letters:
            letters = list(needle) if r < p_match else list(reversed(needle))
            for q, ch in zip(sorted(rng.sample(range(L), len(needle))), letters):
                s[q] = ch if rng.random() < 0.9 else ch.swapcase()  # (a needle with an uppercase letter respects case: most planted rows still match)
        out.append("".join(s))
    return out


@pytest.mark.parametrize("length", [16, 32, None], ids=["len16", "len32", "ragged0-32"])
def test_list_sizes_and_lengths(dev, length):
    rng = random.Random(100 + (length or 0))
    m = F.Matcher("DeadBe", fcfg())
    total = 0
    for n in SIZES:
        hs = make_rows(rng, n, length, "DeadBe", p_match=0.2)
        cp = F.Corpus(hs)
        assert cp.signature_info() == (True, 4 * n)
        assert cp.debug_read("sig").tolist() == want_sig([h.encode() for h in hs]).tolist()
        assert cp.info()["uniform_len"] == (length or 0) or n == 1
        total += check(dev, m, "DeadBe", cp, hs)
    assert total > 500


def tile_of(rng, passing, accepted, needle="deadbe"):
    """one 1024-haystack tile of 32-byte rows: `passing` rows hold the needle's letters (the first `accepted` of them in order), shuffled"""
    rows = make_rows(rng, 1024 - passing, 32, needle, 0.0, 0.0)
    rows += make_rows(rng, accepted, 32, needle, 1.0, 0.0) + make_rows(rng, passing - accepted, 32, needle, 0.0, 1.0)
    rng.shuffle(rows)
    return rows


def test_both_tile_branches_and_the_threshold_between_them(dev):
    rng = random.Random(7)
    T = int(F.lib().fzb_debug_signature_threshold())
    assert 2 <= T < 1023
    # every row passes | none passes | threshold - 1, threshold, threshold + 1 passing rows | every row passes the signature and fails the automaton
    # (the needle's letters in the wrong order) | a short last tile
    hs = tile_of(rng, 1024, 700) + tile_of(rng, 0, 0) + tile_of(rng, T - 1, T // 2) + tile_of(rng, T, T // 2) + tile_of(rng, T + 1, T // 2) + tile_of(rng, 1024, 0)
    hs += tile_of(rng, 300, 100)[:77]
    cp = F.Corpus(hs)
    sig = cp.debug_read("sig")
    assert sig.tolist() == want_sig([h.encode() for h in hs]).tolist()
    ns = py_sig(b"deadbe")
    per_tile = [int(((sig[t * 1024:(t + 1) * 1024] & ns) == ns).sum()) for t in range(6)]
    assert per_tile == [1024, 0, T - 1, T, T + 1, 1024], per_tile
    m = F.Matcher("deadbe", fcfg())
    got = dev.run(m, cp)
    k = check(dev, m, "deadbe", cp, hs)
    idx = got["index"]
    assert k == len(got) and ((idx >= 1024) & (idx < 2048)).sum() == 0 and (idx >= 5 * 1024).sum() == (idx >= 6 * 1024).sum()
    # bit-sharing bytes: the needle a_6 against rows that hold a, _ and 0 (48 % 6 == 54 % 6) but no 6
    rows = ["a_0" + "x" * 29] * 500 + ["xa_x6" + "y" * 27] * 30 + ["6_a" + "z" * 29] * 20 + ["A_6" + "q" * 29] * 10
    rng.shuffle(rows)
    cp2 = F.Corpus(rows)
    m2 = F.Matcher("a_6", fcfg())
    assert check(dev, m2, "a_6", cp2, rows) == 40
    ns2 = py_sig(b"a_6")
    assert int(((cp2.debug_read("sig") & ns2) == ns2).sum()) == len(rows)


def test_sub_ranges_and_offsets(dev):
    rng = random.Random(11)
    hs = make_rows(rng, 4097, 32, "deadbe", p_match=0.15)
    cp = F.Corpus(hs)
    rg = make_rows(rng, 3000, None, "deadbe", p_match=0.15)
    cpr = F.Corpus(rg)
    m = F.Matcher("deadbe", fcfg())
    total = 0
    for first in (0, 1, 3, 1029):
        for count in (1500, 4097 - first, 1):   # ends inside a tile (of the range) | to the end of the list | a single row
            total += check(dev, m, "deadbe", cp, hs, first, count)
        total += check(dev, m, "deadbe", cpr, rg, first, 1100)
    assert total > 1000
    assert check(dev, m, "deadbe", cp, hs, 3, 2500, index_offset=123456) > 100


def test_needles(dev):
    rng = random.Random(13)
    long32 = "abcdefghijklmnopqrstuvwxyzabcdef"
    assert len(long32) == 32
    base = make_rows(rng, 2500, 32, "DeadBe", p_match=0.1) + make_rows(rng, 300, 32, "a_1", 0.3, 0.3) + make_rows(rng, 300, 32, "zz", 0.3, 0.0)
    base += [long32, long32.upper(), long32[:31] + "_", long32[1:] + "a", "z" + "q" * 31, "zZ" + "-" * 30] * 20
    base += ["dé" + "x" * 29, "d" + "x" * 10 + "é" + "y" * 19, "de\0d" + "x" * 28, "dead\0be" + "w" * 25] * 25
    rng.shuffle(base)
    hs = [h.encode() if isinstance(h, str) else h for h in base]
    hs = [h[:32] for h in hs]
    cp = F.Corpus(hs)
    assert cp.signature_info()[0]

    def eligible(m):
        el = C.c_int()
        assert F.lib().fzb_debug_needle_signature(m.h, None, C.byref(el)) == 0
        return bool(el.value)

    for needle in ("DeadBe", "a_1", "zz", long32):
        m = F.Matcher(needle, fcfg())
        assert eligible(m)
        assert check(dev, m, needle, cp, hs) > 0, needle
    # one ineligible needle of each kind: the old kernel (or its own path), and still the oracle's records
    for needle, kw, okw in (("de\0d", {}, {}), ("dé", dict(unicode=F.UnicodeMatching.Ignore), dict(unicode="Ignore")), ("dé", {}, {}), ("deadbe", dict(max_typos=1), dict(max_typos=1)),
                            ("deadbe", dict(max_typos=None), dict(max_typos=None)), ("dead", dict(matching=F.Matching.Substring), dict(matching="Substring")),
                            ("zz", dict(matching=F.Matching.Prefix), dict(matching="Prefix"))):
        m = F.Matcher(needle, fcfg(**kw))
        assert not eligible(m)
        assert check(dev, m, needle, cp, hs, **okw) > 0, (needle, kw)
    # set_pattern on one matcher: eligible -> not -> eligible, the signature follows
    m = F.Matcher("zz", fcfg())
    for needle in ("zz", "de\0d", "a_1"):
        m.set_pattern(needle)
        check(dev, m, needle, cp, hs)


def test_corpus_edits_keep_the_signatures(dev):
    rng = random.Random(17)
    hs = [h.encode() for h in make_rows(rng, 3000, None, "deadbe", p_match=0.15)]
    extra = [h.encode() for h in make_rows(rng, 700, None, "deadbe", p_match=0.3)]
    m = F.Matcher("deadbe", fcfg())
    cp = F.Corpus(hs)

    def same_as_fresh(cur):
        assert len(cp) == len(cur) and cp.signature_info() == (True, 4 * len(cur))
        assert cp.debug_read("sig").tolist() == want_sig(cur).tolist()
        fresh = F.Corpus(cur)
        got = dev.run(m, cp)
        assert got.tolist() == dev.run(m, fresh).tolist() == oracle("deadbe", cur).tolist() and len(got) > 100

    cur = hs + extra
    cp.append(extra)
    same_as_fresh(cur)
    idx = sorted(rng.sample(range(len(cur)), 40))
    new = [h.encode() for h in make_rows(rng, 40, None, "deadbe", p_match=0.5)]
    cp.replace(idx, new)
    for i, h in zip(idx, new):
        cur[i] = h
    same_as_fresh(cur)
    drop = set(rng.sample(range(len(cur)), 55))
    cp.remove(sorted(drop))
    cur = [h for i, h in enumerate(cur) if i not in drop]
    same_as_fresh(cur)
    cp.truncate(2049)
    cur = cur[:2049]
    same_as_fresh(cur)
    # a haystack beyond 32 bytes: the list leaves k1_dfa's lists and the signatures go; removed again, they are rebuilt
    cp.append([b"d" * 40])
    assert cp.signature_info() == (False, 0) and len(cp.debug_read("sig")) == 0
    assert dev.run(m, cp).tolist() == oracle("deadbe", cur + [b"d" * 40]).tolist()
    cp.truncate(2049)
    same_as_fresh(cur)
    # reserved room: appends inside it allocate nothing, signatures included
    cq = F.Corpus([])
    cq.reserve(len(hs), 48 * len(hs))
    m.reserve(cq)
    before = F.device_allocs()
    for b in range(3):
        cq.append(hs[b * 1000:(b + 1) * 1000])
        assert dev.run(m, cq).tolist() == oracle("deadbe", hs[:(b + 1) * 1000]).tolist()
    assert F.device_allocs() == before
    assert cq.debug_read("sig").tolist() == want_sig(hs).tolist()


def test_sharded_corpus(dev):
    rng = random.Random(19)
    hs = make_rows(rng, 5000, 32, "deadbe", p_match=0.15)
    sc = F.ShardedCorpus(hs, ndev=3, oversubscribe=True)
    assert len(sc.shards()) == 3
    m = F.Matcher("deadbe", F.Config(pf_lanes=64, sw_lanes=64))
    want = O.Matcher("deadbe", lanes=LANES).match_list(hs)
    got = m.match_list_parallel_sharded(sc)
    assert len(want) > 300 and got.tolist() == want.tolist()
    with no_signature():
        assert m.match_list_parallel_sharded(sc).tolist() == want.tolist()


def test_borrowed_corpus_gets_and_drops_the_signatures(dev):
    from test_gpu_edges import padded16
    rng = random.Random(23)
    hs = [h.encode() for h in make_rows(rng, 2500, 32, "deadbe", p_match=0.15)]
    cp = padded16(hs, torch.device("cuda", 0), False)
    m = F.Matcher("deadbe", fcfg())
    assert cp.signature_info() == (False, 0)
    want = oracle("deadbe", hs).tolist()
    assert dev.run(m, cp).tolist() == want
    F._check(F.lib().fzb_corpus_set_uniform_len(cp.h, 32))
    assert cp.signature_info() == (True, 4 * len(hs)) and cp.debug_read("sig").tolist() == want_sig(hs).tolist()
    assert check(dev, m, "deadbe", cp, hs) == len(want)
    F._check(F.lib().fzb_corpus_set_uniform_len(cp.h, 0))   # the promise cleared: the signatures go, the query still agrees
    assert cp.signature_info() == (False, 0)
    assert dev.run(m, cp).tolist() == want
    F._check(F.lib().fzb_corpus_set_max_len(cp.h, 32))      # the bound alone (end offsets are read)
    assert cp.signature_info()[0] and check(dev, m, "deadbe", cp, hs) == len(want)
    F._check(F.lib().fzb_corpus_set_max_len(cp.h, 64))      # loosened beyond 32
    assert cp.signature_info() == (False, 0) and dev.run(m, cp).tolist() == want
    rg = [h.encode() for h in make_rows(rng, 1500, None, "deadbe", p_match=0.2)]
    cr = padded16(rg, torch.device("cuda", 0), True)
    F._check(F.lib().fzb_corpus_set_max_len(cr.h, 32))
    assert cr.debug_read("sig").tolist() == want_sig(rg).tolist()
    assert check(dev, m, "deadbe", cr, rg) > 100
