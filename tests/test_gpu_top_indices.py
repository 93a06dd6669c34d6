"""Top-`limit` with matched positions in one fused device call (fzb_match_list_top_indices / _device / fzb_matcher_reserve_top_indices /
fzb_multi_match_list_top_indices): the first min(limit, found) elements of what `Matcher::match_list_indices` returns over the whole list
(src/matcher/mod.rs:234-275), `index` = the corpus index, and `found`.  The reference has no such call - its caller truncates the Vec - so
every expected value here is the ORACLE's full `match_list_indices` list cut on the host, never this library's own `match_list_top` or
`match_list_indices`.

A note on the inputs of test_random_parity_with_cuts_through_tie_groups.  The packing step's scan is only exercised by heads whose records
have DIFFERENT numbers of positions.  On `synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=0..2)` the best 100 records of a Score*
query nearly always matched every needle byte: by the oracle, the first 100 records all have 8 / 4 / 2 positions for (`deadbeef`, 0) /
(`dead`, 0) / (`db`, None) on every seed (a 0-typo match has every needle byte by definition), and for (`deadbeef`, 1) they have {7, 8} on
seeds 0 and 1 but 8 throughout on seed 2.  "The first 100 records of every query with >= 100 matches differ in positions_len" therefore
cannot hold on these inputs whatever is under test; what holds, and is asserted from the oracle's lists alone, is that every seed's
(`deadbeef`, 1) heads of 1000 and more records carry at least three different lengths, some below the needle's - and the same query in
IndexAsc order, added to the set, has mixed lengths within its first 100 records (the one-launch pack of the picker's case)."""
import json
import os
import sys

import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from test_gpu_long_needles import haystacks_for, rand_text
from test_gpu_multi_requery import KEYS, hip_patterns
from test_gpu_parity import LANES, _expand
from test_gpu_topk import SORTS, limits_around, single
from test_oracle_multi import pats as oracle_pats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
MT = json.load(open(os.path.join(G, "matcher.json")))
IX = json.load(open(os.path.join(G, "indices.json")))
MU = json.load(open(os.path.join(G, "multi.json")))
LT = json.load(open(os.path.join(G, "literal.json")))


def unpack(data, ends):
    raw = data.tobytes()
    out, start = [], 0
    for e in ends.tolist():
        out.append(raw[start:e])
        start = e
    return out


def tuples(ms):
    return [(m.index, m.score, m.exact, m.indices) for m in ms]


def assert_top_indices(got, want, limit, ctx=""):
    """got = (list[MatchIndices], found); want = the oracle's full ordered list of (index, score, exact, indices)"""
    recs, found = got
    assert found == len(want), (ctx, limit, found, len(want))
    got_t, exp = tuples(recs), want[:limit]
    if got_t != exp:
        bad = [(i, g, w) for i, (g, w) in enumerate(zip(got_t, exp)) if g != w][:4]
        raise AssertionError(f"{ctx} limit {limit}: len {len(got_t)} vs {len(exp)}; first diffs (at, got, want) {bad}")


@pytest.mark.parametrize("sort", SORTS)
def test_reference_known_answers_cut_at_every_limit(sort):
    cases = [(c["needle"], _expand(c["haystacks"]), dict(c["config"]), c["name"]) for c in MT["cases"]]
    cases += [(needle, [haystack], dict(max_typos=None), ref) for needle, haystack, _, ref in IX["ascii"]]
    cases += [(needle, [haystack], dict(max_typos=None), ref) for needle, haystack, start, _, ref in IX["unicode"] if start == 0]
    for needle, hs, cfg, name in cases:
        cfg["sort"] = sort
        fm, om = single(needle, **cfg)
        want = om.match_list_indices_ordered(hs)
        cp = F.Corpus(hs)
        for limit in limits_around(len(want)):
            assert_top_indices(fm.match_list_top_indices(cp, limit), want, limit, name)


def test_random_parity_with_cuts_through_tie_groups():
    """Records AND positions, limits on both sides of the pack's 2048-record tile.  Asserted from the oracle's lists alone: at least half
    of the (query, limit) pairs of the Score* set have found > limit, at least a quarter cut through a group of equal scores, and the
    heads carry records with different numbers of positions (see the module docstring for what these inputs can and cannot show)."""
    limits = (0, 1, 2, 10, 100, 1000, 2049, 4096)
    pairs = beyond = through_tie = 0
    for seed in range(3):
        data, ends = synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=seed)
        cp = F.Corpus(packed=(data, ends))
        hs = unpack(data, ends)
        for needle, typos in (("deadbeef", 0), ("dead", 0), ("deadbeef", 1), ("db", None)):
            for sort in ("ScoreThenIndexAsc", "ScoreThenIndexDesc"):
                fm, om = single(needle, sort=sort, max_typos=typos)
                want = om.match_list_indices_ordered(hs)
                for limit in limits:
                    assert_top_indices(fm.match_list_top_indices(cp, limit), want, limit, (seed, needle, typos, sort))
                    pairs += 1
                    beyond += len(want) > limit
                    through_tie += 0 < limit < len(want) and want[limit - 1][1] == want[limit][1]
                if (needle, typos) == ("deadbeef", 1):
                    for limit in (1000, 2049, 4096):
                        lens = {len(w[3]) for w in want[:limit]}
                        assert len(lens) >= 3 and min(lens) < len(needle), (seed, sort, limit, sorted(lens))
        # the same typo query in list order: mixed lengths inside the first 100 records, and across the tile boundary
        fm, om = single("deadbeef", sort="IndexAsc", max_typos=1)
        want = om.match_list_indices_ordered(hs)
        assert len({len(w[3]) for w in want[:100]}) >= 3 and len(want) > 2049, seed
        for limit in (100, 2049):
            assert_top_indices(fm.match_list_top_indices(cp, limit), want, limit, (seed, "IndexAsc"))
    print(f"pairs {pairs}, found > limit {beyond}, cut through a tie group {through_tie}")
    assert pairs == 192
    assert 2 * beyond >= pairs and 4 * through_tie >= pairs, (pairs, beyond, through_tie)


def test_both_score_ranges():
    """scores on both sides of 256 (test_gpu_topk.py::test_both_selection_levels asserts it for this input): both radix passes order the head"""
    needle = "deadbeefdeadbeefdead"
    data, ends = synth.ragged_corpus(needle.encode(), 30_000, 4, 96, seed=1)
    cp = F.Corpus(packed=(data, ends))
    hs = unpack(data, ends)
    for sort in ("ScoreThenIndexAsc", "ScoreThenIndexDesc"):
        fm, om = single(needle, sort=sort, max_typos=2)
        want = om.match_list_indices_ordered(hs)
        assert want[99][1] >= 256 > want[999][1]
        for limit in (100, 1000):
            assert_top_indices(fm.match_list_top_indices(cp, limit), want, limit, (needle, sort))


def test_unicode_literal_empty_pattern_no_match_and_empty_corpus():
    data, ends = synth.utf8_corpus(50_000, 32)
    cp = F.Corpus(packed=(data, ends))
    hs = unpack(data, ends)
    for sort in SORTS:
        fm, om = single("إنما", sort=sort)
        want = om.match_list_indices_ordered(hs)
        assert len(want) > 200
        for limit in (0, 1, 100, len(want) - 1, len(want), len(want) + 1, 60_000):
            assert_top_indices(fm.match_list_top_indices(cp, limit), want, limit, ("utf8", sort))
    data, ends = synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=2)
    cp = F.Corpus(packed=(data, ends))
    hs = unpack(data, ends)
    for sort in SORTS:
        for needle, kw in (("dead", {"matching": "Substring"}), ("de", {"matching": "Prefix"})):
            fm, om = single(needle, sort=sort, **kw)
            want = om.match_list_indices_ordered(hs)
            assert len(want) > 100
            for limit in (0, 1, 7, 100, 2049, len(want), len(want) + 5, 40_000):
                assert_top_indices(fm.match_list_top_indices(cp, limit), want, limit, (needle, kw, sort))
        # CompiledPatterns::Empty: every haystack, score 0, no positions; the first `limit` indices or the last `limit` reversed
        want = O.Matcher("", sort=sort).match_list_indices_ordered(hs)
        assert len(want) == 30_000 and all(w[3] == [] for w in want[:10])
        for limit in (0, 1, 100, 30_000, 40_000):
            assert_top_indices(F.Matcher("", F.Config(sort=F.SortStrategy[sort])).match_list_top_indices(cp, limit), want, limit, ("empty needle", sort))
            assert_top_indices(F.MultiMatcher([], F.Config(sort=F.SortStrategy[sort])).match_list_top_indices(cp, limit), want, limit, ("no pattern", sort))
        # nothing matches at all
        for limit in (0, 1, 100):
            recs, found = F.Matcher("@@##", F.Config(sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=64)).match_list_top_indices(cp, limit)
            assert found == 0 and recs == []
            recs, found = F.MultiMatcher(F.parse_query("@@## dead"), F.Config(sort=F.SortStrategy[sort], pf_lanes=64)).match_list_top_indices(cp, limit)
            assert found == 0 and recs == []
    for m in (F.Matcher("abc"), F.Matcher(""), F.MultiMatcher(F.parse_query("abc !d"))):
        recs, found = m.match_list_top_indices([], 5)
        assert found == 0 and recs == []


def test_long_needle():
    """a needle beyond the by-value NeedleDev (> 64 bytes): the traced form of the long-needle pipeline through the same call"""
    rng = np.random.default_rng(11)
    needle = rand_text(rng, 80, b"abcdefgh_/")
    hs = haystacks_for(rng, needle, 2000)
    hs = [h if 100 <= len(h) <= 200 else (h + rand_text(rng, 100 + int(rng.integers(0, 60))))[:200] for h in hs]
    cp = F.Corpus(hs)
    for typos, sort in ((0, "ScoreThenIndexAsc"), (2, "ScoreThenIndexDesc")):
        want = O.Matcher(needle, max_typos=typos, sort=sort).match_list_indices_ordered(hs)
        assert len(want) > 20, len(want)
        fm = F.Matcher(needle, F.Config(max_typos=typos, sort=F.SortStrategy[sort], pf_lanes=64))
        for limit in (10, len(want), len(want) + 100):
            assert_top_indices(fm.match_list_top_indices(cp, limit), want, limit, ("long", typos, sort))


def test_device_form_into_torch_tensors():
    import torch

    data, ends = synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=4)
    cp = F.Corpus(packed=(data, ends))
    hs = unpack(data, ends)
    needle = "deadbeef"
    nb = len(needle)
    for sort in SORTS:
        fm, om = single(needle, sort=sort, max_typos=1)
        want = om.match_list_indices_ordered(hs)
        for limit in (0, 1, 100, 2049, len(want), 10 * len(want)):
            cap = min(limit, len(cp))
            out = torch.zeros((max(cap, 1), 4), dtype=torch.int32, device="cuda")
            pos = torch.full((max(cap * nb, 1),), -1, dtype=torch.int32, device="cuda")
            cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            fm.match_list_top_indices_device(cp, limit, out.data_ptr(), cap, pos.data_ptr(), cap * nb, cnt.data_ptr())
            torch.cuda.synchronize()
            words = cnt.cpu().numpy().view(np.uint32).tolist()
            exp = want[:limit]
            total = sum(len(w[3]) for w in exp)
            assert words == [min(limit, len(want)), len(want), total, 0], (sort, limit, words)
            recs = out.cpu().numpy().reshape(-1).view(F.MATCH_INDICES_DTYPE)[: words[0]]
            flat = pos.cpu().numpy().view(np.uint32)
            # dense: every record's run starts where the previous one ended, nothing is written behind the total
            begins = np.cumsum([0] + [len(w[3]) for w in exp])[:-1].tolist()
            assert recs["positions_begin"].tolist() == begins
            assert (flat[total:] == 0xFFFFFFFF).all()
            got = [(int(r["index"]), int(r["score"]), bool(r["exact"]), flat[int(r["positions_begin"]) : int(r["positions_begin"]) + int(r["positions_len"])].tolist()) for r in recs]
            assert got == exp, (sort, limit)
        # room for fewer than min(limit, n) records, or for fewer than min(limit, n) x needle bytes positions: refused on the host, nothing launched
        for cap, pcap in ((10, 11 * nb), (11, 11 * nb - 1)):
            out = torch.zeros((11, 4), dtype=torch.int32, device="cuda")
            pos = torch.zeros((11 * nb,), dtype=torch.int32, device="cuda")
            cnt = torch.full((4,), -1, dtype=torch.int32, device="cuda")
            with pytest.raises(F.FrizbeeError) as e:
                fm.match_list_top_indices_device(cp, 11, out.data_ptr(), cap, pos.data_ptr(), pcap, cnt.data_ptr())
            assert e.value.code == 5  # FZB_ERR_CAPACITY
            torch.cuda.synchronize()
            assert cnt.cpu().tolist() == [-1, -1, -1, -1]
    with pytest.raises(F.FrizbeeError) as e:  # the empty needle is the host form's
        F.Matcher("").match_list_top_indices_device(cp, 1, out.data_ptr(), 11, pos.data_ptr(), 11 * nb, cnt.data_ptr())
    assert e.value.code == 1
    # an empty corpus zeroes the four words
    F.Matcher("abc").match_list_top_indices_device(F.Corpus([]), 5, out.data_ptr(), 11, pos.data_ptr(), 11 * nb, cnt.data_ptr())
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [0, 0, 0, 0]


def test_no_device_allocation_after_reserve():
    data, ends = synth.paths_corpus()
    ends = ends[:200_000]
    data = data[: int(ends[-1])]
    cp = F.Corpus(packed=(data, ends))
    fm = F.Matcher("srclinuxtest", F.Config(pf_lanes=64, sw_lanes=64))
    fm.reserve(cp)
    fm.reserve_top_indices(cp, 1000, 12)
    before = F.device_allocs()
    for key in KEYS:
        for limit in (1, 100, 1000):
            fm.set_pattern(key.replace(" ", "").replace("!", ""))
            recs, found = fm.match_list_top_indices(cp, limit)
            assert len(recs) == min(limit, found)
    last = fm.match_list_top_indices(cp, 1000)
    fm.set_config(F.Config(pf_lanes=64, sw_lanes=64, sort=F.SortStrategy.ScoreThenIndexDesc))
    fm.set_pattern("srclinux")
    got = fm.match_list_top_indices(cp, 100)
    assert F.device_allocs() == before
    # and what the replay answered is right
    hs = unpack(data, ends)
    assert_top_indices(last, O.Matcher("srclinuxtest").match_list_indices_ordered(hs), 1000, "srclinuxtest")
    want = O.Matcher("srclinux", sort="ScoreThenIndexDesc").match_list_indices_ordered(hs)
    assert len(want) > 100
    assert_top_indices(got, want, 100, "srclinux")


def test_interleaving_on_one_matcher():
    """the fused query shares the sort's buffers, the staging and the matched-indices scratch with the matcher's other entry points"""
    data, ends = synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=5)
    cp = F.Corpus(packed=(data, ends))
    hs = unpack(data, ends)
    odata = np.concatenate([data, np.zeros(64, np.uint8)])
    fm, om = single("deadbeef", sort="ScoreThenIndexDesc", max_typos=1)

    def rounds(om, needle, n):
        full = om.match_packed(odata, ends)
        full_ix = om.match_list_indices_ordered(hs)
        in_order = sorted(full.tolist(), key=lambda r: r[0])
        for _ in range(n):
            recs, found = fm.match_list_top(cp, 50)
            assert recs.tolist() == full[:50].tolist() and found == len(full)
            assert fm.match_list(cp).tolist() == full.tolist()
            assert_top_indices(fm.match_list_top_indices(cp, 300), full_ix, 300, needle)
            sel = full["index"][:40]
            sub = O.Matcher(needle, sort="ScoreThenIndexDesc", max_typos=1).match_list_indices_ordered([hs[i] for i in sel])
            assert tuples(fm.match_list_indices(cp, selection=sel)) == sub
            assert fm.match_list_into(cp).tolist() == in_order
            assert_top_indices(fm.match_list_top_indices(cp, 3000), full_ix, 3000, needle)

    rounds(om, "deadbeef", 2)
    fm.set_pattern("dead")
    rounds(O.Matcher("dead", sort="ScoreThenIndexDesc", max_typos=1), "dead", 1)
    fm.set_config(F.Config(pf_lanes=64, sw_lanes=64, max_typos=0, sort=F.SortStrategy.IndexAsc))
    want = O.Matcher("dead", sort="IndexAsc", max_typos=0).match_list_indices_ordered(hs)
    assert_top_indices(fm.match_list_top_indices(cp, 77), want, 77, "after set_config")


def test_edited_corpus():
    rng = np.random.default_rng(3)
    data, ends = synth.ragged_corpus(b"deadbeef", 5_000, 4, 96, seed=6)
    hs = unpack(data, ends)
    cp = F.Corpus(hs)
    fm, _ = single("deadbeef", sort="ScoreThenIndexAsc", max_typos=1)

    def check(ctx):
        want = O.Matcher("deadbeef", sort="ScoreThenIndexAsc", max_typos=1).match_list_indices_ordered(hs)
        assert len(want) > 100
        for limit in (10, 100, len(want) + 1):
            assert_top_indices(fm.match_list_top_indices(cp, limit), want, limit, ctx)

    check("fresh")
    batch = [b"xx_deadbeef_%d" % i for i in range(30)] + [b"dead/beef", b"", b"deadbee"]
    cp.append(batch)
    hs += batch
    check("append")
    drop = sorted({int(x) for x in rng.integers(0, len(hs), 40)} | {0, len(hs) - 1})
    cp.remove(drop)
    gone = set(drop)
    hs = [h for i, h in enumerate(hs) if i not in gone]
    check("remove")
    at = sorted({int(x) for x in rng.integers(0, len(hs), 25)})
    new = [b"deadbeef" if i % 3 == 0 else b"d_e_a_d_b_e_e_f" * (1 + i % 4) if i % 3 == 1 else b"nothing" for i in range(len(at))]
    cp.replace(at, new)
    for i, h in zip(at, new):
        hs[i] = h
    check("replace")


@pytest.mark.parametrize("sort", SORTS)
def test_multi_pattern_known_answers_cut_at_every_limit(sort):
    cases = [(hip_patterns(oracle_pats(c)), oracle_pats(c), c["haystacks"], c["config"], c["name"]) for c in MU["cases"]]
    cases += [(F.parse_query(q), O.parse_query(q), hs, cfg, q) for q, hs, cfg, _, _ in LT["multi_queries"]]
    for fpats, opats, hs, cfg, name in cases:
        cfg = dict(cfg)
        cfg["sort"] = sort
        want = O.MultiMatcher(opats, lanes=LANES[64], **cfg).match_list_indices_ordered(hs)
        fc = F.Config(max_typos=cfg.get("max_typos", 0), casing=F.CaseMatching[cfg.get("casing", "Smart")], sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=0)
        mm = F.MultiMatcher(fpats, fc)
        cp = F.Corpus(hs)
        for limit in limits_around(len(want)):
            assert_top_indices(mm.match_list_top_indices(cp, limit), want, limit, name)


def test_multi_pattern_over_a_large_list():
    data, ends = synth.ragged_corpus(b"deadbeef", 30_000, 4, 96, seed=1)
    cp = F.Corpus(packed=(data, ends))
    hs = unpack(data, ends)
    q = "dead be !x"
    for sort in ("ScoreThenIndexAsc", "ScoreThenIndexDesc"):
        want = O.MultiMatcher(O.parse_query(q), sort=sort).match_list_indices_ordered(hs)
        assert len(want) > 500
        mm = F.MultiMatcher(F.parse_query(q), F.Config(sort=F.SortStrategy[sort], pf_lanes=64))
        for limit in (10, 500):
            assert_top_indices(mm.match_list_top_indices(cp, limit), want, limit, (q, sort))
