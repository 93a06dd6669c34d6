"""A per-haystack score bias on a resident corpus (fzb_corpus_set_bias / _update_bias / _clear_bias): every record's score becomes
clamp(score + bias[index], 0, 65535) on the device, between the scorers and the selection / ordering stage.  The reference has no such
term - its caller adds it on the host and sorts again - so every expected value here is the ORACLE's IndexAsc records, plus the bias and
the clamp in numpy, plus the reference's ordering rule in numpy (reverse for the *Desc strategies, then argsort(-score, kind="stable") for
the Score* ones: src/matcher/mod.rs:215-221, src/sort.rs:6-40) - never this library's own unbiased result.  The one exception is named
where it is made: the positions of the fused multi-pattern call are held to the unbiased call's, per index."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from test_gpu_multi_requery import hip_patterns
from test_gpu_parity import LANES, _expand
from test_gpu_topk import SORTS, assert_top, limits_around, opad, single
from test_oracle_multi import pats as oracle_pats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
MT = json.load(open(os.path.join(G, "matcher.json")))
MU = json.load(open(os.path.join(G, "multi.json")))
LT = json.load(open(os.path.join(G, "literal.json")))
PATHS = dict(root=ROOT, tests=os.path.join(ROOT, "tests"), tools=os.path.join(ROOT, "tools"))


def biased(index_asc, bias, sort, first=0, index_offset=0):
    """the oracle's IndexAsc records -> what a biased corpus must report under `sort`"""
    w = index_asc.copy()
    at = w["index"].astype(np.int64) - index_offset + first
    w["score"] = np.clip(w["score"].astype(np.int64) + np.asarray(bias, np.int64)[at], 0, 65535).astype(np.uint16)
    if sort in ("IndexDesc", "ScoreThenIndexDesc"):
        w = w[::-1]
    if sort in ("ScoreThenIndexAsc", "ScoreThenIndexDesc"):
        w = w[np.argsort(-w["score"].astype(np.int64), kind="stable")]
    return np.ascontiguousarray(w)


def unpack(data, ends):
    raw = np.asarray(data, np.uint8).tobytes()
    out, start = [], 0
    for e in np.asarray(ends).tolist():
        out.append(raw[start:e])
        start = e
    return out


def same(got, want, ctx=""):
    if got.tolist() != want.tolist():
        n = min(len(got), len(want))
        bad = [(i, got[i].tolist(), want[i].tolist()) for i in range(n) if got[i].tolist() != want[i].tolist()][:5]
        raise AssertionError(f"{ctx}: len {len(got)} vs {len(want)}; first diffs (at, got, want) {bad}")


def small_bias(n, seed):
    return np.random.default_rng(seed).integers(-40, 41, n).astype(np.int16)


@pytest.mark.parametrize("sort", SORTS)
def test_reference_known_answers_with_a_bias(sort):
    for k, case in enumerate(MT["cases"]):
        hs = _expand(case["haystacks"])
        cfg = dict(case["config"])
        cfg.pop("sort", None)
        fm, _ = single(case["needle"], sort=sort, **cfg)
        _, om = single(case["needle"], sort="IndexAsc", **cfg)
        bias = small_bias(len(hs), k)
        want = biased(om.match_list(hs), bias, sort)
        cp = F.Corpus(hs)
        cp.set_bias(bias)
        same(fm.match_list(cp), want, case["name"])
        for limit in limits_around(len(want)):
            assert_top(fm.match_list_top(cp, limit), want, limit, case["name"])


@pytest.mark.parametrize("sort", SORTS)
def test_multi_pattern_known_answers_with_a_bias(sort):
    cases = [(hip_patterns(oracle_pats(c)), oracle_pats(c), c["haystacks"], c["config"], c["name"]) for c in MU["cases"]]
    cases += [(F.parse_query(q), O.parse_query(q), hs, cfg, q) for q, hs, cfg, _, _ in LT["multi_queries"]]
    for k, (fpats, opats, hs, cfg, name) in enumerate(cases):
        cfg = dict(cfg)
        cfg["sort"] = "IndexAsc"
        bias = small_bias(len(hs), 100 + k)
        want = biased(O.MultiMatcher(opats, lanes=LANES[64], **cfg).match_list(hs), bias, sort)
        fc = F.Config(max_typos=cfg.get("max_typos", 0), casing=F.CaseMatching[cfg.get("casing", "Smart")], sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=0)
        mm = F.MultiMatcher(fpats, fc)
        cp = F.Corpus(hs)
        cp.set_bias(bias)
        same(mm.match_list(cp), want, name)
        for limit in limits_around(len(want)):
            assert_top(mm.match_list_top(cp, limit), want, limit, name)


# ---- one corpus, one oracle run, shared by the tests below (never modified: every test uploads its own Corpus) -----------------------
class Fixed:
    rows, ends = synth.fixed_corpus(b"deadbe", 5000, 32, seed=7)
    data = rows.numpy().reshape(-1).copy()
    bias = np.random.default_rng(1).choice([0, 200, -32768, -5, 7], 5000).astype(np.int16)
    _asc = None
    _idx = None

    @classmethod
    def index_asc(cls):
        if cls._asc is None:
            cls._asc = O.Matcher("deadbe", sort="IndexAsc").match_packed(opad(cls.data), cls.ends)
        return cls._asc

    @classmethod
    def positions(cls):
        """index -> the oracle's matched positions (reverse byte order)"""
        if cls._idx is None:
            recs, idx = O.Matcher("deadbe", sort="IndexAsc").match_list_indices(unpack(cls.data, cls.ends))
            assert recs.tolist() == cls.index_asc().tolist()
            cls._idx = {int(r["index"]): ix for r, ix in zip(recs, idx)}
        return cls._idx

    @classmethod
    def corpus(cls):
        return F.Corpus(packed=(cls.data, cls.ends))


LIMITS = (0, 1, 10, 41, 42, 43, 100, 208, 209, 210, 254, 255, 256, 5000)


@pytest.mark.parametrize("sort", ["ScoreThenIndexAsc", "ScoreThenIndexDesc"])
def test_both_selection_levels_through_the_bias(sort):
    asc = Fixed.index_asc()
    # what makes the test mean something, from the oracle alone: one pass without the bias, both levels with it, cuts through tie groups
    assert len(asc) == 255 and int(asc["score"].min()) == 51 and int(asc["score"].max()) == 84
    s = np.clip(asc["score"].astype(np.int64) + Fixed.bias[asc["index"]].astype(np.int64), 0, 65535)
    assert (int((s >= 256).sum()), int(((s >= 1) & (s <= 255)).sum()), int((s == 0).sum())) == (42, 167, 46)
    want = biased(asc, Fixed.bias, sort)
    assert want[0]["score"] == want[1]["score"] and want[99]["score"] == want[100]["score"]
    cp = Fixed.corpus()
    cp.set_bias(Fixed.bias)
    info = cp.bias_info()
    assert info["has_bias"] == 1 and info["bias_hi"] == 200 and info["capacity"] >= 5000
    fm = F.Matcher("deadbe", F.Config(sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=64))
    same(fm.match_list(cp), want, sort)
    same(fm.match_list_parallel(cp, 3), want, sort)
    pos = Fixed.positions()
    for limit in LIMITS:
        assert_top(fm.match_list_top(cp, limit), want, limit, sort)
        recs, found = fm.match_list_top_indices(cp, limit)
        assert found == 255
        got = [(m.index, m.score, m.exact, m.indices) for m in recs]
        exp = [(int(r["index"]), int(r["score"]), bool(r["exact"]), pos[int(r["index"])]) for r in want[:limit]]
        assert got == exp, (sort, limit, [(g, e) for g, e in zip(got, exp) if g != e][:3])


def test_a_small_bias_keeps_one_pass_and_still_orders():
    """bias_hi = 7: max matrix score + exact bonus + 7 stays below 256 (score_bias.h decides), the single radix pass / histogram level serves"""
    asc = Fixed.index_asc()
    bias = np.random.default_rng(2).choice([0, -5, 7, -32768], 5000).astype(np.int16)
    cp = Fixed.corpus()
    cp.set_bias(bias)
    assert cp.bias_info()["bias_hi"] == 7
    for sort in SORTS:
        want = biased(asc, bias, sort)
        fm = F.Matcher("deadbe", F.Config(sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=64))
        same(fm.match_list(cp), want, sort)
        for limit in (1, 10, 100, 254, 255):
            assert_top(fm.match_list_top(cp, limit), want, limit, sort)


def test_range_form_follows_first_and_index_offset():
    asc = Fixed.index_asc()
    sub = asc[(asc["index"] >= 1000) & (asc["index"] < 4000)].copy()
    assert len(sub) == 149
    sub["index"] = sub["index"] - 1000 + 7_000_000
    want = biased(sub, Fixed.bias, "IndexAsc", first=1000, index_offset=7_000_000)
    cp = Fixed.corpus()
    cp.set_bias(Fixed.bias)
    fm = F.Matcher("deadbe", F.Config(pf_lanes=64, sw_lanes=64))
    same(fm.match_list_into(cp, first=1000, count=3000, index_offset=7_000_000), want, "range")
    mm = F.MultiMatcher(["deadbe"], F.Config(pf_lanes=64))
    same(mm.match_list_into(cp, first=1000, count=3000, index_offset=7_000_000), want, "range (multi, one pattern)")


def test_matched_indices_forms_carry_the_bias():
    asc, pos = Fixed.index_asc(), Fixed.positions()
    cp = Fixed.corpus()
    cp.set_bias(Fixed.bias)
    for sort in ("ScoreThenIndexAsc", "IndexDesc"):
        want = biased(asc, Fixed.bias, sort)
        fm = F.Matcher("deadbe", F.Config(sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=64))
        got = [(m.index, m.score, m.exact, m.indices) for m in fm.match_list_indices(cp)]
        assert got == [(int(r["index"]), int(r["score"]), bool(r["exact"]), pos[int(r["index"])]) for r in want], sort
    # a selection: `index` numbers the selection, the bias is the selected haystack's
    sel = asc["index"][::-1][:50].copy()
    fm = F.Matcher("deadbe", F.Config(sort=F.SortStrategy.IndexAsc, pf_lanes=64, sw_lanes=64))
    got = fm.match_list_indices(cp, selection=sel)
    score_of = {int(r["index"]): int(r["score"]) for r in biased(asc, Fixed.bias, "IndexAsc")}
    assert [(m.index, m.score, m.indices) for m in got] == [(k, score_of[int(i)], pos[int(i)]) for k, i in enumerate(sel)]


def test_ragged_list_with_typos():
    data, ends = synth.ragged_corpus(b"deadbeef", 3000, 4, 96, seed=3)
    asc = O.Matcher("deadbeef", sort="IndexAsc", max_typos=1).match_packed(opad(data), ends)
    assert len(asc) == 208
    bias = np.random.default_rng(3).choice([0, 300, -32768, -9, 11], 3000).astype(np.int16)
    cp = F.Corpus(packed=(data, ends))
    cp.set_bias(bias)
    for sort in SORTS:
        want = biased(asc, bias, sort)
        fm, _ = single("deadbeef", sort=sort, max_typos=1)
        same(fm.match_list(cp), want, sort)
        for limit in (0, 1, 50, 207, 208, 209):
            assert_top(fm.match_list_top(cp, limit), want, limit, sort)


def test_utf8_list():
    data, ends = synth.utf8_corpus(2000, 32)
    asc = O.Matcher("إنما", sort="IndexAsc").match_packed(opad(data), ends)
    assert len(asc) > 20
    bias = np.random.default_rng(4).choice([0, 250, -32768, -3, 9], 2000).astype(np.int16)
    cp = F.Corpus(packed=(data, ends))
    cp.set_bias(bias)
    for sort in ("ScoreThenIndexAsc", "ScoreThenIndexDesc"):
        want = biased(asc, bias, sort)
        fm, _ = single("إنما", sort=sort)
        same(fm.match_list(cp), want, sort)
        for limit in (1, 10, len(want)):
            assert_top(fm.match_list_top(cp, limit), want, limit, sort)


def test_three_patterns_with_a_negated_one_on_paths():
    data, ends = synth.paths_corpus(n=20_000)
    q = "li nux !Q"  # by the oracle: 628 of the 20 000 paths, the negated pattern drops most of the rest
    asc = O.MultiMatcher(O.parse_query(q), sort="IndexAsc").match_packed(opad(data), ends)
    assert len(asc) > 100
    bias = np.random.default_rng(5).choice([0, 400, -32768, -7, 13], 20_000).astype(np.int16)
    cp = F.Corpus(packed=(data, ends))
    for sort in ("ScoreThenIndexAsc", "ScoreThenIndexDesc", "IndexDesc"):
        mm = F.MultiMatcher(F.parse_query(q), F.Config(sort=F.SortStrategy[sort], pf_lanes=64))
        cp.set_bias(None)
        plain, plain_found = mm.match_list_top_indices(cp, 20_000)  # the unbiased call: its positions, per index, are the reference for the biased one's
        pos = {m.index: m.indices for m in plain}
        assert plain_found == len(asc) and sorted(pos) == asc["index"].tolist()
        cp.set_bias(bias)
        want = biased(asc, bias, sort)
        same(mm.match_list(cp), want, sort)
        same(mm.match_list_parallel(cp, 2), want, sort)
        for limit in (1, 30, len(want) - 1, len(want) + 1):
            assert_top(mm.match_list_top(cp, limit), want, limit, sort)
            recs, found = mm.match_list_top_indices(cp, limit)
            assert found == len(want)
            got = [(m.index, m.score, m.exact, m.indices) for m in recs]
            assert got == [(int(r["index"]), int(r["score"]), bool(r["exact"]), pos[int(r["index"])]) for r in want[:limit]], (sort, limit)


@pytest.mark.parametrize("n_upd", [1, 64, 1000])
def test_update_bias_then_clear(n_upd):
    asc = Fixed.index_asc()
    rng = np.random.default_rng(n_upd)
    cp = Fixed.corpus()
    fm = F.Matcher("deadbe", F.Config(pf_lanes=64, sw_lanes=64))
    model = np.zeros(5000, np.int16)
    # the updates hit matching haystacks too: half of the indices are drawn from the oracle's matches
    idx = np.unique(np.concatenate([rng.choice(asc["index"], min(n_upd, 200), replace=False), rng.integers(0, 5000, n_upd)]))[:n_upd].astype(np.uint32)
    vals = rng.choice([300, -32768, -2, 5], len(idx)).astype(np.int16)
    cp.update_bias(idx, vals)  # creates an all-zero bias first
    model[idx] = vals
    assert np.array_equal(cp.debug_read("bias"), model)
    assert cp.bias_info()["bias_hi"] == max(0, int(vals.max()))
    same(fm.match_list(cp), biased(asc, model, "ScoreThenIndexAsc"), "after update")
    idx2 = idx[: max(1, len(idx) // 2)]
    cp.update_bias(idx2, np.full(len(idx2), 1, np.int16))
    model[idx2] = 1
    assert cp.bias_info()["bias_hi"] == max(1, int(vals.max()))  # never lowered by an update
    assert np.array_equal(cp.debug_read("bias"), model)
    assert_top(fm.match_list_top(cp, 50), biased(asc, model, "ScoreThenIndexAsc"), 50, "after the second update")
    for bad_idx, bad_vals in (([5000], [1]), ([7, 9, 7], [1, 2, 3])):
        with pytest.raises(F.FrizbeeError, match="position"):
            cp.update_bias(bad_idx, bad_vals)
    assert np.array_equal(cp.debug_read("bias"), model)
    with pytest.raises(F.FrizbeeError):
        cp.set_bias(np.zeros(4999, np.int16))
    cp.set_bias(None)
    assert cp.bias_info()["has_bias"] == 0 and cp.bias_info()["bias_hi"] == 0 and len(cp.debug_read("bias")) == 0
    plain = O.Matcher("deadbe").match_packed(opad(Fixed.data), Fixed.ends)
    assert fm.match_list(cp).tobytes() == plain.tobytes()  # the unbiased result, bit for bit
    assert_top(fm.match_list_top(cp, 50), plain, 50, "after clear")


@pytest.mark.parametrize("sort", SORTS)
def test_empty_needle_and_empty_pattern_list(sort):
    """the picker's empty prompt: every haystack, score clamp(bias, 0, 65535), ORDERED per config.sort (a stated departure from the reference)"""
    cp = Fixed.corpus()
    cp.set_bias(Fixed.bias)
    every = np.zeros(5000, F.MATCH_DTYPE)
    every["index"] = np.arange(5000)
    want = biased(every, Fixed.bias, sort)
    assert int(want["score"].max()) == 200 and int((want["score"] == 0).sum()) > 1000
    fc = F.Config(sort=F.SortStrategy[sort], pf_lanes=64)
    for m in (F.Matcher("", fc), F.MultiMatcher([], fc)):
        same(m.match_list(cp), want, (sort, type(m).__name__))
        same(m.match_list_parallel(cp, 2), want, (sort, "parallel"))
        sub = every[1000:4000].copy()
        sub["index"] = sub["index"] - 1000 + 50
        same(m.match_list_into(cp, first=1000, count=3000, index_offset=50), biased(sub, Fixed.bias, "IndexAsc", first=1000, index_offset=50), (sort, "into"))
        for limit in (0, 1, 100, 4999, 5000, 6000):
            assert_top(m.match_list_top(cp, limit), want, limit, (sort, "top"))
            recs, found = m.match_list_top_indices(cp, limit)
            assert found == 5000
            assert [(r.index, r.score, r.exact, r.indices) for r in recs] == [(int(r["index"]), int(r["score"]), False, []) for r in want[:limit]], (sort, limit)


def test_device_forms_return_biased_records():
    import torch

    asc = Fixed.index_asc()
    cp = Fixed.corpus()
    cp.set_bias(Fixed.bias)
    out = torch.zeros(5000 * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    for sort in ("ScoreThenIndexDesc", "IndexAsc"):
        fm = F.Matcher("deadbe", F.Config(sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=64))
        fm.match_list_device(cp, out.data_ptr(), 5000, cnt.data_ptr())
        torch.cuda.synchronize()
        same(out.cpu().numpy()[: int(cnt[0]) * 8].view(F.MATCH_DTYPE), biased(asc, Fixed.bias, "IndexAsc"), "match_list_device")
        fm.match_list_sorted_device(cp, out.data_ptr(), 5000, cnt.data_ptr())
        torch.cuda.synchronize()
        same(out.cpu().numpy()[: int(cnt[0]) * 8].view(F.MATCH_DTYPE), biased(asc, Fixed.bias, sort), "match_list_sorted_device")
        fm.match_list_top_device(cp, 43, out.data_ptr(), 5000, cnt.data_ptr())
        torch.cuda.synchronize()
        assert cnt[:2].tolist() == [43, 255]
        same(out.cpu().numpy()[: 43 * 8].view(F.MATCH_DTYPE), biased(asc, Fixed.bias, sort)[:43], "match_list_top_device")
        mm = F.MultiMatcher(["deadbe"], F.Config(sort=F.SortStrategy[sort], pf_lanes=64))
        mm.match_list_device(cp, out.data_ptr(), 5000, cnt.data_ptr())
        torch.cuda.synchronize()
        same(out.cpu().numpy()[: int(cnt[0]) * 8].view(F.MATCH_DTYPE), biased(asc, Fixed.bias, "IndexAsc"), "multi match_list_device")


def test_refused_forms_say_bias():
    cp = Fixed.corpus()
    cp.set_bias(Fixed.bias)
    mm = F.MultiMatcher(F.parse_query("dead be"), F.Config(pf_lanes=64))
    l = F.lib()
    import ctypes as C

    with pytest.raises(F.FrizbeeError, match="bias") as e:
        mm.match_list_indices(cp)
    assert e.value.code == 1 and "fzb_multi_match_list_top_indices_fused" in str(e.value)
    with pytest.raises(F.FrizbeeError, match="bias"):
        mm.match_list_indices(cp, selection=[1, 2, 3])
    with pytest.raises(F.FrizbeeError, match="bias"):
        list(mm.match_iter_indices(cp))  # fzb_multi_match_list_indices_into
    out, n, pos, found = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_uint64()
    assert l.fzb_multi_match_list_top_indices(mm.h, cp.h, 10, C.byref(out), C.byref(n), C.byref(pos), C.byref(found)) == 1  # the composed host form
    assert b"bias" in l.fzb_last_error() and b"fzb_multi_match_list_top_indices_fused" in l.fzb_last_error()
    from frizbee_amd.distributed import ShardExchange

    with pytest.raises(F.FrizbeeError, match="bias"):
        ShardExchange.check_corpus(cp)
    cp.set_bias(None)
    ShardExchange.check_corpus(cp)
    assert len(mm.match_list_indices(cp)) > 0


def test_rccl_refuses_a_biased_shard_with_one_rank():
    code = r'''
import sys
sys.path[:0] = [%(root)r, %(tests)r, %(tools)r]
import numpy as np
import frizbee_amd as F, synth
from frizbee_amd.distributed import RcclShardComm
data, ends = synth.ragged_corpus(b"deadbeef", 3000, 4, 96, seed=3)
cp = F.Corpus(packed=(data, ends))
comm = RcclShardComm(rank=0, world=1)
ms = [F.Matcher("deadbeef", F.Config(pf_lanes=64)), F.MultiMatcher(F.parse_query("dead be !x"), F.Config(pf_lanes=64)), F.Matcher("", F.Config(pf_lanes=64))]
cp.update_bias([5], [9])
for m in ms:
    try:
        comm.match_list_parallel(m, cp, 3)
        raise SystemExit("a biased shard was accepted")
    except F.FrizbeeError as e:
        assert e.code == 1 and "bias" in str(e), str(e)
cp.set_bias(None)
for m in ms:
    want = m.match_list(cp); want["index"] += 3
    assert comm.match_list_parallel(m, cp, 3).tolist() == want.tolist()
comm.close()
print("BIAS-RCCL-OK")
''' % PATHS
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("FZB_RCCL_LIB", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "BIAS-RCCL-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_requery_loop_allocates_nothing():
    cp = F.Corpus(packed=(Fixed.data[: 4000 * 32], Fixed.ends[:4000]))
    cp.reserve(5000, 5000 * 32)
    cp.set_bias(Fixed.bias[:4000])
    fm = F.Matcher("deadbe", F.Config(pf_lanes=64, sw_lanes=64))
    fm.reserve(cp)
    fm.reserve_top_indices(cp, 100, 8)
    fm.match_list_top_indices(cp, 100)  # (page-locked host buffers are not counted, but take the first call's lazily made ones out of the way)
    asc = Fixed.index_asc()
    asc = asc[asc["index"] < 4000]
    model = Fixed.bias[:4000].copy()
    before = F.device_allocs()
    for step, needle in enumerate(("d", "de", "dea", "dead", "deadb", "deadbe")):
        idx = np.array([step, 100 + 7 * step, 3999 - step], np.uint32)
        vals = np.array([50 + step, -3, 300], np.int16)
        cp.update_bias(idx, vals)
        model[idx] = vals
        fm.set_pattern(needle)
        recs, found = fm.match_list_top_indices(cp, 100)
    assert F.device_allocs() == before
    want = biased(asc, model, "ScoreThenIndexAsc")
    assert found == len(want) and [(m.index, m.score) for m in recs] == [(int(r["index"]), int(r["score"])) for r in want[:100]]
    # appends within the reserved room: the new haystacks start unbiased, nothing is allocated for the bias
    cap = cp.bias_info()["capacity"]
    cp.append(packed=(Fixed.data[4000 * 32:], Fixed.ends[4000:] - Fixed.ends[3999]))
    assert cp.bias_info()["capacity"] == cap and np.array_equal(cp.debug_read("bias"), np.concatenate([model, np.zeros(1000, np.int16)]))
