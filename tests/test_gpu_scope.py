"""Per-haystack tags and a visibility scope on a resident corpus (fzb_corpus_set_tags / _set_scope).  The contract is one sentence: a query
over a scoped corpus returns what the same query returns over an upload of the visible haystacks alone, in their order, with every index
mapped back to the haystack's index in the full list.  So every expected value here is the ORACLE's result over the visible sub-list plus
the (monotone) index map - with the bias and the reference's ordering rule added in numpy where a bias is present - or plain numpy; never
this library's own unscoped result."""
import ctypes as C
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
from test_gpu_score_bias import Fixed, biased, same, unpack
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


def visible(tags, require, exclude):
    t = np.asarray(tags, np.uint32)
    return ((t & require) == require) & ((t & exclude) == 0)


def random_scope(n, seed):
    """seeded tags over three bits and a scope that requires one and excludes another: about a quarter of the haystacks stay visible"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 8, n).astype(np.uint16), 1, 4


def mapped(recs, vis):
    """records over the visible sub-list -> the same records under the full list's indices"""
    out = recs.copy()
    out["index"] = np.flatnonzero(vis).astype(np.uint32)[recs["index"]]
    return out


def mapped_indices(items, vis):
    at = np.flatnonzero(vis)
    return [(int(at[i]), s, e, ix) for i, s, e, ix in items]


def sub_list(hs, vis):
    return [h for h, v in zip(hs, vis) if v]


def top_indices_tuples(got):
    return [(m.index, m.score, m.exact, m.indices) for m in got]


def check_all_forms(fm, om, om_asc, hs, tags, require, exclude, name):
    """one matcher pair (single or multi) over one list under one scope: match_list, the range form, top at the limits around the cut, top
    with positions"""
    vis = visible(tags, require, exclude)
    sub = sub_list(hs, vis)
    want = mapped(om.match_list(sub), vis) if sub else np.zeros(0, F.MATCH_DTYPE)
    cp = F.Corpus(hs)
    cp.set_tags(tags)
    cp.set_scope(require, exclude)
    same(fm.match_list(cp), want, name)
    # a sub-range with an index_offset: the visible haystacks of the range, index = index_offset + (i - first)
    first, count = len(hs) // 3, len(hs) - len(hs) // 3 - len(hs) // 5
    rvis = np.zeros(len(hs), bool)
    rvis[first:first + count] = vis[first:first + count]
    rsub = sub_list(hs, rvis)
    rwant = mapped(om_asc.match_list(rsub), rvis) if rsub else np.zeros(0, F.MATCH_DTYPE)
    rwant["index"] = rwant["index"] - first + 1000
    same(fm.match_list_into(cp, first=first, count=count, index_offset=1000), rwant, (name, "range"))
    items = mapped_indices(om.match_list_indices_ordered(sub), vis) if sub else []
    assert [(i, s, e) for i, s, e, _ in items] == [(int(r["index"]), int(r["score"]), bool(r["exact"])) for r in want], name
    for limit in limits_around(len(want)):
        assert_top(fm.match_list_top(cp, limit), want, limit, name)
        recs, found = fm.match_list_top_indices(cp, limit)  # (a MultiMatcher's is the fused form)
        assert found == len(want), (name, limit)
        assert top_indices_tuples(recs) == items[:limit], (name, limit)


@pytest.mark.parametrize("sort", SORTS)
def test_reference_known_answers_under_a_random_scope(sort):
    for k, case in enumerate(MT["cases"]):
        hs = _expand(case["haystacks"])
        cfg = dict(case["config"])
        cfg.pop("sort", None)
        fm, om = single(case["needle"], sort=sort, **cfg)
        _, om_asc = single(case["needle"], sort="IndexAsc", **cfg)
        tags, require, exclude = random_scope(len(hs), k)
        check_all_forms(fm, om, om_asc, hs, tags, require, exclude, case["name"])


@pytest.mark.parametrize("sort", SORTS)
def test_multi_pattern_known_answers_under_a_random_scope(sort):
    cases = [(hip_patterns(oracle_pats(c)), oracle_pats(c), c["haystacks"], c["config"], c["name"]) for c in MU["cases"]]
    cases += [(F.parse_query(q), O.parse_query(q), hs, cfg, q) for q, hs, cfg, _, _ in LT["multi_queries"]]
    for k, (fpats, opats, hs, cfg, name) in enumerate(cases):
        cfg = dict(cfg)
        cfg["sort"] = sort
        om = O.MultiMatcher(opats, lanes=LANES[64], **cfg)
        om_asc = O.MultiMatcher(opats, lanes=LANES[64], **dict(cfg, sort="IndexAsc"))
        fc = F.Config(max_typos=cfg.get("max_typos", 0), casing=F.CaseMatching[cfg.get("casing", "Smart")], sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=0)
        mm = F.MultiMatcher(fpats, fc)
        tags, require, exclude = random_scope(len(hs), 100 + k)
        check_all_forms(mm, om, om_asc, hs, tags, require, exclude, name)


# ---- tile edges: short haystacks that all match a one-letter needle, so records = haystacks ---------------------------------------------
SHAPES = (b"a", b"ba", b"xa", b"bxa", b"A", b"aa")


def one_letter_list(n, seed):
    rng = np.random.default_rng(seed)
    return [SHAPES[k] for k in rng.integers(0, len(SHAPES), n)]


def edge_scopes(n, rng):
    """name -> visible mask (tag bit 0 = hidden, the scope excludes it; always ACTIVE)"""
    out = {"nothing_hidden": np.ones(n, bool), "everything_hidden": np.zeros(n, bool), "only_first": np.arange(n) == 0, "only_last": np.arange(n) == n - 1,
           "alternating": np.arange(n) % 2 == 0, "random_half": rng.random(n) < 0.5}
    tile = np.ones(n, bool)
    tile[1024:2048] = False  # one whole tile hidden between visible ones (where the list has one)
    out["a_whole_tile"] = tile
    return out


@pytest.mark.parametrize("n", (1, 64, 65, 1023, 1024, 1025, 2049, 4097))
def test_tile_edges(n):
    rng = np.random.default_rng(n)
    hs = one_letter_list(n, n)
    cp = F.Corpus(hs)
    for sort in ("ScoreThenIndexAsc", "IndexDesc"):
        fm, om = single("a", sort=sort)
        assert len(om.match_list(hs)) == n  # every haystack matches: the drop pass sees n records
        for name, vis in edge_scopes(n, rng).items():
            cp.set_tags((~vis).astype(np.uint16))
            cp.set_scope(exclude=1)
            assert cp.scope_info()["active"] == 1
            sub = sub_list(hs, vis)
            want = mapped(om.match_list(sub), vis) if sub else np.zeros(0, F.MATCH_DTYPE)
            assert len(want) == int(vis.sum())
            same(fm.match_list(cp), want, (n, sort, name))
            for limit in (1, max(1, len(want) // 2), len(want) + 1):
                assert_top(fm.match_list_top(cp, limit), want, limit, (n, sort, name))


def test_large_list_a_workgroup_owns_a_run_of_tiles():
    """600 000 four-byte haystacks that all match: 586 tiles of records, more than the compaction's grid has workgroups"""
    n = 600_000
    rng = np.random.default_rng(6)
    rows = rng.choice(np.frombuffer(b"bcdx", np.uint8), (n, 4))
    rows[np.arange(n), rng.integers(0, 4, n)] = ord("a")
    ends = (np.arange(1, n + 1) * 4).astype(np.uint64)
    tags = rng.integers(0, 4, n).astype(np.uint16)
    tags[300 * 1024:310 * 1024] = 2  # ten whole tiles hidden
    vis = visible(tags, 0, 2)
    cp = F.Corpus(packed=(rows.reshape(-1).copy(), ends))
    cp.set_tags(tags)
    cp.set_scope(0, 2)
    nv = int(vis.sum())
    sub_ends = (np.arange(1, nv + 1) * 4).astype(np.uint64)
    for sort in ("ScoreThenIndexDesc", "IndexAsc"):
        fm, om = single("a", sort=sort)
        want = mapped(om.match_packed(opad(rows[vis].reshape(-1).copy()), sub_ends), vis)
        assert len(want) == nv and 250_000 < nv < 350_000
        same(fm.match_list(cp), want, sort)
        assert_top(fm.match_list_top(cp, 1000), want, 1000, sort)


def test_device_form_with_too_little_room():
    import torch

    n = 3000
    hs = one_letter_list(n, 3)
    vis = np.random.default_rng(3).random(n) < 0.6
    kept = int(vis.sum())
    cp = F.Corpus(hs)
    cp.set_tags((~vis).astype(np.uint16))
    cp.set_scope(exclude=1)
    _, om = single("a", sort="IndexAsc")
    want = mapped(om.match_list(sub_list(hs, vis)), vis)
    assert len(want) == kept
    for m, no_pattern in ((F.Matcher("a", F.Config(sort=F.SortStrategy.IndexAsc, pf_lanes=64, sw_lanes=64)), False), (F.MultiMatcher(["a"], F.Config(pf_lanes=64)), False),
                          (F.MultiMatcher(F.parse_query("a !q"), F.Config(pf_lanes=64)), False), (F.MultiMatcher([], F.Config(pf_lanes=64)), True)):
        exp = want
        if no_pattern:  # every visible haystack, score 0
            exp = np.zeros(kept, F.MATCH_DTYPE)
            exp["index"] = np.flatnonzero(vis)
        for capacity in (kept, kept - 1, 1025, 100, 1):
            out = torch.full(((capacity + 64) * 8,), 0xEE, dtype=torch.uint8, device="cuda")
            cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
            m.match_list_device(cp, out.data_ptr(), capacity, cnt.data_ptr())
            torch.cuda.synchronize()
            assert cnt[:2].tolist() == [capacity, kept], (type(m).__name__, capacity, cnt.tolist())
            host = out.cpu().numpy()
            same(host[: capacity * 8].view(F.MATCH_DTYPE), exp[:capacity], (type(m).__name__, capacity))
            assert (host[capacity * 8:] == 0xEE).all(), "wrote beyond the capacity"


@pytest.mark.parametrize("sort", ["ScoreThenIndexAsc", "ScoreThenIndexDesc"])
def test_scope_and_bias_together_with_ties_at_the_cut(sort):
    rng = np.random.default_rng(8)
    tags = rng.integers(0, 4, 5000).astype(np.uint16)
    vis = visible(tags, 0, 1)
    sub_data = Fixed.data.reshape(5000, 32)[vis].reshape(-1).copy()
    asc = mapped(O.Matcher("deadbe", sort="IndexAsc").match_packed(opad(sub_data), Fixed.ends[: int(vis.sum())]), vis)
    assert 80 < len(asc) < 200
    want = biased(asc, Fixed.bias, sort)
    ties = [k for k in range(1, len(want)) if want[k]["score"] == want[k - 1]["score"]]
    assert len(ties) > 10  # cuts through groups of equal scores exist
    cp = Fixed.corpus()
    cp.set_bias(Fixed.bias)
    cp.set_tags(tags)
    cp.set_scope(exclude=1)
    fm = F.Matcher("deadbe", F.Config(sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=64))
    same(fm.match_list(cp), want, sort)
    same(fm.match_list_parallel(cp, 3), want, sort)
    sub_hs = unpack(sub_data, Fixed.ends[: int(vis.sum())])
    recs, idx = O.Matcher("deadbe", sort="IndexAsc").match_list_indices(sub_hs)
    pos = {int(np.flatnonzero(vis)[int(r["index"])]): ix for r, ix in zip(recs, idx)}
    for limit in (0, 1, ties[0], ties[len(ties) // 2], ties[-1], len(want), len(want) + 5):
        assert_top(fm.match_list_top(cp, limit), want, limit, sort)
        got, found = fm.match_list_top_indices(cp, limit)
        assert found == len(want)
        assert top_indices_tuples(got) == [(int(r["index"]), int(r["score"]), bool(r["exact"]), pos[int(r["index"])]) for r in want[:limit]], (sort, limit)
    mm = F.MultiMatcher(["deadbe"], F.Config(sort=F.SortStrategy[sort], pf_lanes=64))
    same(mm.match_list(cp), want, (sort, "multi"))
    assert_top(mm.match_list_top(cp, ties[0]), want, ties[0], (sort, "multi"))


@pytest.mark.parametrize("sort", SORTS)
@pytest.mark.parametrize("with_bias", [False, True])
def test_empty_needle_and_empty_pattern_list(sort, with_bias):
    """the picker's empty prompt with "hide ignored" switched on: the visible haystacks, score 0 (reversed for *Desc, never sorted) or the
    clamped bias (ordered per config.sort)"""
    rng = np.random.default_rng(12)
    tags = rng.integers(0, 16, 5000).astype(np.uint16)
    vis = visible(tags, 8, 2)
    nv = int(vis.sum())
    assert 500 < nv < 2500
    every = np.zeros(nv, F.MATCH_DTYPE)
    every["index"] = np.flatnonzero(vis)
    cp = Fixed.corpus()
    cp.set_tags(tags)
    cp.set_scope(8, 2)
    if with_bias:
        cp.set_bias(Fixed.bias)
        want = biased(every, Fixed.bias, sort)
    else:
        want = every[::-1].copy() if sort in ("IndexDesc", "ScoreThenIndexDesc") else every
    fc = F.Config(sort=F.SortStrategy[sort], pf_lanes=64)
    for m in (F.Matcher("", fc), F.MultiMatcher([], fc)):
        who = (sort, with_bias, type(m).__name__)
        same(m.match_list(cp), want, who)
        same(m.match_list_parallel(cp, 2), want, who)
        sub = every[(every["index"] >= 1000) & (every["index"] < 4000)].copy()
        sub["index"] = sub["index"] - 1000 + 50
        rwant = biased(sub, Fixed.bias, "IndexAsc", first=1000, index_offset=50) if with_bias else sub
        same(m.match_list_into(cp, first=1000, count=3000, index_offset=50), rwant, (who, "into"))
        for limit in (0, 1, 100, nv - 1, nv, nv + 1, 6000):
            assert_top(m.match_list_top(cp, limit), want, limit, (who, "top"))
            recs, found = m.match_list_top_indices(cp, limit)
            assert found == nv
            assert top_indices_tuples(recs) == [(int(r["index"]), int(r["score"]), False, []) for r in want[:limit]], (who, limit)


def test_cheap_toggles():
    asc_all = Fixed.index_asc()
    plain = O.Matcher("deadbe").match_packed(opad(Fixed.data), Fixed.ends)
    rng = np.random.default_rng(21)
    tags = rng.integers(0, 8, 5000).astype(np.uint16)
    cp = Fixed.corpus()
    cp.set_tags(tags)
    assert cp.scope_info()["active"] == 0 and np.array_equal(cp.debug_read("tags"), tags)
    fm = F.Matcher("deadbe", F.Config(pf_lanes=64, sw_lanes=64))
    mm = F.MultiMatcher(F.parse_query("dead be"), F.Config(pf_lanes=64))
    fm.reserve(cp)
    mm.reserve(cp)
    fm.reserve_top_indices(cp, 100, 8)
    for m in (fm, mm):  # (page-locked host buffers are not counted, but take the first calls' lazily made ones out of the way)
        m.match_list(cp)
        m.match_list_top(cp, 100)
    fm.match_list_top_indices(cp, 100)
    scopes = [(1, 0), (0, 1), (0, 0), (3, 4), (6, 6), (0, 7)]
    before = F.device_allocs()
    got = []
    for require, exclude in scopes:
        cp.set_scope(require, exclude)
        got.append((fm.match_list(cp), fm.match_list_top(cp, 100), fm.match_list_top_indices(cp, 100), mm.match_list(cp), mm.match_list_top(cp, 100)))
    assert F.device_allocs() == before, "toggling the scope on a reserved matcher allocated device memory"
    om = O.MultiMatcher(O.parse_query("dead be"), lanes=LANES[64])
    rows = Fixed.data.reshape(5000, 32)
    for (require, exclude), (full, top, top_idx, mfull, mtop) in zip(scopes, got):
        vis = visible(tags, require, exclude)
        nv = int(vis.sum())
        sub = opad(rows[vis].reshape(-1).copy())
        want = mapped(O.Matcher("deadbe").match_packed(sub, Fixed.ends[:nv]), vis) if nv else np.zeros(0, F.MATCH_DTYPE)
        same(full, want, (require, exclude))
        assert_top(top, want, 100, (require, exclude))
        assert top_idx[1] == len(want) and [(m.index, m.score) for m in top_idx[0]] == [(int(r["index"]), int(r["score"])) for r in want[:100]]
        mwant = mapped(om.match_packed(sub, Fixed.ends[:nv]), vis) if nv else np.zeros(0, F.MATCH_DTYPE)
        same(mfull, mwant, (require, exclude, "multi"))
        assert_top(mtop, mwant, 100, (require, exclude, "multi"))
    assert len(got[4][0]) == 0  # a bit in both masks hides everything
    # set_pattern keeps the tags and the scope
    cp.set_scope(1, 0)
    fm.set_pattern("dead")
    vis = visible(tags, 1, 0)
    nv = int(vis.sum())
    same(fm.match_list(cp), mapped(O.Matcher("dead").match_packed(opad(rows[vis].reshape(-1).copy()), Fixed.ends[:nv]), vis), "after set_pattern")
    fm.set_pattern("deadbe")
    # scope (0, 0) and clear_tags: the unscoped oracle result, bit for bit
    cp.set_scope(0, 0)
    assert fm.match_list(cp).tobytes() == plain.tobytes()
    cp.set_scope(1, 0)
    cp.clear_tags()
    info = cp.scope_info()
    assert info["active"] == 0 and info["scope"] == 0 and info["capacity"] >= 5000 and not cp.debug_read("tags").any()
    assert fm.match_list(cp).tobytes() == plain.tobytes()
    assert len(plain) == len(asc_all)
    # update_tags on a corpus without tags creates an all-zero array first; bad updates name the position and change nothing
    cp2 = Fixed.corpus()
    assert len(cp2.debug_read("tags")) == 0 and cp2.scope_info()["capacity"] == 0
    hit = asc_all["index"][:7].astype(np.uint32)
    cp2.update_tags(hit, np.full(7, 0x8000, np.uint16))
    model = np.zeros(5000, np.uint16)
    model[hit] = 0x8000
    assert np.array_equal(cp2.debug_read("tags"), model)
    for bad_idx, bad_vals in (([5000], [1]), ([7, 9, 7], [1, 2, 3])):
        with pytest.raises(F.FrizbeeError, match="position"):
            cp2.update_tags(bad_idx, bad_vals)
    with pytest.raises(F.FrizbeeError):
        cp2.set_tags(np.zeros(4999, np.uint16))
    assert np.array_equal(cp2.debug_read("tags"), model)
    cp2.set_scope(require=0x8000)
    got7 = fm.match_list(cp2)
    assert sorted(got7["index"].tolist()) == sorted(hit.tolist())
    # a scope on a corpus without tags: an all-zero array is created, (require != 0) hides everything
    cp3 = Fixed.corpus()
    cp3.set_scope(require=1)
    assert cp3.scope_info()["active"] == 1 and cp3.scope_info()["capacity"] >= 5000 and len(fm.match_list(cp3)) == 0
    assert fm.match_list_top(cp3, 10)[1] == 0


def test_refused_forms_say_scope():
    cp = Fixed.corpus()
    cp.update_tags([1], [1])
    cp.set_scope(exclude=1)
    fm = F.Matcher("deadbe", F.Config(pf_lanes=64, sw_lanes=64))
    mm = F.MultiMatcher(F.parse_query("dead be"), F.Config(pf_lanes=64))
    l = F.lib()
    with pytest.raises(F.FrizbeeError, match="scope") as e:
        fm.match_list_indices(cp)
    assert e.value.code == 1 and "fzb_match_list_top_indices" in str(e.value)
    with pytest.raises(F.FrizbeeError, match="scope"):
        fm.match_list_indices(cp, selection=[1, 2, 3])
    with pytest.raises(F.FrizbeeError, match="scope"):
        list(fm.match_iter_indices(cp))  # fzb_match_list_indices_into
    with pytest.raises(F.FrizbeeError, match="scope") as e:
        mm.match_list_indices(cp)
    assert e.value.code == 1 and "fzb_multi_match_list_top_indices_fused" in str(e.value)
    with pytest.raises(F.FrizbeeError, match="scope"):
        list(mm.match_iter_indices(cp))  # fzb_multi_match_list_indices_into
    out, n, pos, found = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_uint64()
    assert l.fzb_multi_match_list_top_indices(mm.h, cp.h, 10, C.byref(out), C.byref(n), C.byref(pos), C.byref(found)) == 1  # the composed host form
    assert b"scope" in l.fzb_last_error() and b"fzb_multi_match_list_top_indices_fused" in l.fzb_last_error()
    from frizbee_amd.distributed import ShardExchange

    with pytest.raises(F.FrizbeeError, match="scope"):
        ShardExchange.check_corpus(cp)
    cp.set_scope(0, 0)
    ShardExchange.check_corpus(cp)
    assert len(fm.match_list_indices(cp)) > 0 and len(mm.match_list_indices(cp)) > 0


def test_rccl_refuses_a_scoped_shard_with_one_rank():
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
cp.update_tags([5], [9])
cp.set_scope(exclude=1)
for m in ms:
    try:
        comm.match_list_parallel(m, cp, 3)
        raise SystemExit("a scoped shard was accepted")
    except F.FrizbeeError as e:
        assert e.code == 1 and "scope" in str(e), str(e)
cp.set_scope(0, 0)
for m in ms:
    want = m.match_list(cp); want["index"] += 3
    assert comm.match_list_parallel(m, cp, 3).tolist() == want.tolist()
comm.close()
print("SCOPE-RCCL-OK")
''' % PATHS
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("FZB_RCCL_LIB", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "SCOPE-RCCL-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
