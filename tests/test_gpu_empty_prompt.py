"""The empty prompt on the device: `Matcher("")` over a corpus with a score bias, an active scope or a candidate set (kernels_prompt.hip,
prompt_records.h; the two new entry points fzb_prompt_list_device / fzb_prompt_top_device).  Every expected value comes from the numpy model
`prompt` below - the rule of include/frizbee_hip.h: the haystacks of the range, or of the subset, visible under the scope, in index order,
score clamp(bias, 0, 65535) or 0, exact 0; reversed for the *Desc strategies; sorted stably by descending score for the Score* strategies
only when the corpus is biased; found = the number visible - never from the library."""
import contextlib
import os

import numpy as np
import pytest
import torch  # (ahead of the library, as in the modules that import tools/synth.py: one HIP runtime per process, torch's)

import frizbee_amd as F

pytestmark = pytest.mark.gpu

SORTS = ("ScoreThenIndexAsc", "ScoreThenIndexDesc", "IndexAsc", "IndexDesc")
LENGTHS = (1, 64, 65, 1023, 1024, 1025, 2049, 5000)  # word and tile edges of tile_compact.h, and the bias tests' 5000
TERMS = ("bias", "scope", "bias+scope", "subset", "subset+bias+scope")
SCOPE = (8, 2)


def prompt(n, bias=None, tags=None, scope=(0, 0), items=None, sort="IndexAsc", first=0, count=None, index_offset=0):
    """the model: MATCH_DTYPE records of the empty prompt over a list of n haystacks"""
    local = np.arange(n - first if count is None else count, dtype=np.int64) if items is None else np.asarray(items, np.int64)
    h = first + local
    keep = np.ones(len(local), bool)
    if tags is not None and scope != (0, 0):
        t = np.asarray(tags, np.uint32)[h]
        keep = ((t & scope[0]) == scope[0]) & ((t & scope[1]) == 0)
    w = np.zeros(int(keep.sum()), F.MATCH_DTYPE)
    w["index"] = index_offset + local[keep]
    if bias is not None:
        w["score"] = np.clip(np.asarray(bias, np.int64)[h[keep]], 0, 65535)
    if sort in ("IndexDesc", "ScoreThenIndexDesc"):
        w = w[::-1]
    if bias is not None and sort in ("ScoreThenIndexAsc", "ScoreThenIndexDesc"):
        w = w[np.argsort(-w["score"].astype(np.int64), kind="stable")]
    return np.ascontiguousarray(w)


def same(got, want, ctx=""):
    if got.tolist() != want.tolist():
        k = min(len(got), len(want))
        bad = [(i, got[i].tolist(), want[i].tolist()) for i in range(k) if got[i].tolist() != want[i].tolist()][:5]
        raise AssertionError(f"{ctx}: len {len(got)} vs {len(want)}; first diffs (at, got, want) {bad}")


def assert_top(got, want, limit, ctx=""):
    recs, found = got
    assert found == len(want), (ctx, limit, found, len(want))
    same(recs, want[:limit], (ctx, "limit", limit))


def tuples(recs):
    return [(r.index, r.score, r.exact, r.indices) for r in recs]


def haystacks(n, seed=0):
    """what the haystacks hold does not matter to an empty needle; their number does"""
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(97, 123, int(k)).astype(np.uint8)) for k in rng.integers(1, 33, n)]


BIASES = {  # straddling 256: the single radix pass, two passes, and the clamp's two ends
    "max40": lambda rng, n: rng.integers(-40, 41, n),
    "max300": lambda rng, n: rng.choice([-50, 0, 3, 255, 256, 300], n),
    "extremes": lambda rng, n: rng.choice([0, 200, -32768, -5, 7, 32767], n),
}


def bias_of(kind, n, seed):
    b = np.asarray(BIASES[kind](np.random.default_rng(seed), n)).astype(np.int16)
    b[n // 2] = {"max40": 40, "max300": 300, "extremes": 32767}[kind]  # the maximum is present at every length
    return b


class Lists:
    _hs = {}

    @classmethod
    def get(cls, n):
        if n not in cls._hs:
            cls._hs[n] = haystacks(n, n)
        return cls._hs[n]


def forms(fm, cp, n, sort, bias, tags, scope, items, sub, ctx):
    """every host form against the model"""
    want = prompt(n, bias, tags, scope, items, sort)
    kw = {} if sub is None else dict(subset=sub)
    same(fm.match_list(cp, **kw), want, (ctx, "match_list"))
    if sub is None:
        same(fm.match_list_parallel(cp, 2), want, (ctx, "parallel"))
        first, count = (1000, 3000) if n == 5000 else (n // 4, n // 2)
        same(fm.match_list_into(cp, first=first, count=count, index_offset=50), prompt(n, bias, tags, scope, None, "IndexAsc", first, count, 50), (ctx, "into"))
    found = len(want)
    for limit in sorted({x for x in (0, 1, 7, found - 1, found, found + 1) if x >= 0}):
        assert_top(fm.match_list_top(cp, limit, **kw), want, limit, (ctx, "top"))
        recs, f = fm.match_list_top_indices(cp, limit, **kw)
        assert f == found, (ctx, limit)
        assert tuples(recs) == [(int(r["index"]), int(r["score"]), False, []) for r in want[:limit]], (ctx, "top_indices", limit)


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("n", LENGTHS)
def test_parity_over_the_forms(n, terms):
    rng = np.random.default_rng(1000 + n)
    cp = F.Corpus(Lists.get(n))
    tags = rng.integers(0, 16, n).astype(np.uint16)
    items = np.flatnonzero(rng.random(n) < 0.3).astype(np.uint32)
    sub = None
    if "subset" in terms:
        sub = F.Subset(cp)
        sub.set_indices(items)
    scoped = "scope" in terms
    if scoped:
        cp.set_tags(tags)
        cp.set_scope(*SCOPE)
    for kind in (BIASES if "bias" in terms else (None,)):
        bias = None
        if kind:
            bias = bias_of(kind, n, n)
            cp.set_bias(bias)
            if n == 5000:
                assert int((np.clip(bias, 0, None) == 0).sum()) >= 1000  # ties: the stable order and its reversal
        for sort in SORTS:
            fm = F.Matcher("", F.Config(sort=F.SortStrategy[sort], pf_lanes=64))
            forms(fm, cp, n, sort, bias, tags if scoped else None, SCOPE if scoped else (0, 0), items if sub is not None else None, sub, (n, terms, kind, sort))


def test_edges():
    n = 2049
    cp, other = F.Corpus(Lists.get(n)), F.Corpus(Lists.get(n))
    rng = np.random.default_rng(4)
    bias = bias_of("max300", n, 4)
    tags = rng.integers(0, 4, n).astype(np.uint16)
    cp.set_bias(bias)
    cp.set_tags(tags)
    fm = F.Matcher("", F.Config(pf_lanes=64))
    sort = "ScoreThenIndexAsc"
    cp.set_scope(4, 4)  # hides everything
    recs, found = fm.match_list_top(cp, 10)
    assert found == 0 and len(recs) == 0 and len(fm.match_list(cp)) == 0
    cp.set_scope(0, 8)  # a scope that hides nothing
    same(fm.match_list(cp), prompt(n, bias, sort=sort), "hides nothing")
    assert_top(fm.match_list_top(cp, 7), prompt(n, bias, sort=sort), 7, "hides nothing")
    cp.set_scope(1, 0)
    sub, cap = F.Subset(cp), F.Subset(cp)
    sub.set_indices([])  # an empty subset
    assert len(fm.match_list(cp, subset=sub)) == 0
    recs, found = fm.match_list_top(cp, 5, subset=sub)
    assert found == 0 and len(recs) == 0
    sub.set_indices(np.arange(n))  # a full one
    same(fm.match_list(cp, subset=sub), prompt(n, bias, tags, (1, 0), sort=sort), "full subset")
    # capture= : `in` itself, or the whole list
    items = np.flatnonzero(rng.random(n) < 0.5).astype(np.uint32)
    sub.set_indices(items)
    want = prompt(n, bias, tags, (1, 0), items, sort)
    same(fm.match_list(cp, subset=sub, capture=cap), want, "capture of in")
    assert np.array_equal(cap.read(), items)
    assert_top(fm.match_list_top(cp, 9, capture=cap), prompt(n, bias, tags, (1, 0), sort=sort), 9, "capture of all")
    assert np.array_equal(cap.read(), np.arange(n))
    # a subset filled by a _device capture: its count is unknown on the host
    out = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    cp.set_scope(0, 0)
    cp.set_bias(None)
    F.Matcher("e", F.Config(pf_lanes=64)).match_list_top_device(cp, 3, out.data_ptr(), n, cnt.data_ptr(), capture=cap)
    cp.set_bias(bias)
    cp.set_scope(1, 0)
    got = fm.match_list_top(cp, 11, subset=cap)  # (queried while the count is still unknown)
    has_e = np.array([i for i, h in enumerate(Lists.get(n)) if b"e" in h], np.uint32)
    assert 100 < len(has_e) < n
    assert_top(got, prompt(n, bias, tags, (1, 0), has_e, sort), 11, "device capture")
    same(fm.match_list(cp, subset=cap), prompt(n, bias, tags, (1, 0), has_e, sort), "device capture, list")
    # stale and foreign subsets
    foreign = F.Subset(other)
    foreign.set_indices([1, 2])
    with pytest.raises(F.FrizbeeError, match="stale") as e:
        fm.match_list_top(cp, 3, subset=foreign)
    assert e.value.code == 1
    cp.append([b"one more"])
    for call in (lambda: fm.match_list(cp, subset=sub), lambda: fm.match_list_top(cp, 3, subset=sub), lambda: fm.match_list_top_indices(cp, 3, subset=sub),
                 lambda: fm.prompt_top_device(cp, 3, out.data_ptr(), n, cnt.data_ptr(), subset=sub)):
        with pytest.raises(F.FrizbeeError, match="stale") as e:
            call()
        assert e.value.code == 1


def device_records(out, k):
    return out.cpu().numpy()[: k * 8].view(F.MATCH_DTYPE)


def test_new_device_forms():
    n = 5000
    rng = np.random.default_rng(9)
    cp = F.Corpus(Lists.get(n))
    bias = bias_of("max300", n, 9)
    tags = rng.integers(0, 16, n).astype(np.uint16)
    items = np.flatnonzero(rng.random(n) < 0.3).astype(np.uint32)
    sub = F.Subset(cp)
    sub.set_indices(items)
    out = torch.zeros((n + 8) * 8, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    for step, (b, t, scope) in enumerate(((None, None, (0, 0)), (bias, None, (0, 0)), (None, tags, SCOPE), (bias, tags, SCOPE))):
        cp.set_bias(b)
        if t is not None:
            cp.set_tags(t)
        cp.set_scope(*scope)
        for sort in SORTS:
            fm = F.Matcher("", F.Config(sort=F.SortStrategy[sort], pf_lanes=64))
            for s, it in ((None, None), (sub, items)):
                st = stream.cuda_stream if step % 2 else 0
                want = prompt(n, b, t, scope, it, "IndexAsc")
                out.zero_()
                torch.cuda.synchronize()
                fm.prompt_list_device(cp, out.data_ptr(), n, cnt.data_ptr(), st, subset=s)
                torch.cuda.synchronize()
                assert cnt[:2].tolist() == [len(want), len(want)], (step, sort, "list")
                same(device_records(out, len(want)), want, (step, sort, "prompt_list_device"))
                assert not out.cpu().numpy()[len(want) * 8:].any(), "wrote beyond the records"
                cut = len(want) // 3  # too little room: the prefix, and the full count
                fm.prompt_list_device(cp, out.data_ptr(), cut, cnt.data_ptr(), subset=s)
                torch.cuda.synchronize()
                assert cnt[:2].tolist() == [cut, len(want)]
                same(device_records(out, cut), want[:cut], (step, sort, "cut list"))
                want = prompt(n, b, t, scope, it, sort)
                for limit in (0, 43, len(want) + 1):
                    fm.prompt_top_device(cp, limit, out.data_ptr(), n, cnt.data_ptr(), st, subset=s)
                    torch.cuda.synchronize()
                    k = min(limit, len(want))
                    assert cnt[:2].tolist() == [k, len(want)], (step, sort, limit)
                    same(device_records(out, k), want[:limit], (step, sort, "prompt_top_device", limit))
            if sort == "IndexAsc":  # a range, numbered from an offset
                want = prompt(n, b, t, scope, None, "IndexAsc", 1000, 3000, 50)
                fm.prompt_list_device(cp, out.data_ptr(), n, cnt.data_ptr(), first=1000, count=3000, index_offset=50)
                torch.cuda.synchronize()
                assert cnt[:2].tolist() == [len(want), len(want)]
                same(device_records(out, len(want)), want, (step, "range"))
    fm = F.Matcher("", F.Config(pf_lanes=64))
    # too small a capacity: refused, nothing launched, the count words untouched
    cnt.fill_(77)
    torch.cuda.synchronize()
    with pytest.raises(F.FrizbeeError) as e:
        fm.prompt_top_device(cp, 100, out.data_ptr(), 99, cnt.data_ptr())
    assert e.value.code == 5  # FZB_ERR_CAPACITY
    torch.cuda.synchronize()
    assert cnt.tolist() == [77] * 4
    # a subset is queried over the whole corpus only
    with pytest.raises(F.FrizbeeError, match="whole corpus") as e:
        fm.prompt_list_device(cp, out.data_ptr(), n, cnt.data_ptr(), subset=sub, first=1, count=10)
    assert e.value.code == 1
    # an empty corpus zeroes the pair
    empty = F.Corpus([])
    for call in (lambda: fm.prompt_top_device(empty, 5, out.data_ptr(), n, cnt.data_ptr()), lambda: fm.prompt_list_device(empty, out.data_ptr(), n, cnt.data_ptr())):
        cnt.fill_(77)
        call()
        torch.cuda.synchronize()
        assert cnt.tolist() == [0, 0, 77, 77]
    # a matcher with a needle is refused, and the message names the needle
    with_needle = F.Matcher("abc", F.Config(pf_lanes=64))
    for call in (lambda: with_needle.prompt_top_device(cp, 5, out.data_ptr(), n, cnt.data_ptr()), lambda: with_needle.prompt_list_device(cp, out.data_ptr(), n, cnt.data_ptr())):
        with pytest.raises(F.FrizbeeError, match="needle") as e:
            call()
        assert e.value.code == 1
    # the old _device forms still refuse an empty needle
    for call in (lambda: fm.match_list_top_device(cp, 5, out.data_ptr(), n, cnt.data_ptr()), lambda: fm.match_list_top_device(cp, 5, out.data_ptr(), n, cnt.data_ptr(), subset=sub),
                 lambda: fm.match_list_device(cp, out.data_ptr(), n, cnt.data_ptr())):
        with pytest.raises(F.FrizbeeError, match="empty needle") as e:
            call()
        assert e.value.code == 1


@contextlib.contextmanager
def device_of(cus):
    """the library behaves as on a device of `cus` compute units for the block (tests/test_gpu_small_device.py)"""
    saved = os.environ.get("FZB_DEBUG_CUS")
    try:
        os.environ["FZB_DEBUG_CUS"] = str(cus)
        F.lib().fzb_debug_reload_knobs()
        yield
    finally:
        if saved is None:
            os.environ.pop("FZB_DEBUG_CUS", None)
        else:
            os.environ["FZB_DEBUG_CUS"] = saved
        F.lib().fzb_debug_reload_knobs()


def test_it_runs_on_the_device_and_its_loops_take_more_than_one_trip():
    n = 5000
    rng = np.random.default_rng(2)
    bias = bias_of("max300", n, 2)
    tags = rng.integers(0, 16, n).astype(np.uint16)

    def run():
        cp = F.Corpus(Lists.get(n))
        cp.set_bias(bias)
        fm = F.Matcher("", F.Config(pf_lanes=64))
        F.launch_grids()
        plain = fm.match_list_top(cp, 100)
        g1 = F.launch_grids()
        cp.set_tags(tags)
        cp.set_scope(*SCOPE)
        scoped = fm.match_list_top(cp, 100)
        g2 = F.launch_grids()
        return plain, scoped, g1, g2

    with device_of(1):
        plain, scoped, g1, g2 = run()
    assert "k_prompt_records" in g1 and "k_prompt_flag" not in g1, sorted(g1)
    assert "k_prompt_flag" in g2 and "k_prompt_compact" in g2 and "k_prompt_records" not in g2, sorted(g2)
    assert "k_identity_records" not in g1 and "k_bias_apply" not in g1 and "k_bias_apply" not in g2
    print("grids", g1["k_prompt_records"], g2["k_prompt_flag"], g2["k_prompt_compact"])
    assert n / (g1["k_prompt_records"][1] * 256) >= 2  # trips per thread of the grid-stride loop
    tiles = (n + 1023) // 1024
    assert tiles / g2["k_prompt_flag"][1] >= 2 and tiles / g2["k_prompt_compact"][1] >= 2  # tiles per workgroup
    assert_top(plain, prompt(n, bias, sort="ScoreThenIndexAsc"), 100, "one compute unit")
    assert_top(scoped, prompt(n, bias, tags, SCOPE, sort="ScoreThenIndexAsc"), 100, "one compute unit, scoped")
    plain0, scoped0, g1, g2 = run()  # without the switch: the same results, nothing recorded
    assert g1 == {} and g2 == {}
    same(plain0[0], plain[0])
    same(scoped0[0], scoped[0])
    assert plain0[1] == plain[1] and scoped0[1] == scoped[1]


def test_no_allocation_after_reserve():
    n = 5000
    rng = np.random.default_rng(6)
    cp = F.Corpus(Lists.get(n))
    cp.set_bias(bias_of("max40", n, 6))
    cp.set_tags(rng.integers(0, 16, n).astype(np.uint16))
    sub = F.Subset(cp)
    sub.from_scope(1, 0)
    fm = F.Matcher("", F.Config(pf_lanes=64))
    fm.reserve(cp)
    cp.update_bias([0], [1])  # (the corpus' own staging of the pairs is made by its first update)
    before = F.device_allocs()
    for k in range(3):
        fm.match_list_top(cp, 100)
        fm.match_list(cp)
        cp.update_bias([k, 100 + k], [300 + k, -7])  # (past 255: the ordering takes both radix passes from here on)
        cp.set_scope(*SCOPE)
        fm.match_list_top(cp, 100)
        fm.match_list_top_indices(cp, 10)
        fm.match_list_top(cp, 100, subset=sub)
        fm.match_list(cp)
        fm.match_list_into(cp, first=10, count=1000, index_offset=3)
        cp.set_scope(0, 0)
    assert F.device_allocs() == before


def test_after_edits():
    n = 3000
    rng = np.random.default_rng(8)
    hs = list(Lists.get(5000)[:n])
    bias = bias_of("max300", n, 8).astype(np.int64)
    tags = rng.integers(0, 16, n).astype(np.int64)
    cp = F.Corpus(hs)
    cp.set_bias(bias.astype(np.int16))
    cp.set_tags(tags.astype(np.uint16))
    cp.set_scope(*SCOPE)
    fm = F.Matcher("", F.Config(sort=F.SortStrategy.ScoreThenIndexDesc, pf_lanes=64))

    def check(ctx):
        assert len(cp) == len(bias) == len(tags)
        want = prompt(len(bias), bias, tags, SCOPE, sort="ScoreThenIndexDesc")
        same(fm.match_list(cp), want, ctx)
        assert_top(fm.match_list_top(cp, 50), want, 50, ctx)

    check("before")
    cp.append(haystacks(1500, 77))  # new haystacks: bias 0, tag 0
    bias, tags = np.concatenate([bias, np.zeros(1500, np.int64)]), np.concatenate([tags, np.zeros(1500, np.int64)])
    cp.update_bias([n + 5], [123])
    bias[n + 5] = 123
    check("append")
    gone = rng.choice(len(bias), 700, replace=False)
    cp.remove(gone)
    bias, tags = np.delete(bias, gone), np.delete(tags, gone)
    check("remove")
    cp.replace([3, 1500, 2047], [b"a", b"bb", b"ccc"])  # a renamed path keeps its bias and tags
    check("replace")
    cp.truncate(1025)
    bias, tags = bias[:1025], tags[:1025]
    check("truncate")
