"""Small-device parity: the library told to behave as on a device of 1, 2 and 5 compute units (FZB_DEBUG_CUS, knobs.h), so that every
grid-stride loop and every per-workgroup run of tiles takes more than one trip on lists of 20 000 haystacks - the trips that otherwise only
lists of millions reach.  Every expected value is the ORACLE's result (with the bias and the reference's ordering rule added in numpy where
a bias is present), plain numpy, or tests/corpus_layout_model.py; never this library's own result at the full compute-unit count.  Records
are integers and must be identical.

Each test ends with its proof of coverage at 1 compute unit: for the kernels it names, work units / (recorded grid x units one workgroup
takes per trip) >= 2, from the grids the library recorded for that very call (fzb_debug_launch_grids), the survivors of last_counters()
and the oracle's matches.  UNITS is the table of DESIGN.md "Small-device parity"; the families that no test here proves are listed there."""
import contextlib
import os
import sys

import numpy as np
import pytest

import frizbee_amd as F
import oracle_lib as O
from sig_host_lib import py_sig_bit
from test_gpu_corpus_append import check_layout
from test_gpu_parity import LANES
from test_gpu_scope import mapped, sub_list, top_indices_tuples, visible
from test_gpu_score_bias import biased, same
from test_gpu_subset import check_subset, device_top, filter_kernel, mask_of, unpack
from test_gpu_topk import SORTS, assert_top, limits_around, opad, single

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
CUS = (1, 2, 5)  # (five is odd: runs and remainders do not line up with tiles)
N = 20 * 1024 + 37  # 21 tiles, a short last one: three rounds of a `cus * 8` filter, runs of six tiles at `cus * 4`
NEEDLE = "deadbe"
PLANTED = b"deaDbe"  # what the ASCII lists hold: the lowercase needle finds it (smart case ignores case), and so does the needle as planted
UNEEDLE = "إنما"
OUTLIERS = 140  # haystacks beyond 256 bytes in the paths list: two trips of the outlier filter's 16 workgroups of four waves

# kernel -> (work unit, units one workgroup takes per trip of its loop).  Work units: n = haystacks of the range (or candidates of an item
# list), surv = survivors of the filter stage (last_counters), match = records (the oracle's), wide = multi-chunk windows (last_counters),
# top = records of a top-`limit` head, gen = windows handed to the wave-per-window kernel, long = haystacks beyond 256 bytes, pairs = (index,
# value) pairs of a column update or indices of a removal
UNITS = {
    # streaming filters and the compactions: a 1024-haystack tile per trip
    "k1_dfa": ("n", 1024), "k1_dfa_sig": ("n", 1024), "k1_filter": ("n", 1024), "k1_cdfa_view": ("n", 1024), "k1_cdfa_ragged": ("n", 1024), "k1_dfa_ragged_burst": ("n", 1024),
    "k1_items": ("n", 1024), "k1_items_dfa": ("n", 1024), "k_literal_filter": ("n", 1024), "k_compact1": ("n", 1024), "k_compact1_classify": ("n", 1024),
    "k2a_window": ("surv", 1024), "k2a_window_pre": ("surv", 256), "k_compact2": ("surv", 1024), "k1_cdfa_outliers": ("long", 4),
    # scorers: a thread per survivor, 128 (256) threads per workgroup
    "k2b_dp_short": ("surv", 128), "k2b_dp": ("surv", 128), "k2u_dp_unicode": ("surv", 128), "k2u_dp_unicode_half": ("surv", 128), "k2u_dp_unicode_half_w2": ("surv", 128), "k2w_classify": ("surv", 512), "k_literal_score": ("surv", 256),
    "k2d_dp_multi_t": ("wide", 128), "k2d_dp_multi": ("wide", 128), "k2d_dp_long_quad": ("surv", 64), "k2d_dp_long": ("surv", 128), "k2u_dp_unicode_multi": ("wide", 128), "k2c_generic": ("gen", 4),
    # ordering, selection, terms, capture: 2048-record tiles or a thread per record
    "k_sort_hist": ("match", 2048), "k_sort_scatter": ("match", 2048), "k_reverse": ("match", 512), "k_topk_hist": ("match", 256), "k_topk_tile_counts": ("match", 2048),
    "k_topk_scatter": ("match", 2048), "k_bias_apply": ("match", 256), "k_scope_flag": ("match", 1024), "k_scope_compact": ("match", 1024), "k_subset_capture": ("match", 256),
    "k_subset_scope_flag": ("n", 1024), "k_top_items": ("top", 256), "k_concat_runs": ("match", 256), "k_ipack_tile_sums": ("top", 2048), "k_ipack_scatter": ("top", 2048),
    # multi-pattern narrowing
    "k_records_to_items": ("match", 256), "k_join_add": ("match", 256), "k_flag_absent": ("match", 1024), "k_compact_records": ("match", 1024), "k_copy_records": ("match", 256), "k_identity_records": ("n", 256),
    # corpus side
    "k_up_measure": ("n", 256), "k_sig_build": ("n", 256), "k_col_scatter": ("pairs", 256), "k_ed_mark": ("pairs", 256), "k_ed_place": ("n", 256),
}


@contextlib.contextmanager
def device_of(cus, **env):
    """the library behaves as on a device of `cus` compute units (and under the other switches given) for the block; matchers and corpora are
    created inside it"""
    env = dict(env, FZB_DEBUG_CUS=str(cus))
    saved = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        F.lib().fzb_debug_reload_knobs()
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        F.lib().fzb_debug_reload_knobs()


def quotients(grids, work):
    return {k: round(work[UNITS[k][0]] / (g[1] * UNITS[k][1]), 2) for k, g in sorted(grids.items()) if k in UNITS and UNITS[k][0] in work}


def prove(cus, grids, work, kernels, ctx):
    """the proof of coverage: each named kernel was launched in the recorded call(s) and its loop took at least two trips"""
    q = quotients(grids, work)
    print("coverage", cus, ctx, work, q, {k: g for k, g in grids.items() if k not in UNITS})
    if cus != 1:  # the shapes are the smallest that give two trips at ONE compute unit
        return
    for spec in kernels:  # "a|b": the forms of one stage - the one that ran
        ran = [k for k in spec.split("|") if k in grids]
        assert ran, (ctx, spec, "not launched", sorted(grids))
        for k in ran:
            assert q[k] >= 2, (ctx, k, q[k], grids[k], work)


# ---- the lists: built once per module, never modified (every test uploads its own Corpus) ----------------------------------------------
class Lists:
    _made, _want = {}, {}

    @classmethod
    def get(cls, name):
        if name not in cls._made:
            cls._made[name] = getattr(cls, "_" + name)()
        return cls._made[name]

    @classmethod
    def want(cls, name, needle, sort="ScoreThenIndexAsc", **cfg):
        """the oracle's records for one query over one list, computed once"""
        key = (name, needle, sort, tuple(sorted(cfg.items())))
        if key not in cls._want:
            cls._want[key] = single(needle, sort=sort, **cfg)[1].match_list(cls.get(name))
        return cls._want[key]

    @staticmethod
    def _uniform32():
        rows, ends = synth.fixed_corpus(PLANTED, N, 32, seed=21, full=0.5)
        return unpack(rows.numpy().reshape(-1), ends)

    @staticmethod
    def _ragged32():
        return unpack(*synth.ragged_corpus(PLANTED, N, 1, 32, seed=22, full=0.65))

    @staticmethod
    def _paths():
        hs = unpack(*synth.ragged_corpus(PLANTED, N, 8, 250, seed=23, full=0.5))
        rng = np.random.default_rng(23)
        for i in rng.choice(N, OUTLIERS, replace=False).tolist():  # beyond 256 bytes: the view's outliers, as many as it admits (n / 256 + 64)
            hs[i] = (hs[i] * 40)[: int(rng.integers(257, 301))]
        return hs

    @staticmethod
    def _utf8():
        return unpack(*synth.utf8_corpus(N, 32, seed=24, needle=UNEEDLE, full=0.5))

    @staticmethod
    def _utf8w():  # unicode windows wider than a chunk
        return [h * 4 for h in Lists.get("utf8")]

    @staticmethod
    def _long():
        return unpack(*synth.ragged_corpus(b"deadbeef" * 10, N, 100, 200, seed=25, full=0.5))


ASCII_QUERIES = [  # (needle, oracle configuration, sort orders)
    (NEEDLE, {}, SORTS),
    (NEEDLE, dict(max_typos=1), ("ScoreThenIndexDesc",)),
    (NEEDLE, dict(max_typos=2), ("IndexDesc",)),
    (NEEDLE, dict(max_typos=None), ("ScoreThenIndexAsc", "IndexAsc")),
    ("deaDbe", dict(casing="Smart"), ("ScoreThenIndexAsc",)),  # an uppercase letter: smart case respects it
    ("xq", dict(max_typos=1), ("ScoreThenIndexAsc",)),         # nearly every haystack survives the filter: the lane-exact window stage at full width
]
QUERIES = {
    "uniform32": ASCII_QUERIES, "ragged32": ASCII_QUERIES, "paths": ASCII_QUERIES,
    "utf8": [(UNEEDLE, {}, SORTS), (UNEEDLE, dict(max_typos=1), ("ScoreThenIndexDesc",)), (UNEEDLE, dict(max_typos=None), ("IndexAsc",))],
}
# what a 0-typo ScoreThenIndexAsc query over each list must have run more than once around (filter, compaction, scorer, the sort's passes)
ZERO_TYPO_KERNELS = {
    "uniform32": ("k1_dfa_sig", "k2b_dp_short", "k_sort_hist", "k_sort_scatter"),
    "ragged32": ("k1_dfa_sig", "k2b_dp_short", "k_sort_hist", "k_sort_scatter"),
    "paths": ("k1_cdfa_view", "k1_cdfa_outliers", "k_compact1", "k2w_classify", "k_sort_hist", "k_sort_scatter"),
    "utf8": ("k1_dfa", "k_compact1", "k2u_dp_unicode|k2u_dp_unicode_half|k2u_dp_unicode_half_w2", "k_sort_hist", "k_sort_scatter"),
}
TYPO_KERNELS = {
    "uniform32": ("k_compact1", "k2b_dp_short"),
    "ragged32": ("k_compact1", "k2b_dp_short"),
    "paths": ("k1_cdfa_view", "k_compact1", "k_compact2", "k2w_classify"),
    "utf8": ("k_compact1",),
}


def run_query(cp, name, needle, cfg, sort, **more):
    fm, _ = single(needle, sort=sort, **cfg)
    F.launch_grids()
    got = fm.match_list(cp)
    grids = F.launch_grids()
    want = Lists.want(name, needle, sort, **cfg)
    same(got, want, (name, needle, cfg, sort))
    c = fm.last_counters()
    return fm, grids, dict(more, n=len(cp), surv=c["filter_survivors"], match=len(want), wide=c["multi_chunk_scored"], gen=c["multi_chunk_scored"])


@pytest.mark.parametrize("which", sorted(QUERIES))
@pytest.mark.parametrize("cus", CUS)
def test_match_list_in_every_sort_order(cus, which):
    hs = Lists.get(which)
    with device_of(cus):
        cp = F.Corpus(hs)
        for needle, cfg, sorts in QUERIES[which]:
            for sort in sorts:
                fm, grids, work = run_query(cp, which, needle, cfg, sort, long=OUTLIERS)
                assert work["match"] > 8192, (which, needle, cfg, work)  # two rounds of the 2048-record tiles at a grid of two
                if not cfg and sort == "ScoreThenIndexAsc":
                    prove(cus, grids, work, ZERO_TYPO_KERNELS[which], (which, needle, "0 typos"))
                elif cfg.get("max_typos") == 1 and needle == NEEDLE:
                    prove(cus, grids, work, TYPO_KERNELS[which], (which, needle, "1 typo"))
                elif needle == "xq":
                    assert which != "paths" or work["surv"] > 16 * 1024 + 512
                    prove(cus, grids, work, ("k2a_window_pre", "k_compact2") if which == "paths" else ("k_compact1",), (which, needle, "1 typo, most survive"))
                else:  # (the *Desc orders reverse the records first)
                    prove(cus, grids, work, ("k_reverse",) if sort.endswith("Desc") else (), (which, needle, cfg, sort))


@pytest.mark.parametrize("which", ("uniform32", "paths", "utf8"))
@pytest.mark.parametrize("cus", CUS)
def test_top_positions_and_the_range_form(cus, which):
    """match_list_top around the cut, match_list_indices, match_list_top_indices, match_list_top_device and the range form with `first` and
    `index_offset`"""
    hs = Lists.get(which)
    needle = UNEEDLE if which == "utf8" else NEEDLE
    with device_of(cus):
        cp = F.Corpus(hs)
        for sort in ("ScoreThenIndexAsc", "IndexDesc"):
            fm, om = single(needle, sort=sort)
            want = Lists.want(which, needle, sort)
            found = len(want)
            for limit in limits_around(found) + [found // 2]:
                assert_top(fm.match_list_top(cp, limit), want, limit, (which, sort))
            F.launch_grids()
            got, words = device_top(fm, cp, found - 3)
            grids = F.launch_grids()
            assert words[:2] == [found - 3, found] and words[2:] == [-1, -1], words
            same(got, want[:found - 3], (which, sort, "device"))
            # (an index order needs no threshold score: the selection is the scatter alone)
            prove(cus, grids, dict(n=N, match=found), ("k_topk_hist", "k_topk_tile_counts", "k_topk_scatter") if sort.startswith("Score") else ("k_topk_scatter",), (which, sort, "top_device"))
            items = om.match_list_indices_ordered(hs)
            assert [(i, s, e) for i, s, e, _ in items] == [(int(r["index"]), int(r["score"]), bool(r["exact"])) for r in want]
            F.launch_grids()
            recs, nfound = fm.match_list_top_indices(cp, found - 3)
            grids = F.launch_grids()
            assert nfound == found and top_indices_tuples(recs) == items[:found - 3], (which, sort)
            # (gen: the traced scorer walks the head)
            prove(cus, grids, dict(match=found, top=found - 3, gen=found - 3), ("k_top_items", "k2c_generic", "k_ipack_tile_sums", "k_ipack_scatter"), (which, sort, "top_indices"))
            assert top_indices_tuples(fm.match_list_indices(cp)) == items, (which, sort, "match_list_indices")
        # the range form: unsorted, input order, index = index_offset + (i - first)
        first, count = 1024 + 511, N - 1024 - 511 - 300
        fm, om = single(needle, sort="IndexAsc")
        rwant = om.match_list(hs[first:first + count])
        rwant["index"] += 1000
        same(fm.match_list_into(cp, first=first, count=count, index_offset=1000), rwant, (which, "range"))


def bias_crossing_256(n, seed):
    return np.random.default_rng(seed).choice([0, 230, 250, -32768, -5, 7], n).astype(np.int16)


@pytest.mark.parametrize("cus", CUS)
def test_scores_on_both_sides_of_256_with_bias_tags_and_scope(cus):
    """both radix passes and both selection levels: a bias that carries scores across 256, under a scope, in every sort order"""
    hs = Lists.get("uniform32")
    rng = np.random.default_rng(41)
    bias = bias_crossing_256(N, 41)
    tags = rng.choice([0, 0, 0, 0, 0, 0, 1, 2, 6], N).astype(np.uint16)  # two thirds stay visible under exclude = 4 | 1
    vis = visible(tags, 0, 5)
    asc_all = Lists.want("uniform32", NEEDLE, "IndexAsc")
    with device_of(cus):
        cp = F.Corpus(hs)
        cp.set_bias(bias)
        for sort in SORTS:
            fm, _ = single(NEEDLE, sort=sort)
            want = biased(asc_all, bias, sort)
            F.launch_grids()
            same(fm.match_list(cp), want, ("bias", sort))
            grids = F.launch_grids()
            assert int((want["score"] >= 256).sum()) > 2048 and int((want["score"] < 256).sum()) > 2048
            by_score = sort.startswith("Score")
            prove(cus, grids, dict(n=N, match=len(want), surv=fm.last_counters()["filter_survivors"]), ("k_bias_apply",) + (("k_sort_hist", "k_sort_scatter") if by_score else ()), ("bias", sort))
            assert not by_score or grids["k_sort_scan"][2] == 2, grids  # both radix passes ran
            above = int((want["score"] >= 256).sum())
            for limit in (above // 2, above + (len(want) - above) // 2):  # a cut above 255 and one below: the high byte's level, then the low byte's
                assert_top(fm.match_list_top(cp, limit), want, limit, ("bias", sort))
        # tags and a scope on top: the terms kernels drop the hidden records before the bias is added
        cp.set_tags(tags)
        cp.set_scope(0, 5)
        asc = mapped(single(NEEDLE, sort="IndexAsc")[1].match_list(sub_list(hs, vis)), vis)
        for sort in SORTS:
            fm, _ = single(NEEDLE, sort=sort)
            want = biased(asc, bias, sort)
            assert len(want) > 4096
            F.launch_grids()
            same(fm.match_list(cp), want, ("scope", sort))
            grids = F.launch_grids()
            prove(cus, grids, dict(n=N, match=len(asc_all)), ("k_scope_flag", "k_scope_compact"), ("scope", sort))
            for limit in (1, len(want) // 2, len(want) + 1):
                assert_top(fm.match_list_top(cp, limit), want, limit, ("scope", sort))


@pytest.mark.parametrize("cus", CUS)
def test_an_80_byte_needle(cus):
    """a needle beyond the by-value arrays over haystacks of 100..200 bytes: scores far beyond 256"""
    hs = Lists.get("long")
    needle = "deadbeef" * 10
    with device_of(cus):
        cp = F.Corpus(hs)
        for sort in ("ScoreThenIndexAsc", "ScoreThenIndexDesc"):
            fm, grids, work = run_query(cp, "long", needle, {}, sort)
            want = Lists.want("long", needle, sort)
            assert len(want) > 8192 and int(want["score"].min()) >= 256
            prove(cus, grids, work, ("k1_dfa_ragged_burst", "k_compact1", "k2d_dp_long_quad", "k_sort_hist", "k_sort_scatter"), ("long", sort))
            for limit in (10, len(want) // 2):
                assert_top(fm.match_list_top(cp, limit), want, limit, ("long", sort))
        # one typo: the lane-exact window kernel in its long-needle form decides every haystack of the range (no streaming automaton)
        fm, grids, work = run_query(cp, "long", needle, dict(max_typos=1), "ScoreThenIndexAsc")
        assert work["surv"] > 8192
        prove(cus, grids, dict(work, surv=len(hs)), ("k2a_window",), ("long", "1 typo, window"))
        prove(cus, grids, work, ("k_compact2", "k2d_dp_long_quad"), ("long", "1 typo"))
        # matched positions: the wave-per-window kernel in its long-needle form walks the head
        fm, om = single(needle)
        items = om.match_list_indices_ordered(hs)[:100]
        F.launch_grids()
        recs, found = fm.match_list_top_indices(cp, 100)
        grids = F.launch_grids()
        assert found == len(Lists.want("long", needle)) and top_indices_tuples(recs) == items
        prove(cus, grids, dict(gen=100, top=100), ("k2c_generic",), ("long", "top_indices"))
    with device_of(cus, FZB_NO_DP_CFM="1"):  # a thread per window instead of four lanes
        cp = F.Corpus(hs)
        fm, grids, work = run_query(cp, "long", needle, {}, "ScoreThenIndexAsc")
        prove(cus, grids, work, ("k1_dfa_ragged_burst", "k_compact1", "k2d_dp_long"), ("long", "FZB_NO_DP_CFM"))


LITERAL = (("Exact", "exact_needle_here"), ("Prefix", "dea"), ("Suffix", "dbe"), ("Substring", "aDb"))


@pytest.mark.parametrize("cus", CUS)
def test_the_four_literal_modes(cus):
    rng = np.random.default_rng(51)
    hs = list(Lists.get("ragged32"))
    for i in np.flatnonzero(rng.random(N) < 0.6).tolist():  # an eighth of the list matches each literal mode
        k = i % 4
        hs[i] = (b"exact_needle_here", b"dea" + hs[i][3:], hs[i][:-3] + b"dbe", hs[i][:4] + b"aDb" + hs[i][7:])[k] if len(hs[i]) >= 8 else hs[i]
    with device_of(cus):
        cp = F.Corpus(hs)
        for mode, needle in LITERAL:
            for sort in ("ScoreThenIndexAsc", "IndexDesc"):
                fm, om = single(needle, sort=sort, matching=mode)
                F.launch_grids()
                got = fm.match_list(cp)
                grids = F.launch_grids()
                want = om.match_list(hs)
                same(got, want, (mode, sort))
                assert len(want) > 2048, (mode, len(want))
                prove(cus, grids, dict(n=N, surv=len(want), match=len(want)), ("k1_dfa" if mode == "Substring" else "k_literal_filter", "k_compact1", "k_literal_score"), (mode, sort))  # (a substring: its automaton in the streaming filter)
                assert_top(fm.match_list_top(cp, len(want) // 2), want, len(want) // 2, (mode, sort))


LONG_LITERAL = ("aab" * 22)[:65]  # periodic, beyond the by-value needle: the literal kernels with the needle's arrays in device memory


def long_literal_list():
    """N ragged haystacks of up to 256 bytes around the 65-byte needle (tests/lit_forms_lib.py: glued prefixes, near-misses, overlapping
    occurrences); three in twenty are made the needle itself, three start with it and three end with it, so that every mode keeps thousands"""
    from lit_forms_lib import make_list
    rng = np.random.default_rng(65)
    nb = LONG_LITERAL.encode()
    hs = make_list("aab*65", "v256", n_rows=N, seed=2)
    for i in np.flatnonzero(rng.random(N) < 0.6).tolist():
        k, body = i % 4, hs[i][: 256 - len(nb)]
        own = nb.upper() if i % 3 == 0 else nb  # (a lowercase needle under smart case: found in either case, scored differently)
        hs[i] = (own, own + body, body + own, hs[i])[k]
    return hs


@pytest.mark.parametrize("cus", CUS)
def test_the_four_literal_modes_over_a_needle_beyond_64_bytes(cus):
    """k_literal_filter / k_literal_score in their long-needle form (NeedleLongDev): more than two trips of both grid-stride loops at one compute unit"""
    if "long_literal" not in Lists._made:
        Lists._made["long_literal"] = long_literal_list()
    hs = Lists.get("long_literal")
    with device_of(cus):
        cp = F.Corpus(hs)
        for mode in ("Exact", "Prefix", "Suffix", "Substring"):
            for sort in ("ScoreThenIndexAsc", "IndexDesc"):
                fm, om = single(LONG_LITERAL, sort=sort, matching=mode)
                F.launch_grids()
                got = fm.match_list(cp)
                grids = F.launch_grids()
                want = Lists.want("long_literal", LONG_LITERAL, sort, matching=mode)
                same(got, want, (mode, sort))
                assert N >= 4097 and len(want) >= 2049, (mode, len(want))
                assert not any(k.startswith("k1_") for k in grids), sorted(grids)  # no streaming automaton for such a needle
                prove(cus, grids, dict(n=N, surv=len(want), match=len(want)), ("k_literal_filter", "k_compact1", "k_literal_score"), ("long needle", mode, sort))
                assert_top(fm.match_list_top(cp, len(want) // 2), want, len(want) // 2, ("long needle", mode, sort))


@pytest.mark.parametrize("cus", CUS)
def test_a_parsed_multi_pattern_query_with_and_and_not(cus):
    hs = Lists.get("uniform32")
    query = "deadbe ea !zqj"
    with device_of(cus):
        cp = F.Corpus(hs)
        for sort in SORTS:
            want = O.MultiMatcher(O.parse_query(query), lanes=LANES[64], sort=sort).match_list(hs)
            assert 4096 < len(want) < len(Lists.want("uniform32", NEEDLE)), len(want)  # (the negated pattern drops some)
            mm = F.MultiMatcher(F.parse_query(query), F.Config(sort=F.SortStrategy[sort], pf_lanes=64, sw_lanes=0))
            F.launch_grids()
            same(mm.match_list(cp), want, (query, sort))
            grids = F.launch_grids()
            prove(cus, grids, dict(n=N, match=len(want)), ("k_records_to_items", "k_join_add", "k_flag_absent", "k_compact_records", "k_copy_records"), (query, sort))
            for limit in (1, len(want) // 2, len(want) + 1):
                assert_top(mm.match_list_top(cp, limit), want, limit, (query, sort))
        # every pattern negated: every haystack starts as a candidate
        want = O.MultiMatcher(O.parse_query("!zqj"), lanes=LANES[64]).match_list(hs)
        mm = F.MultiMatcher(F.parse_query("!zqj"), F.Config(pf_lanes=64, sw_lanes=0))
        F.launch_grids()
        same(mm.match_list(cp), want, "!zqj")
        grids = F.launch_grids()
        assert 8192 < len(want) < N
        prove(cus, grids, dict(n=N, match=len(want)), ("k_identity_records", "k_flag_absent", "k_compact_records"), "!zqj")
        items = O.MultiMatcher(O.parse_query(query), lanes=LANES[64], sort="ScoreThenIndexAsc").match_list_indices_ordered(hs)
        mm = F.MultiMatcher(F.parse_query(query), F.Config(pf_lanes=64, sw_lanes=0))
        recs, found = mm.match_list_top_indices(cp, 5000)
        assert found == len(items) and top_indices_tuples(recs) == items[:5000]


@pytest.mark.parametrize("kernel", ("items", "items_dfa"))
@pytest.mark.parametrize("cus", CUS)
def test_candidate_sets_through_both_item_list_filters(cus, kernel):
    """subset= (17 000 candidates: more than two rounds of either item-list filter), capture=, from_scope and a narrowing chain"""
    for which in ("uniform32", "paths"):
        hs = Lists.get(which)
        rng = np.random.default_rng(61)
        idx = np.flatnonzero(rng.random(N) < 0.85)
        assert len(idx) > 16 * 1024 + 512
        with device_of(cus), filter_kernel(kernel):
            cp = F.Corpus(hs)
            sub, cap = F.Subset(cp), F.Subset(cp)
            found = check_subset(hs, cp, sub, cap, idx, NEEDLE, {}, 64, (which, kernel, cus), ("ScoreThenIndexAsc",))
            assert found > 8192
            fm, _ = single(NEEDLE)
            F.launch_grids()
            fm.match_list(cp, subset=sub, capture=cap)
            grids = F.launch_grids()
            work = dict(n=len(idx), surv=fm.last_counters()["filter_survivors"], match=found)
            prove(cus, grids, work, ("k1_items" if kernel == "items" else "k1_items_dfa", "k_compact1", "k_subset_capture"), (which, kernel))
            # one typo over the candidate set: the lane-exact window kernel re-decides the survivors of the item-list filter
            in_sub = mask_of(idx, N)
            fm1, om1 = single(NEEDLE, max_typos=1)
            want1 = mapped(om1.match_list(sub_list(hs, in_sub)), in_sub)
            F.launch_grids()
            same(fm1.match_list(cp, subset=sub), want1, (which, kernel, "1 typo"))
            grids = F.launch_grids()
            prove(cus, grids, dict(n=len(idx), surv=fm1.last_counters()["filter_survivors"], match=len(want1)), ("k1_items", "k_compact1", "k2a_window", "k_compact2"), (which, kernel, "1 typo"))
            # from_scope: the visible haystacks of a scope the corpus does not have set, as a candidate set
            tags = rng.integers(0, 8, N).astype(np.uint16)
            cp.set_tags(tags)
            F.launch_grids()
            sub.from_scope(0, 4)
            grids = F.launch_grids()
            vis = visible(tags, 0, 4)
            assert np.array_equal(sub.read(), np.flatnonzero(vis).astype(np.uint32))
            prove(cus, grids, dict(n=N), ("k_subset_scope_flag", "k_compact1"), (which, "from_scope"))
            same(fm.match_list(cp, subset=sub), mapped(single(NEEDLE)[1].match_list(sub_list(hs, vis)), vis), (which, kernel, "from_scope"))
            # a narrowing chain: every query over the capture of the one before
            a, b = F.Subset(cp), F.Subset(cp)
            src, dst, prev = None, a, np.ones(N, bool)
            for needle in ("d", "de", "dea", "dead", "deadb", "deadbe"):
                fm.set_pattern(needle)
                om = O.Matcher(needle)
                want = mapped(om.match_list(sub_list(hs, prev)), prev)
                assert_top(fm.match_list_top(cp, 9000, subset=src, capture=dst), want, 9000, (which, kernel, needle))
                got = dst.read()
                assert np.array_equal(got, np.sort(want["index"])), (which, kernel, needle)
                prev = mask_of(got, N)
                src, dst = dst, (b if dst is a else a)
            assert prev.sum() > 8192


KNOB_FORMS = [
    {"FZB_NO_SEG_LIST": "1"}, {"FZB_NO_FUSED_CLASSIFY": "1"}, {"FZB_NO_DP_CLASSES": "1"}, {"FZB_NO_DP_CFM": "1"}, {"FZB_NO_LCS_DFA": "1"}, {"FZB_TYPO_EXACT_WINDOW": "1"},
    {"FZB_COOP_BELOW": "0"}, {"FZB_COOP_BELOW": "100000000"}, {"FZB_UNICODE_MULTI": "0"}, {"FZB_UNICODE_MULTI": "1"}, {"FZB_PARK_LDS_KB": "0"}, {"FZB_NO_CDFA": "1"},
]
# the kernels a form brings in, by (switch, list, max_typos of the query): they too must go around more than once
KNOB_KERNELS = {
    ("FZB_NO_SEG_LIST", "ragged32", 0): ("k1_dfa_sig", "k_compact1", "k2b_dp_short"),
    ("FZB_NO_DP_CLASSES", "paths", 0): ("k2b_dp", "k2d_dp_multi_t"), ("FZB_NO_DP_CLASSES", "paths", 1): ("k2b_dp", "k2d_dp_multi_t"),
    ("FZB_NO_DP_CFM", "paths", 0): ("k2w_classify", "k2d_dp_multi"), ("FZB_NO_DP_CFM", "paths", None): ("k2w_classify", "k2d_dp_multi"),
    ("FZB_NO_LCS_DFA", "ragged32", 1): ("k1_filter", "k_compact1"), ("FZB_NO_LCS_DFA", "paths", 1): ("k1_filter", "k_compact1", "k_compact2"),
    ("FZB_TYPO_EXACT_WINDOW", "ragged32", 1): ("k1_dfa", "k_compact1", "k_compact2"), ("FZB_TYPO_EXACT_WINDOW", "paths", 1): ("k_compact1", "k_compact2"),
    ("FZB_NO_CDFA", "paths", 0): ("k1_dfa_ragged_burst", "k_compact1"), ("FZB_NO_CDFA", "paths", 1): ("k1_dfa_ragged_burst", "k_compact1"),
    ("FZB_UNICODE_MULTI", "utf8w", 0): ("k1_cdfa_ragged", "k_compact1", "k2u_dp_unicode_multi|k2c_generic"),
    ("FZB_UNICODE_MULTI", "utf8w", None): ("k2u_dp_unicode_multi|k2c_generic",),
    ("FZB_UNICODE_MULTI", "utf8w", 1): ("k1_cdfa_ragged", "k_compact1", "k_compact2", "k2u_dp_unicode_multi|k2c_generic"),
    ("FZB_PARK_LDS_KB", "paths", 0): ("k2w_classify",), ("FZB_COOP_BELOW", "paths", 0): ("k2w_classify",), ("FZB_NO_FUSED_CLASSIFY", "paths", 0): ("k_compact1", "k2w_classify"),
}


@pytest.mark.parametrize("env", KNOB_FORMS, ids=[",".join(f"{k}={v}" for k, v in e.items()) for e in KNOB_FORMS])
@pytest.mark.parametrize("cus", CUS)
def test_the_knob_forms_on_a_small_device(cus, env):
    """every other shipping form of a stage, each also with fewer compute units: smaller class queues, and where an overflow path is taken its
    records are still the oracle's"""
    unicode_form = "FZB_UNICODE_MULTI" in env
    with device_of(cus, **env):
        for which in (("utf8w",) if unicode_form else ("ragged32", "paths")):
            if which == "utf8w":
                queries = [(UNEEDLE, {}), (UNEEDLE, dict(max_typos=None)), (UNEEDLE, dict(max_typos=1))]
            else:
                queries = [(NEEDLE, {}), (NEEDLE, dict(max_typos=1)), (NEEDLE, dict(max_typos=None))]
            cp = F.Corpus(Lists.get(which))
            for needle, cfg in queries:
                fm, grids, work = run_query(cp, which, needle, cfg, "ScoreThenIndexAsc")
                assert work["match"] > 8192
                kernels = KNOB_KERNELS.get((list(env)[0], which, cfg.get("max_typos", 0)), ())
                if unicode_form:  # by name: thread per window when forced on, wave per window when forced off
                    kernels = tuple(("k2u_dp_unicode_multi" if env["FZB_UNICODE_MULTI"] == "1" else "k2c_generic") if "|" in k else k for k in kernels)
                prove(cus, grids, work, kernels, (env, which, cfg))


@pytest.mark.parametrize("cus", CUS)
def test_the_fused_compaction_and_classification_where_a_small_device_still_takes_it(cus):
    """k_compact1_classify serves ragged lists of at most two tiles per compute unit, so it has fewer tiles than workgroups by construction:
    run on a small device, with a second round of its classifier's 512-survivor batches only"""
    hs = Lists.get("paths")[: cus * 2048 - 11]
    with device_of(cus):
        cp = F.Corpus(hs)
        for needle, cfg in ((NEEDLE, {}), (NEEDLE, dict(max_typos=None))):
            fm, om = single(needle, **cfg)
            F.launch_grids()
            same(fm.match_list(cp), om.match_list(hs), ("fused", cus, cfg))
            grids = F.launch_grids()
            print("coverage", cus, "fused", cfg, grids)
            assert ("k_compact1_classify" in grids) == (not cfg), grids  # (whole-haystack windows of a query without a filter: k2w_classify)


def np_signatures(rows):
    bits = np.array([0] + [1 << py_sig_bit(b) for b in range(1, 256)], np.uint32)
    return np.bitwise_or.reduce(bits[rows], axis=1)


def model_check(cp, model, ctx):
    assert len(cp) == len(model), ctx
    for name, col, dtype in (("bias", 1, np.int16), ("tags", 2, np.uint16)):
        got, want = cp.debug_read(name), np.array([p[col] for p in model], dtype)
        assert np.array_equal(got, want), (ctx, name, np.flatnonzero(got != want)[:8].tolist() if len(got) == len(want) else (len(got), len(want)))


def model_query(cp, model, ctx):
    """a biased, scoped query against the oracle over the model's visible haystacks, the bias added, every index mapped back"""
    vis = visible([t for _, _, t in model], 0, 4)
    asc = mapped(single(NEEDLE, sort="IndexAsc")[1].match_list([h for (h, _, _), v in zip(model, vis) if v]), vis)
    want = biased(asc, [b for _, b, _ in model], "ScoreThenIndexAsc")
    assert len(want) > 4096, ctx
    fm = single(NEEDLE)[0]
    same(fm.match_list(cp), want, ctx)
    assert_top(fm.match_list_top(cp, len(want) // 2), want, len(want) // 2, ctx)


@pytest.mark.parametrize("which", ("uniform32", "paths"))
@pytest.mark.parametrize("cus", CUS)
def test_the_corpus_side_on_a_small_device(cus, which):
    """upload, view and signatures, then the editing family and both columns, against the Python model and corpus_layout_model.py; every edit
    is followed by a query against the oracle"""
    hs = list(Lists.get(which))
    rng = np.random.default_rng(71)
    with device_of(cus):
        F.launch_grids()
        cp = F.Corpus(hs)
        grids = F.launch_grids()
        info = check_layout(cp, hs)
        if which == "uniform32":
            assert cp.signature_info()[0]
            assert np.array_equal(cp.debug_read("sig"), np_signatures(np.frombuffer(b"".join(hs), np.uint8).reshape(N, 32)))
            prove(cus, grids, dict(n=N), ("k_sig_build",), (which, "upload"))
        else:
            assert info["has_view"] == 1 and info["outliers"] == OUTLIERS
        bias, tags = bias_crossing_256(N, 72), rng.choice([0, 1, 2, 3, 4], N).astype(np.uint16)
        cp.set_bias(bias)
        cp.set_tags(tags)
        cp.set_scope(0, 4)
        model = [(h, int(b), int(t)) for h, b, t in zip(hs, bias.tolist(), tags.tolist())]
        model_check(cp, model, "set")
        model_query(cp, model, (which, "set"))
        # updates of 3000 pairs each: more than two trips of the scatter's grid
        at = rng.choice(len(model), 3000, replace=False)
        nb, nt = rng.integers(-300, 301, 3000), rng.integers(0, 8, 3000)
        F.launch_grids()
        cp.update_bias(at, nb.astype(np.int16))
        cp.update_tags(at, nt.astype(np.uint16))
        grids = F.launch_grids()
        for i, b, t in zip(at.tolist(), nb.tolist(), nt.tolist()):
            model[i] = (model[i][0], int(b), int(t))
        model_check(cp, model, "update")
        prove(cus, grids, dict(pairs=3000), ("k_col_scatter",), (which, "update"))
        model_query(cp, model, (which, "update"))
        # append, then truncate behind the old end
        extra = Lists.get("ragged32" if which == "uniform32" else "paths")[:3 * 1024 + 5]
        cp.append(extra)
        model += [(h, 0, 0) for h in extra]
        model_check(cp, model, "append")
        check_layout(cp, [h for h, _, _ in model])
        model_query(cp, model, (which, "append"))
        model = model[:N + 1500]
        cp.truncate(len(model))
        model_check(cp, model, "truncate")
        check_layout(cp, [h for h, _, _ in model])
        # remove 5000 haystacks from the second tile on: two trips of the mark pass, a suffix of many tiles for the place pass
        gone = 1500 + rng.choice(len(model) - 1500, 5000, replace=False)
        F.launch_grids()
        cp.remove(gone)
        grids = F.launch_grids()
        dropped = set(gone.tolist())
        model = [p for k, p in enumerate(model) if k not in dropped]
        model_check(cp, model, "remove")
        check_layout(cp, [h for h, _, _ in model])
        prove(cus, grids, dict(pairs=5000, n=len(model) - int(gone.min())), ("k_ed_mark", "k_ed_place", "k_up_measure"), (which, "remove"))  # (n: the kept haystacks of the suffix)
        model_query(cp, model, (which, "remove"))
        # replace: same places, other lengths
        idx = np.sort(rng.choice(len(model), 600, replace=False))
        new = [(b"src/" + PLANTED + b"/renamed_to_something_longer/file.cc", b"", PLANTED, b"x" * 31)[k % 4] for k in range(600)]
        cp.replace(idx, new)
        for i, h in zip(idx.tolist(), new):
            model[i] = (h, model[i][1], model[i][2])
        model_check(cp, model, "replace")
        check_layout(cp, [h for h, _, _ in model])
        model_query(cp, model, (which, "replace"))


@pytest.mark.parametrize("cus", CUS)
def test_eight_shards_on_one_gpu(cus):
    """the root's concatenation and sort with a small grid"""
    rows, ends = synth.fixed_corpus(PLANTED, N, 32, seed=21, full=0.5)  # (Lists' uniform32, packed)
    data = rows.numpy().reshape(-1)
    have = F.device_count()
    with device_of(cus):
        sc = F.ShardedCorpus(packed=(data, ends), ndev=8, oversubscribe=8 > have)
        for sort in SORTS:
            fm, _ = single(NEEDLE, sort=sort)
            want = Lists.want("uniform32", NEEDLE, sort)
            F.launch_grids()
            same(fm.match_list_parallel_sharded(sc), want, ("sharded", sort))
            grids = F.launch_grids()
            prove(cus, grids, dict(match=len(want)), ("k_concat_runs",) + (("k_sort_hist", "k_sort_scatter") if sort.startswith("Score") else ()), ("sharded", sort))
            for limit in (10, len(want) // 2):
                assert_top(fm.match_list_top_sharded(sc, limit), want, limit, ("sharded top", sort))
        del sc


# ---- the compaction's later batches: the one case that needs a larger list --------------------------------------------------------------
BIG_TILES = 1025
BIG_N = BIG_TILES * 1024 + 5  # 1026 tiles: runs of 257 tiles at a grid of 4 (a second batch), of 513 at a grid of 2 (three batches)


def big_list():
    """packed 8-byte haystacks.  "deadbe" is planted in the first, the 256th, the 257th and the last tile of every workgroup's run at both
    grids and in NO other tile, so that a wrong prefix or a count carried over from the first batch cannot cancel out; "zyxw" in every
    tenth haystack, everywhere."""
    rng = np.random.default_rng(81)
    rows = rng.choice(np.frombuffer(b"ghijklmnopqrstuv", np.uint8), (BIG_N, 8))
    dense = np.flatnonzero(rng.random(BIG_N) < 0.1)
    rows[dense, :4] = np.frombuffer(b"zyxw", np.uint8)
    ntiles = BIG_TILES + 1
    tiles = set()
    for grid in (4, 2):
        T = -(-ntiles // grid)
        for w in range(grid):
            t0, t1 = min(w * T, ntiles), min(w * T + T, ntiles)
            for b in range(t0, t1, 256):
                tiles |= {b, min(b + 255, t1 - 1)}
            tiles.add(t1 - 1)
    sparse = []
    for t in sorted(tiles):
        lo, hi = t * 1024, min(t * 1024 + 1024, BIG_N)
        at = np.unique(np.concatenate([[lo, hi - 1], rng.integers(lo, hi, 40)]))
        rows[at, :6] = np.frombuffer(b"deadbe", np.uint8)
        rows[at[::3], 2] = ord("X")  # a third of them one substitution away: only the typo query finds these
        sparse.append(at)
    return rows.reshape(-1).copy(), np.arange(1, BIG_N + 1, dtype=np.uint64) * np.uint64(8), sorted(tiles)


def same_records(got, want, ctx):
    if not np.array_equal(got, want):  # (100 000 records: the element-wise report only when they differ)
        same(got, want, ctx)
        raise AssertionError(ctx)


def test_the_compactions_later_batches_at_one_compute_unit():
    data, ends, tiles = big_list()
    odata = opad(data)
    ntiles = BIG_TILES + 1
    wants = {}
    with device_of(1):
        cp = F.Corpus(packed=(data, ends))
        sub = F.Subset(cp)
        sub.set_indices(np.arange(BIG_N))
        for needle, cfg, env in (("deadbe", dict(max_typos=1), {}), ("zyxw", dict(max_typos=1), {}), ("deadbe", {}, {}), ("zyxw", {}, {}),
                                 ("deadbe", {}, {"FZB_NO_SEG_LIST": "1"}), ("zyxw", {}, {"FZB_NO_SEG_LIST": "1"})):
            with device_of(1, **env):
                fm, om = single(needle, **cfg)
                key = (needle, tuple(cfg.items()))
                if key not in wants:
                    wants[key] = om.match_packed(odata, ends)
                want = wants[key]
                assert len(want) > (300 if needle == "deadbe" else 90_000)
                if needle == "deadbe":  # the survivors sit in the planted tiles alone
                    assert sorted(set((want["index"] // 1024).tolist())) == tiles
                F.launch_grids()
                same_records(fm.match_list(cp), want, (needle, cfg, env, "plain"))
                grids = F.launch_grids()
                print("coverage 1 big", needle, cfg, env, grids)
                if cfg or env:  # (the 0-typo query as shipped lets the filter list its survivors: no k_compact1)
                    assert -(-ntiles // grids["k_compact1"][1]) > 256, grids  # a workgroup's run is longer than one 256-tile batch
                # subset = the whole list: the item form of the compaction, half the grid, positions mapped through `src`
                F.launch_grids()
                same_records(fm.match_list(cp, subset=sub), want, (needle, cfg, env, "subset"))
                grids = F.launch_grids()
                print("coverage 1 big subset", needle, cfg, env, grids)
                assert -(-ntiles // grids["k_compact1"][0]) > 512, grids  # three batches


# ---- the record passes' later batches: tile_compact.h's compaction behind k_flag_absent, k_scope_flag and the lane-exact window stage -------
REC_N = 513 * 1024 + 5  # 514 tiles: at one compute unit the record passes' grid is 2, a run of 257 tiles - a second 256-tile batch
REC_ODD = 500           # haystacks that hold nothing of the needles


def record_list():
    """packed 8-byte haystacks over letters that spell neither "zqj" nor "de": all but REC_ODD start with "deadbe" (a tenth of those with
    one substitution, which only the typo query forgives), so that "de" leaves 513 tiles of records and "!zqj" keeps every haystack"""
    rng = np.random.default_rng(91)
    rows = rng.choice(np.frombuffer(b"ghiklmnoprstuv", np.uint8), (REC_N, 8))
    rows[:, :6] = np.frombuffer(b"deadbe", np.uint8)
    rows[rng.random(REC_N) < 0.1, 3] = ord("X")
    odd = rng.choice(REC_N, REC_ODD, replace=False)
    rows[odd] = rng.choice(np.frombuffer(b"ghiklmnoprstuv", np.uint8), (REC_ODD, 8))
    return rows


def packed(rows):
    return rows.reshape(-1).copy(), np.arange(1, len(rows) + 1, dtype=np.uint64) * np.uint64(8)


def tiles_per_workgroup(records, grid):
    return -(-(-(-records // 1024)) // grid)


def test_the_record_compactions_later_batches_at_one_compute_unit():
    import torch

    rows = record_list()
    data, ends = packed(rows)
    odata = opad(data)
    with device_of(1):
        cp = F.Corpus(packed=(data, ends))
        # every pattern negated, every haystack kept: identity records -> k_flag_absent -> k_compact_records over 514 tiles
        want = O.MultiMatcher(O.parse_query("!zqj"), lanes=LANES[64]).match_packed(odata, ends)
        assert len(want) == REC_N
        mm = F.MultiMatcher(F.parse_query("!zqj"), F.Config(pf_lanes=64, sw_lanes=0))
        F.launch_grids()
        same_records(mm.match_list(cp), want, "!zqj")
        grids = F.launch_grids()
        print("coverage 1 records !zqj", grids)
        assert "k_flag_absent" in grids and tiles_per_workgroup(REC_N, grids["k_compact_records"][1]) > 256, grids
        # a negated pattern that removes a part, behind a pattern nearly every haystack matches
        want = O.MultiMatcher(O.parse_query("de !X"), lanes=LANES[64]).match_packed(odata, ends)
        assert 400_000 < len(want) < REC_N - REC_ODD - 40_000
        mm = F.MultiMatcher(F.parse_query("de !X"), F.Config(pf_lanes=64, sw_lanes=0))
        F.launch_grids()
        same_records(mm.match_list(cp), want, "de !X")
        grids = F.launch_grids()
        print("coverage 1 records de !X", grids)
        assert tiles_per_workgroup(REC_N - REC_ODD, grids["k_compact_records"][1]) > 256, grids
        # the 1-typo query over a candidate set that is the whole list: k_compact2's 64-tile batches, five to a run
        sub = F.Subset(cp)
        sub.set_indices(np.arange(REC_N))
        fm, om = single("deadbe", max_typos=1)
        want = om.match_packed(odata, ends)
        assert len(want) == REC_N - REC_ODD
        F.launch_grids()
        same_records(fm.match_list(cp, subset=sub), want, "1 typo")
        grids = F.launch_grids()
        print("coverage 1 records 1 typo", grids, fm.last_counters())
        assert tiles_per_workgroup(fm.last_counters()["filter_survivors"], grids["k_compact2"][1]) > 64, grids
        # tags and a scope that hides every third haystack: k_scope_flag -> k_scope_compact over 513 tiles of records
        vis = np.arange(REC_N) % 3 != 0
        cp.set_tags((~vis).astype(np.uint16))
        cp.set_scope(exclude=1)
        fm, om = single("de", sort="IndexAsc")
        matches = len(om.match_packed(odata, ends))
        assert matches == REC_N - REC_ODD
        vdata, vends = packed(rows[vis])
        want = mapped(om.match_packed(opad(vdata), vends), vis)
        kept = len(want)
        assert kept > 256 * 1024
        F.launch_grids()
        same_records(fm.match_list(cp), want, "scope")
        grids = F.launch_grids()
        print("coverage 1 records scope", grids)
        assert "k_scope_flag" in grids and tiles_per_workgroup(matches, grids["k_scope_compact"][1]) > 256, grids
        # a bounded destination: the first `capacity` kept records and the (written, found) pair
        for capacity in (kept // 2, 1):
            out = torch.full(((capacity + 64) * 8,), 0xEE, dtype=torch.uint8, device="cuda")
            cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
            fm.match_list_device(cp, out.data_ptr(), capacity, cnt.data_ptr())
            torch.cuda.synchronize()
            assert cnt[:2].tolist() == [capacity, kept], (capacity, cnt.tolist())
            host = out.cpu().numpy()
            same_records(host[: capacity * 8].view(F.MATCH_DTYPE), want[:capacity], ("scope", capacity))
            assert (host[capacity * 8:] == 0xEE).all(), "wrote beyond the capacity"


@pytest.mark.parametrize("n", (0, 1, 1023, 1024, 1025))
def test_degenerate_record_counts_into_the_record_compaction(n):
    """no tile, one record, a tile less one, a full tile, a tile and one: a NOT pattern over lists of those lengths"""
    rng = np.random.default_rng(95 + n)
    hs = [bytes(r) for r in rng.choice(np.frombuffer(b"ghiklmnoprstuv", np.uint8), (n, 8))]
    with device_of(1):
        cp = F.Corpus(hs)
        for query in ("!g", "!zqj", "!i !k"):
            want = O.MultiMatcher(O.parse_query(query), lanes=LANES[64]).match_list(hs) if n else np.zeros(0, F.MATCH_DTYPE)
            assert query != "!zqj" or len(want) == n
            mm = F.MultiMatcher(F.parse_query(query), F.Config(pf_lanes=64, sw_lanes=0))
            F.launch_grids()
            same(mm.match_list(cp), want, (n, query))
            grids = F.launch_grids()
            assert not n or ("k_flag_absent" in grids and "k_compact_records" in grids), (n, query, grids)
