"""Records against the oracle on BOTH sides of every form gate (tests/form_gates.py: the gate's expression exactly T - 1 and exactly T, one
point of prefix bonus apart), on lists that hold the windows built to push the operands up (tests/form_gate_lists.py).  Only a GPU run sees
v_pk_maximum3_f16 (p_max3_s, dp_body.h) on operands next to 0x7C00; tests/test_form_gates_host.py measures the same scorings on the CPU.

Which form ran: every query runs inside device_of(4) and the launch record names the scorers - k2b_dp_short / k2w_classify (or the fused
k_compact1_classify) / k2_classes_all / k2d_dp_multi_t / k2d_dp_long_quad inside a gate, k2b_dp / k2d_dp_multi / k2d_dp_long outside.
bias_ok and cfu_ok are template flags of kernels that keep their names: there the side taken is what form_gates.py says and nothing else shows it.

The ordering gate (fzb_order_flags: score ceiling + exact_match_bonus < 256) is crossed at 255 / 256 with lists whose best score IS the bound;
the side shows in k_sort_scan's launches (one radix pass against two) and k_topk_hist's (one histogram level against two)."""
import numpy as np
import pytest

import form_gate_lists as L
import form_gates as G
import frizbee_amd as F
import oracle_lib as O
from test_gpu_fuzz_isa import make_unicode_list
from test_gpu_scope import top_indices_tuples, visible
from test_gpu_small_device import device_of
from test_gpu_topk import SORTS, assert_top

pytestmark = pytest.mark.gpu
CUS = 4
FAST = ("k2b_dp_short", "k2w_classify", "k_compact1_classify", "k2_classes_all", "k2b_dp_class")
ROWS = {"cf": 13, "cfm": 13, "bias": 13, "cfu": 13}


def pair(needle, sc, pf, sort="ScoreThenIndexAsc", max_typos=0):
    om = O.Matcher(needle, lanes=L.LANES[pf], scoring=list(sc), sort=sort, max_typos=max_typos)
    oi = om.info()
    fc = F.Config(max_typos=max_typos, sort=F.SortStrategy[sort], scoring=F.Scoring(*sc), pf_lanes=oi["pf_lanes"], sw_lanes=oi["sw_lanes"])
    return F.Matcher(needle, fc), om, oi["sw_lanes"]


def same(got, want, ctx):
    if got.tolist() != want.tolist():
        n = min(len(got), len(want))
        bad = next((i for i in range(n) if got[i].tolist() != want[i].tolist()), n)
        raise AssertionError((ctx, "records", len(got), len(want), "first difference at", bad, got[bad:bad + 2].tolist(), want[bad:bad + 2].tolist()))


def check_names(gate, kind, inside, grids, ctx):
    """the scorer's name on the gate's side (pf_lanes 64, 0 typos)"""
    names = set(grids)
    if gate == "cf":
        assert ("k2b_dp" in names) == (not inside) and bool(names & set(FAST)) == inside, (ctx, sorted(names))
    elif gate == "cfm" and kind == "ragged":
        assert ("k2d_dp_multi" in names) == (not inside) and bool(names & {"k2d_dp_multi_t", "k2_classes_all"}) == inside, (ctx, sorted(names))
    elif gate == "cfm_long":
        assert ("k2d_dp_long_quad" in names) == inside and ("k2d_dp_long" in names) == (not inside), (ctx, sorted(names))


def run_side(gate, needle, sc, inside, kinds, lanes, typos, positions=True):
    """one scoring over the lists of `kinds`: records at every lane triple and typo budget, the form's name, matched positions"""
    rows = len(needle)
    assert L.oracle_accepts(needle, sc)
    assert G.gate(gate, sc, rows, pad_ok=0 not in needle) == inside
    with device_of(CUS):
        for pf in lanes:
            sw = O.Matcher(needle, lanes=L.LANES[pf], scoring=list(sc)).info()["sw_lanes"]
            for kind in kinds:
                if kind == "short" and sw // 2 < rows:  # (16-lane chunks: no haystack of half a chunk holds the needle, and no short-haystack scorer exists there)
                    continue
                hs = L.gate_list(kind, needle, sw, seed=rows * 100 + pf)
                cp = F.Corpus(hs)
                for k in typos:
                    if k is not None and k >= rows:
                        continue
                    fm, om, _ = pair(needle, sc, pf, max_typos=k)
                    want = om.match_list(hs)
                    assert len(want) > 200, (gate, kind, pf, k, len(want))
                    F.launch_grids()
                    got = fm.match_list(cp)
                    grids = F.launch_grids()
                    ctx = (gate, "inside" if inside else "outside", sc, needle, kind, pf, k)
                    same(got, want, ctx)
                    print("form", ctx, "matches", len(want), "scorers", sorted(g for g in grids if g.startswith(("k2", "k_compact1_classify"))))
                    if pf == 64 and k == 0:
                        check_names(gate, kind, inside, grids, ctx)
                if positions and pf == lanes[0]:
                    fm, om, _ = pair(needle, sc, pf)
                    items = om.match_list_indices_ordered(hs)
                    assert top_indices_tuples(fm.match_list_indices(cp)) == items, (gate, sc, kind, "match_list_indices")
                    recs, found = fm.match_list_top_indices(cp, len(items) // 2)
                    assert found == len(items) and top_indices_tuples(recs) == items[: len(items) // 2], (gate, sc, kind, "match_list_top_indices")


SHORT_GATES = [(g, fam) for g in ("cf", "cfm", "bias", "cfu") for fam in G.FAMILIES]


@pytest.mark.parametrize("gate,family", SHORT_GATES, ids=["%s-%s" % c for c in SHORT_GATES])
def test_records_on_both_sides_of_a_short_needles_gate(gate, family):
    """bias / cfu: no kernel name tells the sides apart (template flags of k2b_dp, k2d_dp_multi, the unicode scorers); the side is form_gates.py's"""
    needle = L.capital_needle(ROWS[gate])
    inside, outside = G.gate_scorings(gate, len(needle), family)
    for sc, side in ((inside, True), (outside, False)):
        run_side(gate, needle, sc, side, ("short", "ragged"), (64, 32), (0, 1, None))
    run_side(gate, needle, inside, True, ("ragged",), (16,), (0,), positions=False)  # one pass at 16 lanes (no short-haystack scorer there)


@pytest.mark.parametrize("rows", (65, 130))
@pytest.mark.parametrize("family", G.FAMILIES)
def test_records_on_both_sides_of_the_long_needles_gate(family, rows):
    needle = L.capital_needle(rows)
    inside, outside = G.gate_scorings("cfm_long", rows, family)
    for sc, side in ((inside, True), (outside, False)):
        run_side("cfm_long", needle, sc, side, ("long",), (64, 32), (0, 1, None))


@pytest.mark.parametrize("gate", ("cf", "cfm", "cfm_long"))
def test_the_gap_clause_at_its_edge(gate):
    """2 * gap_extend == mismatch_penalty (inside) and == mismatch_penalty + 1 (outside), the bound far away"""
    needle = L.capital_needle(65 if gate == "cfm_long" else 13)
    inside, outside = G.clause_scorings(gate, len(needle))
    for sc, side in ((inside, True), (outside, False)):
        run_side(gate, needle, sc, side, ("long",) if gate == "cfm_long" else ("short", "ragged"), (64, 32), (0, None), positions=False)


@pytest.mark.parametrize("family", G.FAMILIES)
def test_a_nul_byte_in_the_needle_closes_cf_ok_on_its_last_scoring(family):
    """pad_ok: the T - 1 scoring of cf_ok with a needle that holds a NUL byte - dp_cf.h's closed-form padding does not apply, k2b_dp scores"""
    needle = b"ABCDEF\0GHIJKL"
    inside, _ = G.gate_scorings("cf", len(needle), family)
    run_side("cf", needle, inside, False, ("short", "ragged"), (64, 32), (0, 1, None), positions=False)


@pytest.mark.parametrize("gate", ("cf", "cfm"))
def test_the_dense_bonus_needle_on_both_sides_of_the_gate_as_it_stands_now(gate):
    """named case (form_gates.dense_bonus_case): the scoring that sat inside the gate while it stood on the reference's amortised bound - operands
    beyond 0x7C00 into v_pk_maximum3_f16 - is outside now, and the gate's present last scoring is inside"""
    needle, before, now = G.dense_bonus_case(gate)
    run_side(gate, needle, before, False, ("ragged",), (64, 32), (0, None))
    run_side(gate, needle, now, True, ("ragged",), (64, 32), (0, None))


@pytest.mark.parametrize("gate,family", [(g, f) for g in ("bias", "cfu") for f in G.FAMILIES])
def test_unicode_needles_on_both_sides_of_bias_ok_and_cfu_ok(gate, family):
    """the unicode scorers exist only under bias_ok (pipe_score_unicode) and take dp_unicode.h's biased-throughout form under cfu_ok: template
    flags again, so the side is form_gates.py's.  Multi-chunk windows: up to 90 scalars a haystack."""
    rng = np.random.default_rng(77)
    with device_of(CUS):
        for needle in ("éa", "إنما"):
            rows = len(needle)
            data, ends = make_unicode_list(rng, needle, 1500, 90)
            cp = F.Corpus(packed=(data, ends))
            for sc, side in zip(G.gate_scorings(gate, rows, family), (True, False)):
                assert G.gate(gate, sc, rows) == side
                for pf in (64, 32):
                    for k in (0, None):
                        om = O.Matcher(needle, lanes=L.LANES[pf], scoring=list(sc), max_typos=k)
                        oi = om.info()
                        fm = F.Matcher(needle, F.Config(max_typos=k, scoring=F.Scoring(*sc), pf_lanes=oi["pf_lanes"], sw_lanes=oi["sw_lanes"]))
                        want = om.match_packed(data, ends)
                        assert len(want) > 200
                        same(fm.match_list(cp), want, (gate, family, needle, sc, pf, k))


# ---- the ordering gate ---------------------------------------------------------------------------------------------------------------------------
def ordering_cases():
    out = []
    for rows in (1, 6, 12):
        for bound in (255, 256):
            out.append(("bound-%d-rows-%d" % (bound, rows), G.bound_scoring(rows, bound), rows))
    for rows in (11, 12, 13):  # the default scoring's own edge: ceiling + exact = 240 at 11 rows, 260 at 12
        out.append(("default-rows-%d" % rows, G.DEFAULT, rows))
    return out


@pytest.mark.parametrize("name,sc,rows", ordering_cases(), ids=[c[0] for c in ordering_cases()])
def test_the_ordering_gate_at_its_bound(name, sc, rows):
    one_pass = G.one_pass(sc, rows)
    bound = G.expression("one_pass", sc, rows)
    best, needle, best_hay = L.best_score_search(sc, rows)
    hs = L.ordering_list(needle, best_hay, seed=rows)
    tags = (np.arange(len(hs)) % 3).astype(np.uint16)
    want = {sort: O.Matcher(needle, scoring=list(sc), sort=sort).match_list(hs) for sort in SORTS}
    w = want["ScoreThenIndexAsc"]
    scores = w["score"].astype(np.int64)
    found = len(w)
    top = int(scores[0])
    n_top = int((scores == top).sum())
    second = int(scores[scores < top].max())
    n_second = int((scores == second).sum())
    # from the oracle's records alone: two trips of the 2048-record tiles, the best score the search found, long tie groups, both sides of 256
    assert found > 2 * 2048 and top == best and n_top > 100 and n_second > 100, (name, found, top, best, n_top, n_second)
    if name.startswith("bound"):
        assert top == bound
    if bound >= 256 and name.startswith("bound"):
        assert top >= 256 and int((scores < 256).sum()) > 100
    print("ordering", name, sc, needle, "found", found, "top", top, n_top, "second", second, n_second, "one_pass", one_pass)
    sections = [(1, 0), (0, 1)]
    with device_of(CUS):
        cp = F.Corpus(hs)
        cp.set_tags(tags)
        for sort in SORTS:
            fm = F.Matcher(needle, F.Config(sort=F.SortStrategy[sort], scoring=F.Scoring(*sc), pf_lanes=64, sw_lanes=0))
            F.launch_grids()
            same(fm.match_list(cp), want[sort], (name, sort))
            grids = F.launch_grids()
            if sort.startswith("Score"):
                assert grids["k_sort_scan"][2] == (1 if one_pass else 2), (name, sort, grids["k_sort_scan"])
            for limit in (n_top // 2, n_top + n_second // 2, found):
                F.launch_grids()
                assert_top(fm.match_list_top(cp, limit), want[sort], limit, (name, sort))
                grids = F.launch_grids()
                if sort.startswith("Score") and limit < found:
                    assert grids["k_topk_hist"][2] == (1 if one_pass else 2), (name, sort, limit, grids["k_topk_hist"])
            got = fm.match_list_top_sections(cp, sections, 1024)
            for (req, exc), (recs, nfound) in zip(sections, got):
                ws = want[sort][visible(tags, req, exc)[want[sort]["index"]]]
                assert nfound == len(ws), (name, sort, req, exc, nfound, len(ws))
                same(recs, ws[:1024], (name, sort, "section", req, exc))
        data, ends = O.pack(hs)
        shc = F.ShardedCorpus(packed=(data[:-64].copy(), ends), ndev=8, oversubscribe=8 > F.device_count())
        for sort in ("ScoreThenIndexAsc", "ScoreThenIndexDesc"):
            fm = F.Matcher(needle, F.Config(sort=F.SortStrategy[sort], scoring=F.Scoring(*sc), pf_lanes=64, sw_lanes=0))
            for limit in (n_top // 2, n_top + n_second // 2):
                assert_top(fm.match_list_top_sharded(shc, limit), want[sort], limit, (name, sort, "sharded"))
        del shc
