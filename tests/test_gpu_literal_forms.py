"""Literal modes with periodic needles through every filter and scorer form, record for record against the oracle.

A Substring needle on the ASCII path runs as its Knuth-Morris-Pratt automaton in the streaming filter kernels that were written for automata
which never step back (k1_dfa, k1_cdfa_view, k1_cdfa_outliers, k1_cdfa_ragged, k1_dfa_ragged_burst); an item list (a candidate set, a later
pattern of a MultiMatcher), the unicode path, the anchored modes and needles beyond 63 bytes take k_literal_filter's first-byte scan instead;
k_literal_score / lit_find then report the best-scoring occurrence, the earliest on ties.  The needles here have borders (tests/lit_forms_lib.py),
so the automaton restarts from deep states and most accepted rows hold several occurrences; occurrences end on and straddle byte 4, 16, 32,
128, 256 and the row's last byte.  Before the device is asked, each list is checked on the second transcription of the reference
(tests/lit_second_transcription.py) and on the oracle alone: 10 % .. 80 % of the rows accepted, a quarter of those with two or more
occurrences, in 5 % of those the reported occurrence is not the first.

Which kernel serves a case is read back from the launch record (F.launch_grids; FZB_DEBUG_CUS set to the device's own compute-unit count
records without changing a grid).  The record holds a kernel's name, not its template arguments; which instantiation a name stands for
follows from fzb_launch_filter's conditions and is chosen here by construction:
  k1_cdfa_view, 1024 threads, no lengths:  a needle without a NUL byte on a list of fewer tiles than two per compute unit (the device's own count)
  k1_cdfa_view, 256 threads, no lengths:   the same under FZB_DEBUG_CUS=1 (four tiles >= two per compute unit)
  k1_cdfa_view, sanitising, with lengths:  the needle that holds a NUL byte
  NV = 8 / 16:  the v128 / v256 shapes;  G = 4 / 2:  the needle of 14 byte classes has G = 2, asserted through fzb_debug_cdfa_state.
The tie rule of lit_find (`>` - the earliest of the best-scoring occurrences) is what test_positions_say_which_occurrence_was_chosen sees
directly: positions of every accepted row, under a scoring of pairwise different bonuses and under the default."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import frizbee_amd as F
import oracle_lib as O
from lit_forms_lib import CASINGS, N_ROWS, NEEDLES, SCORINGS, conditions_hold, make_list, statistics
from test_gpu_topk import assert_top, single

pytestmark = pytest.mark.gpu
NAMES = list(NEEDLES)


def own_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def form(cus=None, **env):
    """the switches of one filter form for the block, the launches recorded (at the device's own compute-unit count unless `cus` says otherwise)"""
    env = dict(env, FZB_DEBUG_CUS=str(cus or own_cus()))
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


_pairs = {}


def pair(name, shape):
    """the list of one (needle, shape) pair - made once, its conditions checked on the transcription and the oracle before any device call"""
    if (name, shape) not in _pairs:
        hs = make_list(name, shape)
        assert len(hs) == N_ROWS and max(map(len, hs)) == (700 if shape == "out" else int(shape[1:])) and min(map(len, hs)) == 0
        stats, rows = statistics(name, hs)
        share = (round(stats[0] / len(hs), 3), round(stats[1] / stats[0], 3), round(stats[2] / max(stats[1], 1), 3))
        print("list", repr(name), shape, "accepted / several occurrences / not the first:", share)
        assert conditions_hold(stats, len(hs)), (name, shape, stats)
        recs, idx = O.Matcher(NEEDLES[name][0], matching="Substring", sort="IndexAsc").match_list_indices(hs)
        assert [(int(r["index"]), int(r["score"]), bool(r["exact"]), ix) for r, ix in zip(recs, idx)] == [(i,) + r for i, r in enumerate(rows) if r is not None]
        _pairs[name, shape] = hs
    return _pairs[name, shape]


_wants = {}


def want_of(name, shape, sort, casing, sname, matching="Substring"):
    key = (name, shape, sort, casing, sname, matching)
    if key not in _wants:
        _wants[key] = O.Matcher(NEEDLES[name][0], matching=matching, sort=sort, casing=casing, scoring=SCORINGS[sname]).match_list(pair(name, shape))
    return _wants[key]


def hip(name, sort, casing, sname, matching="Substring"):
    return single(NEEDLES[name][0], sort=sort, casing=casing, scoring=SCORINGS[sname], matching=matching)[0]


def width_of(name):
    """the composition width the library built for the needle's Substring automaton (0: no composite table), None where there is no automaton"""
    needle = NEEDLES[name][0]
    if not needle.isascii() or len(needle) > 63:
        return None
    kg = (C.c_int32 * 2)()
    m = F.Matcher(needle, F.Config(matching=F.Matching.Substring))
    return kg[1] if F.lib().fzb_debug_cdfa_state(m.h, b"", 0, kg) >= 0 else 0


def filter_forms(name, shape):
    """[(switches, the filter kernels that must have run)] for a Substring query over one (needle, shape) pair"""
    g = width_of(name)
    assert g == NEEDLES[name][2], (name, g)
    if g is None:  # the unicode path, a needle in device memory: the first-byte scan
        return [({}, ("k_literal_filter",))]
    if shape == "s32":
        return [({}, ("k1_dfa",))]
    burst = (dict(FZB_NO_CDFA="1"), ("k1_dfa_ragged_burst",))
    if g == 0:
        return [({}, ("k1_dfa_ragged_burst",)), burst]
    view = ("k1_cdfa_view", "k1_cdfa_outliers") if shape == "out" else ("k1_cdfa_view",)
    return [({}, view), (dict(cus=1), view), (dict(FZB_FILTER_VIEW="0"), ("k1_cdfa_ragged",)), burst]


def same(got, want, ctx):
    if got.tolist() != want.tolist():
        n = min(len(got), len(want))
        bad = [i for i in range(n) if got[i].tolist() != want[i].tolist()][:5]
        raise AssertionError(f"{ctx}: {len(got)} records, the oracle has {len(want)}; first differences {[(got[i].tolist(), want[i].tolist()) for i in bad]}")


@pytest.mark.parametrize("name", NAMES)
def test_match_list_through_every_filter_form(name):
    served = {}
    for shape in NEEDLES[name][1]:
        hs = pair(name, shape)
        for env, kernels in filter_forms(name, shape):
            with form(**env):
                cp = F.Corpus(hs)
                if "k1_cdfa_view" in kernels:
                    assert cp.build_view(), "the list has no filter view"
                for k, (casing, sname) in enumerate((c, s) for c in CASINGS for s in SCORINGS):
                    for sort in ("ScoreThenIndexAsc", "IndexDesc") if not env else (("ScoreThenIndexAsc", "IndexDesc")[k % 2],):
                        want = want_of(name, shape, sort, casing, sname)
                        F.launch_grids()
                        got = hip(name, sort, casing, sname).match_list(cp)
                        grids = F.launch_grids()
                        same(got, want, (name, shape, env, casing, sname, sort))
                        assert all(kn in grids for kn in kernels + ("k_compact1", "k_literal_score")), (name, shape, env, sorted(grids))
                        assert sum(kn.startswith(("k1_", "k_literal_filter")) for kn in grids) == len(kernels), (name, shape, env, sorted(grids))
                        served[shape, tuple(sorted(env.items()))] = {kn: grids[kn][:2] for kn in kernels + ("k_literal_score",)}
    print("served", repr(name), served)


@pytest.mark.parametrize("name", NAMES)
def test_positions_say_which_occurrence_was_chosen(name):
    """match_list_indices over every accepted row: the positions are the chosen occurrence's, so a wrong tie rule or a wrong best cannot hide
    behind an equal score; and the top-`limit` forms of both entry points"""
    for shape in NEEDLES[name][1]:
        hs = pair(name, shape)
        with form():
            cp = F.Corpus(hs)
            for k, (casing, sname) in enumerate((c, s) for c in CASINGS for s in SCORINGS):
                sort = ("ScoreThenIndexAsc", "IndexAsc", "ScoreThenIndexDesc")[k % 3]
                fm, om = single(NEEDLES[name][0], sort=sort, casing=casing, scoring=SCORINGS[sname], matching="Substring")
                items = om.match_list_indices_ordered(hs)
                got = [(m.index, m.score, m.exact, m.indices) for m in fm.match_list_indices(cp)]
                assert got == items, (name, shape, casing, sname, sort, next((a, b) for a, b in zip(got + [None], items + [None]) if a != b))
                want = want_of(name, shape, sort, casing, sname)
                assert [t[:3] for t in items] == [(int(r["index"]), int(r["score"]), bool(r["exact"])) for r in want]
                if casing == "Smart":
                    for limit in (1, 37, len(want) // 2, len(want) + 5):
                        assert_top(fm.match_list_top(cp, limit), want, limit, (name, shape, sname, sort))
                        recs, found = fm.match_list_top_indices(cp, limit)
                        assert found == len(want) and [(m.index, m.score, m.exact, m.indices) for m in recs] == items[:limit], (name, shape, sname, sort, limit)


@pytest.mark.parametrize("name", NAMES)
def test_item_lists_anchored_modes_and_later_patterns(name):
    """the second accept implementation (lit_accepts: a first-byte scan over aligned 16-byte vectors) against the oracle on the same lists: a
    candidate set's item list - the identity set and a sparse one -, the anchored modes over the range, a later pattern of a MultiMatcher"""
    needle = NEEDLES[name][0]
    shape = NEEDLES[name][1][len(name) % len(NEEDLES[name][1])]
    hs = pair(name, shape)
    rng = np.random.default_rng(len(hs) + len(needle))
    sets = {"identity": np.arange(len(hs)), "sparse": np.flatnonzero(rng.random(len(hs)) < 0.3)}
    with form():
        cp = F.Corpus(hs)
        sub = F.Subset(cp)
        for casing in CASINGS:
            want = want_of(name, shape, "IndexAsc", casing, "distinct")
            fm = hip(name, "IndexAsc", casing, "distinct")
            whole = fm.match_list(cp)
            same(whole, want, (name, shape, casing, "range"))
            for label, idx in sets.items():
                sub.set_indices(idx)
                F.launch_grids()
                got = fm.match_list(cp, subset=sub)
                grids = F.launch_grids()
                same(got, want[np.isin(want["index"], idx)], (name, shape, casing, label))
                same(got, whole[np.isin(whole["index"], idx)], (name, shape, casing, label, "the range form's records"))
                assert "k_literal_filter" in grids and "k_literal_score" in grids and not any(kn.startswith("k1_") for kn in grids), (name, label, sorted(grids))
            for mode in ("Exact", "Prefix", "Suffix"):
                want = want_of(name, shape, "ScoreThenIndexAsc", casing, "distinct", matching=mode)
                F.launch_grids()
                got = hip(name, "ScoreThenIndexAsc", casing, "distinct", matching=mode).match_list(cp)
                grids = F.launch_grids()
                same(got, want, (name, shape, casing, mode))
                assert len(want) > 0 and "k_literal_filter" in grids and "k_literal_score" in grids, (name, mode, len(want), sorted(grids))
        # a later positive Substring pattern, and a negated one, behind a fuzzy pattern that keeps most rows which hold the needle's first letter
        first = needle[0].lower()
        for negated in (False, True):
            fq = [F.Pattern(first), F.Pattern(needle, negated=negated, matching=F.Matching.Substring)]
            oq = [O.P(first), O.P(needle, negated=negated, matching="Substring")]
            want = O.MultiMatcher(oq).match_list(hs)
            F.launch_grids()
            got = F.MultiMatcher(fq, F.Config(pf_lanes=64)).match_list(cp)
            grids = F.launch_grids()
            same(got, want, (name, shape, "multi", negated))
            assert 0 < len(want) < len(hs) and "k_literal_filter" in grids, (name, negated, len(want), sorted(grids))
