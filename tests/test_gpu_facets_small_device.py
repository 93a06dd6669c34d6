"""Small-device parity of the tag facets: the library told to behave as on a device of 1, 2 and 5 compute units (FZB_DEBUG_CUS) on the
21-tile list of tests/test_gpu_facets.py, so that the grid-stride loop of every new kernel and instantiation - the record form
(k_facets_records), the form fused into the scope's flag pass (k_scope_flag_facets) and the column form (k_facets_column) - takes more than
one trip.  Results are the oracle's match set plus numpy over the tags; the proof of the trips is from the grids the library recorded for
that very call: work units / (recorded grid x the 1024 items one workgroup takes per trip) >= 2 at one compute unit."""
import numpy as np
import pytest

import frizbee_amd as F
from facets_model import facet_words
from test_gpu_facets import N, NEEDLE, Data, check, device_list, not_vacuous
from test_gpu_small_device import CUS, device_of
from test_gpu_topk import single

pytestmark = pytest.mark.gpu
WIDE = "g"  # a needle most haystacks of the list match: more records than two trips of a grid of two take
TILE = 1024


def prove_trips(cus, grids, kernel, units, ctx):
    """the kernel was launched in the recorded call, and at one compute unit its loop took at least two trips"""
    assert kernel in grids, (ctx, kernel, "not launched", sorted(grids))
    q = units / (grids[kernel][1] * TILE)
    print("coverage", cus, ctx, kernel, grids[kernel], units, round(q, 2))
    if cus == 1:
        assert q >= 2, (ctx, kernel, q, grids[kernel], units)


@pytest.mark.parametrize("cus", CUS)
def test_the_three_forms_on_a_small_device(cus):
    d = Data.get()
    hs, tags = d["hs"], d["tags"]
    a = Data.matches(NEEDLE)
    wide = Data.matches(WIDE)
    not_vacuous(a, tags, N)
    not_vacuous(wide, tags, N)
    assert len(wide) > 4 * TILE  # two trips of a grid of two workgroups
    with device_of(cus):
        cp = F.Corpus(hs)
        cp.set_tags(tags)
        sink = F.Facets(cp)
        for needle, aset in ((NEEDLE, a), (WIDE, wide)):
            fm, _ = single(needle)
            fm.set_facets(sink)
            # no active scope: the record form, once over the producer's records
            cp.set_scope(0, 0)
            want = facet_words(tags[aset])
            F.launch_grids()
            recs, found = fm.match_list_top(cp, 50)
            grids = F.launch_grids()
            check(sink, want, (cus, needle, "records"), found=found)
            assert "k_scope_flag_facets" not in grids and "k_facets_column" not in grids, grids
            if needle == WIDE:
                prove_trips(cus, grids, "k_facets_records", len(aset), "record form")
            else:
                assert "k_facets_records" in grids, grids
            # an active scope: the count rides in the flag pass, no second pass over the records
            cp.set_scope(2, 1)
            want = facet_words(tags[aset], 2, 1)
            F.launch_grids()
            got = fm.match_list(cp)
            grids = F.launch_grids()
            check(sink, want, (cus, needle, "fused"), found=len(got))
            assert "k_facets_records" not in grids and "k_scope_flag" not in grids, grids
            if needle == WIDE:
                prove_trips(cus, grids, "k_scope_flag_facets", len(aset), "fused form")
            # an output with room for 10 records, no scope: the scratch route and the fused form under the scope (0, 0)
            cp.set_scope(0, 0)
            want = facet_words(tags[aset])
            F.launch_grids()
            written, found = device_list(fm, cp, 10)
            grids = F.launch_grids()
            assert written == 10
            check(sink, want, (cus, needle, "capacity 10"), found=found)
            assert "k_scope_flag_facets" in grids, grids
        # the column form: the empty prompt over the range and over a candidate set
        fe = F.Matcher("", F.Config(pf_lanes=64, sw_lanes=64))
        fe.set_facets(sink)
        cp.set_scope(2, 1)
        F.launch_grids()
        recs, found = fe.match_list_top(cp, 50)
        grids = F.launch_grids()
        check(sink, facet_words(tags, 2, 1), (cus, "column, range"), found=found)
        prove_trips(cus, grids, "k_facets_column", N, "column form, range")
        s = F.Subset(cp)
        s.set_indices(wide)
        F.launch_grids()
        recs, found = fe.match_list_top(cp, 50, subset=s)
        grids = F.launch_grids()
        check(sink, facet_words(tags[wide], 2, 1), (cus, "column, subset"), found=found)
        prove_trips(cus, grids, "k_facets_column", len(wide), "column form, subset")
        # a `from_patterns` matcher with no pattern: identity records, then the record form
        mm = F.MultiMatcher([], F.Config(pf_lanes=64, sw_lanes=0))
        mm.set_facets(sink)
        cp.set_scope(0, 0)
        F.launch_grids()
        recs, found = mm.match_list_top(cp, 50)
        grids = F.launch_grids()
        check(sink, facet_words(tags), (cus, "no pattern"), found=found)
        prove_trips(cus, grids, "k_facets_records", N, "record form, no pattern")
