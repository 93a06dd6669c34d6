"""Small-device parity of the sectioned top-`limit`: the library told to behave as on a device of 1, 2 and 5 compute units (FZB_DEBUG_CUS)
with the needle `g`, which most of test_gpu_facets' list matches, so that every grid-stride loop of kernels_sections.hip - over records
(k_sec_hist), over 2048-record tiles (k_sec_tile_counts, k_sec_scatter), over the 2S tile rows (k_sec_scan) and over the sections
(k_sec_cut, k_sec_order) - takes more than one trip.  Results are the oracle's, as in tests/test_gpu_sections.py; the proof of the trips is
from the grids the library recorded for that very call: work units / (recorded grid x the units one workgroup takes per trip) >= 2 at one
compute unit."""
import pytest

import frizbee_amd as F
from test_gpu_sections import SECTIONS, assert_sections, corpus, relies_on, want_list
from test_gpu_small_device import CUS, device_of
from test_gpu_topk import single

pytestmark = pytest.mark.gpu
WIDE = "g"
S = len(SECTIONS)
# kernel -> (what its loop strides over, units per workgroup and trip)
LOOPS = {"k_sec_hist": ("records", 256), "k_sec_tile_counts": ("tiles", 1), "k_sec_scatter": ("tiles", 1), "k_sec_scan": ("rows", 1), "k_sec_cut": ("sections", 1),
         "k_sec_order": ("sections", 1)}


def prove_trips(cus, grids, kernels, records, ctx):
    units = {"records": records, "tiles": (records + 2047) // 2048, "rows": 2 * S, "sections": S}
    assert set(k for k in grids if k.startswith("k_sec_")) == set(kernels), (ctx, sorted(grids))
    for kernel in kernels:
        what, per_trip = LOOPS[kernel]
        q = units[what] / (grids[kernel][1] * per_trip)
        print("coverage", cus, ctx, kernel, grids[kernel], what, units[what], round(q, 2))
        if cus == 1:
            assert q >= 2, (ctx, kernel, q, grids[kernel], units[what])


@pytest.mark.parametrize("cus", CUS)
def test_every_loop_of_the_stage_on_a_small_device(cus):
    # (sort, bias, the kernels the form launches): two levels under the bias, one level without, no histogram by index
    forms = (("ScoreThenIndexDesc", True, ("k_sec_hist", "k_sec_cut", "k_sec_tile_counts", "k_sec_scan", "k_sec_scatter", "k_sec_order")),
             ("ScoreThenIndexAsc", False, ("k_sec_hist", "k_sec_cut", "k_sec_tile_counts", "k_sec_scan", "k_sec_scatter", "k_sec_order")),
             ("IndexDesc", False, ("k_sec_cut", "k_sec_tile_counts", "k_sec_scan", "k_sec_scatter", "k_sec_order")),
             ("IndexAsc", True, ("k_sec_cut", "k_sec_tile_counts", "k_sec_scan", "k_sec_scatter")))
    for sort, use_bias, kernels in forms:
        wants = [want_list(WIDE, sort, (0, 0), sec, use_bias) for sec in SECTIONS]
        records = len(wants[2])  # section (0, 0): every match
        assert records > 2 * 2 * 2048 and records > 2 * 2 * 256  # two trips of a grid of two workgroups, by tiles and by records
        assert {"ties", "keep_all", "empty"} <= relies_on(wants, (5, 1024), sort)
        with device_of(cus):
            cp = corpus((0, 0), use_bias)
            fm, _ = single(WIDE, sort=sort)
            for limit in (5, 1024):
                F.launch_grids()
                got = fm.match_list_top_sections(cp, SECTIONS, limit)
                grids = F.launch_grids()
                assert_sections(got, wants, limit, (cus, sort, use_bias, limit))
                prove_trips(cus, grids, kernels, records, (sort, use_bias, limit))
            if sort == "ScoreThenIndexDesc":
                assert grids["k_sec_hist"][2] == 2 and grids["k_sec_cut"][2] == 2  # both levels
            if sort == "ScoreThenIndexAsc":
                assert grids["k_sec_hist"][2] == 1 and grids["k_sec_cut"][2] == 1  # every score is below 256: one level
