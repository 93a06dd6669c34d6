"""Small-device parity of the sectioned top-`limit` with matched positions: the library told to behave as on a device of 1, 2 and 5 compute
units (FZB_DEBUG_CUS) with the needle `g`, test_gpu_sections' eight sections and limit 1024, so that the grid-stride loop of k_sec_items over
the S * limit slab slots takes more than one trip.  Results are the oracle's, as in tests/test_gpu_sections_indices.py; the proof of the trips
is from the grid the library recorded for that very call: S * limit / (recorded grid x 256) >= 2 at one compute unit."""
import pytest

import frizbee_amd as F
from test_gpu_sections import SECTIONS, corpus, relies_on, want_list
from test_gpu_sections_indices import assert_sections_indices, positions_of, totals
from test_gpu_small_device import CUS, device_of
from test_gpu_topk import single

pytestmark = pytest.mark.gpu
WIDE = "g"
S = len(SECTIONS)
LIMIT = 1024


@pytest.mark.parametrize("cus", CUS)
def test_the_items_kernel_on_a_small_device(cus):
    pos = positions_of(WIDE)
    for sort, use_bias in (("ScoreThenIndexDesc", True), ("IndexAsc", False)):
        wants = [want_list(WIDE, sort, (0, 0), sec, use_bias) for sec in SECTIONS]
        assert {"ties", "keep_all", "empty"} <= relies_on(wants, (LIMIT,), sort) and totals(wants, LIMIT) > 2048
        with device_of(cus):
            cp = corpus((0, 0), use_bias)
            fm, _ = single(WIDE, sort=sort)
            F.launch_grids()
            got = fm.match_list_top_sections_indices(cp, SECTIONS, LIMIT)
            grids = F.launch_grids()
        assert_sections_indices(got, wants, pos, LIMIT, (cus, sort, use_bias))
        assert grids["k_sec_items"][2] == 1 and "k_top_items" not in grids, sorted(grids)
        q = S * LIMIT / (grids["k_sec_items"][1] * 256)
        print("coverage", cus, sort, "k_sec_items", grids["k_sec_items"], round(q, 2))
        if cus == 1:
            assert q >= 2, (q, grids["k_sec_items"])
