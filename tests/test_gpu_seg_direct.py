"""The short scorer over the filter's segmented survivor list (k2b_dp_short<.., SEG>, seg_list.h): workgroup b takes the first 128 survivors of
segment b directly, the rest is a pool.  Lists of 6 and 21 tiles with rows planted so that segments hold exactly 0, 1, 127, 128, 129
survivors or every row, on devices of 1, 2 and 5 compute units (FZB_DEBUG_CUS) and with the segment size set through
fzb_debug_set_filter_grid.  Every case runs in the segmented form and with FZB_NO_SEG_LIST=1: the two results must be byte-identical and both
must equal the ORACLE's records - never this library's own."""
import contextlib

import numpy as np
import pytest

import frizbee_amd as F
from test_gpu_score_bias import same
from test_gpu_small_device import device_of
from test_gpu_topk import opad, single

pytestmark = pytest.mark.gpu
CUS = (1, 2, 5)
TILE = 1024
N = 20 * 1024 + 37  # 21 tiles, a short last one
N6 = 5 * 1024 + 300  # 6 tiles
NEEDLE = "deadbe"
FILLER = np.frombuffer(b"ghijklmnopqrstuv", np.uint8)  # spells nothing of the needle
VARIANTS = (b"deadbe", b"deaDbe", b"DEADBE", b"de_ad-be", b"xdeadbe")  # every one matches the lowercase needle without a typo; scores differ
ALL = -1  # a segment's count: every row of the segment


def layout(n, cus, debug_grid=0):
    """(segments, rows per segment) as the host lays the filter out: grid = min(cus * 8, 2048, tiles[, the debug grid]), runs of ceil(tiles / grid)"""
    ntiles = -(-n // TILE)
    grid = min(cus * 8, 2048, ntiles)
    if debug_grid:
        grid = min(grid, debug_grid)
    return grid, -(-ntiles // grid) * TILE


def planted_at(n, nseg, seg_rows, counts, seed):
    """the planted indices: counts[s] rows of segment s (its first and its last row among them where the count allows), ascending"""
    rng = np.random.default_rng(seed)
    at = []
    for s in range(nseg):
        lo, hi = min(s * seg_rows, n), min((s + 1) * seg_rows, n)
        c = hi - lo if counts[s] == ALL else min(counts[s], hi - lo)
        if c >= hi - lo:
            pick = np.arange(lo, hi)
        else:
            ends = [x for x in (hi - 1, lo)][: min(c, 2)]
            inner = rng.choice(np.arange(lo + 1, hi - 1), c - len(ends), replace=False) if c > len(ends) else np.zeros(0, np.int64)
            pick = np.sort(np.concatenate([np.array(ends, np.int64), inner]))
        at.append(pick)
    return np.concatenate(at).astype(np.int64) if at else np.zeros(0, np.int64)


def make_rows(n, at, width=32, seed=0, variants=VARIANTS):
    """n rows of `width` filler bytes, a variant of the needle planted at a varying offset in the rows `at`"""
    rng = np.random.default_rng(1000 + seed)
    rows = rng.choice(FILLER, (n, width))
    for k, i in enumerate(at.tolist()):
        v = np.frombuffer(variants[(k + i) % len(variants)], np.uint8)
        off = (k * 7 + i) % (width - len(v) + 1)
        rows[i, off:off + len(v)] = v
    return rows


def packed(rows):
    return rows.reshape(-1).copy(), np.arange(1, len(rows) + 1, dtype=np.uint64) * np.uint64(rows.shape[1])


@contextlib.contextmanager
def filter_grid(g):
    F.lib().fzb_debug_set_filter_grid(int(g))
    try:
        yield
    finally:
        F.lib().fzb_debug_set_filter_grid(0)


def both_forms(cus, data, ends, run, want, ctx, nseg=None, seg=True):
    """run(matcher-side callable: corpus -> records) in the segmented form and with FZB_NO_SEG_LIST=1: byte-identical, both the oracle's"""
    got = {}
    for env in ({}, {"FZB_NO_SEG_LIST": "1"}):
        with device_of(cus, **env):
            cp = F.Corpus(packed=(data, ends))
            F.launch_grids()
            got[bool(env)] = run(cp)
            grids = F.launch_grids()
            assert "k2b_dp_short" in grids, (ctx, env, sorted(grids))
            if seg:  # the form under test ran: no compaction launch between the filter and the scorer
                assert ("k_compact1" in grids) == bool(env), (ctx, env, sorted(grids))
                if nseg is not None and not env:
                    assert grids["k1_dfa_sig"][1] == nseg, (ctx, grids["k1_dfa_sig"], nseg)
    same(got[False], want, (ctx, "segmented"))
    same(got[True], want, (ctx, "FZB_NO_SEG_LIST"))
    assert got[False].tobytes() == got[True].tobytes(), ctx


def per_segment(indices, nseg, seg_rows):
    return np.bincount(np.asarray(indices, np.int64) // seg_rows, minlength=nseg).tolist()


EDGE = (0, 1, 127, 128, 129, ALL)


@pytest.mark.parametrize("cus", CUS)
def test_segments_of_every_edge_count(cus):
    """0, 1, 127, 128, 129 survivors and a dense segment, in turn over the segments of a 21-tile list: segments of 3, 2 and 1 tiles"""
    nseg, seg_rows = layout(N, cus)
    for shift in (0, 3):
        counts = [EDGE[(s + shift) % len(EDGE)] for s in range(nseg)]
        at = planted_at(N, nseg, seg_rows, counts, seed=cus)
        data, ends = packed(make_rows(N, at, seed=cus))
        fm, om = single(NEEDLE)
        want = om.match_packed(opad(data), ends)
        assert per_segment(want["index"], nseg, seg_rows) == per_segment(at, nseg, seg_rows), "the planting"
        both_forms(cus, data, ends, fm.match_list, want, ("edge counts", cus, shift), nseg)


@pytest.mark.parametrize("grid", (1, 2, 3, 6))
@pytest.mark.parametrize("cus", CUS)
def test_a_six_tile_list_with_the_segment_size_set(cus, grid):
    """segments of 6, 3, 2 and 1 tiles: edge counts; every survivor inside one segment, the others empty; no survivor at all"""
    with filter_grid(grid):
        nseg, seg_rows = layout(N6, cus, grid)
        plans = [[EDGE[(s + 1) % len(EDGE)] for s in range(nseg)], [0] * nseg]
        plans.append([(128, 1, 0, 127)[(s + cus) % 4] for s in range(nseg)])  # no segment beyond the direct round: no pool at all
        for only in sorted({0, nseg // 2, nseg - 1}):
            for c in (129, ALL):
                plans.append([c if s == only else 0 for s in range(nseg)])
        for k, counts in enumerate(plans):
            at = planted_at(N6, nseg, seg_rows, counts, seed=10 * cus + grid)
            data, ends = packed(make_rows(N6, at, seed=k))
            fm, om = single(NEEDLE)
            want = om.match_packed(opad(data), ends)
            assert len(want) == len(at) and (any(counts) or len(want) == 0)
            both_forms(cus, data, ends, fm.match_list, want, ("six tiles", cus, grid, counts), nseg)


@pytest.mark.parametrize("cus", CUS)
def test_capacity_below_the_number_of_matches(cus):
    import torch

    nseg, seg_rows = layout(N, cus)
    counts = [EDGE[(s + 2) % len(EDGE)] for s in range(nseg)]
    at = planted_at(N, nseg, seg_rows, counts, seed=20 + cus)
    data, ends = packed(make_rows(N, at, seed=20 + cus))
    fm, om = single(NEEDLE, sort="IndexAsc")
    want = om.match_packed(opad(data), ends)
    found = len(want)
    assert found > 1024
    for capacity in (found - 1, found // 2, 130, 1):

        def run(cp):
            out = torch.full(((capacity + 64) * 8,), 0xEE, dtype=torch.uint8, device="cuda")
            cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
            fm.match_list_device(cp, out.data_ptr(), capacity, cnt.data_ptr())
            torch.cuda.synchronize()
            assert cnt[:2].tolist() == [capacity, found], (capacity, cnt.tolist())
            host = out.cpu().numpy()
            assert (host[capacity * 8:] == 0xEE).all(), "wrote beyond the capacity"
            return host[: capacity * 8].view(F.MATCH_DTYPE).copy()

        both_forms(cus, data, ends, run, want[:capacity], ("capacity", cus, capacity), nseg)


@pytest.mark.parametrize("cus", CUS)
def test_a_range_that_starts_at_a_tile_with_an_index_offset(cus):
    first, count = 2 * TILE, N - 2 * TILE - 300
    nseg, seg_rows = layout(count, cus)
    counts = [EDGE[(s + 4) % len(EDGE)] for s in range(nseg)]
    at = first + planted_at(count, nseg, seg_rows, counts, seed=30 + cus)
    at = np.concatenate([np.arange(0, first, 3), at, np.arange(first + count, N)])  # matches in front of and behind the range as well
    rows = make_rows(N, at, seed=30 + cus)
    data, ends = packed(rows)
    fm, om = single(NEEDLE, sort="IndexAsc")
    rdata, rends = packed(rows[first:first + count])
    want = om.match_packed(opad(rdata), rends)
    assert per_segment(want["index"], nseg, seg_rows) == per_segment(at[(at >= first) & (at < first + count)] - first, nseg, seg_rows), "the planting"
    want["index"] += 1000
    both_forms(cus, data, ends, lambda cp: fm.match_list_into(cp, first=first, count=count, index_offset=1000), want, ("range", cus), nseg)


@pytest.mark.parametrize("cus", CUS)
def test_an_uppercase_needle(cus):
    """smart case respects the needle's uppercase letter: the UPPER instantiation"""
    nseg, seg_rows = layout(N6, cus)
    counts = [EDGE[(s + 1) % len(EDGE)] for s in range(nseg)]
    at = planted_at(N6, nseg, seg_rows, counts, seed=40 + cus)
    data, ends = packed(make_rows(N6, at, seed=40 + cus, variants=(b"deaDbe", b"xdeaDbe", b"de_aD-be")))
    fm, om = single("deaDbe", casing="Smart")
    want = om.match_packed(opad(data), ends)
    assert per_segment(want["index"], nseg, seg_rows) == per_segment(at, nseg, seg_rows), "the planting"
    both_forms(cus, data, ends, fm.match_list, want, ("uppercase", cus), nseg)


@pytest.mark.parametrize("cus", CUS)
def test_thirty_two_lanes_over_haystacks_of_at_most_sixteen_bytes(cus):
    """sw_lanes = 32: the SWL = 32 instantiation, rows of 7 .. 16 bytes behind end offsets"""
    nseg, seg_rows = layout(N6, cus)
    counts = [EDGE[(s + 5) % len(EDGE)] for s in range(nseg)]
    at = planted_at(N6, nseg, seg_rows, counts, seed=50 + cus)
    rows = make_rows(N6, at, width=16, seed=50 + cus, variants=(b"deadbe", b"DEADBE"))
    lens = np.random.default_rng(50 + cus).integers(7, 17, N6)
    for i in at.tolist():  # a planted row keeps its needle: cut behind it only
        lens[i] = max(lens[i], int(np.flatnonzero(~np.isin(rows[i], FILLER)).max()) + 1)
    data = np.concatenate([rows[i, : lens[i]] for i in range(N6)])
    ends = np.cumsum(lens).astype(np.uint64)
    fm, om = single(NEEDLE, pf=32)
    want = om.match_packed(opad(data), ends)
    assert per_segment(want["index"], nseg, seg_rows) == per_segment(at, nseg, seg_rows), "the planting"
    both_forms(cus, data, ends, fm.match_list, want, ("32 lanes", cus), nseg)
