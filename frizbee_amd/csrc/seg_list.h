// The SEGMENTED survivor list of the signature filter (k1_dfa_sig<.., SEG>, kernels_filter.hip -> k2b_dp_short<.., SEG>, kernels_dp.hip).
// Workgroup b of the filter owns the contiguous run of tiles tile_compact.h gives it (tc_run, T = tc_tiles_per_run(ntiles, grid)), and lists the
// survivors of its run itself, in ascending order, at seg_list[b * T * FZB_TILE + k]; seg_counts[b] says how many.  Segment b starts at its
// first tile's first item, so segments cannot overlap and the list needs no more room than the range rounded up to a tile.  The scorer turns
// the <= FZB_SEG_MAX counts into exclusive prefixes in LDS and maps its work items to (segment, slot) - no compaction launch in between.
//
// The scorer's work assignment (G = its grid): its workgroup b takes the first FZB_SEG_DIRECT survivors of segment b DIRECTLY - lane t scores
// seg_list[b * stride + t], an address known at launch, and the one word seg_counts[b] says which lanes hold one (a lane beyond it reads
// nothing: a trailing segment's run may lie beyond the list's room) - so its first rows are in flight before any prefix exists.  What the
// direct round leaves (all of a segment s >= G, the survivors beyond the first FZB_SEG_DIRECT of a segment s < G) is the POOL, walked
// grid-strided: pool item j' belongs to the last segment whose exclusive prefix of the REST counts is <= j'.
// A survivor's output position is its rank in the whole list either way (exclusive prefix of the counts + its slot), so records stay
// index-ordered and dense.  With d[s] = seg_direct, r[s] = seg_rest, P / R = exclusive prefixes of the counts / of the rests:
//   direct item (b, t), t < d[b]:  list entry t of segment b                        -> output position P[b] + t
//   pool item j' < sum(r):         list entry d[s] + (j' - R[s]) of s = seg_find(R) -> output position P[s] + that entry
//
// Pure functions, host and device: tests/test_seg_list_host.py and tests/test_seg_direct_host.py compile this header for the CPU.
#pragma once
#include <stdint.h>

#include "tile_compact.h"

#ifndef FZB_SEG_FN
#define FZB_SEG_FN __host__ __device__ inline
#endif

#define FZB_SEG_MAX 2048u  // segments (= workgroups of the filter) at most: the scorer's prefix array in LDS

// The largest power of two below nseg (1 for nseg <= 2): the first step of seg_find.
FZB_SEG_FN uint32_t seg_top(uint32_t nseg) {
    uint32_t top = 1;
    while (2u * top < nseg) top *= 2u;
    return top;
}
// The LAST segment s with pre[s] <= j, pre = exclusive prefix of the nseg counts (pre[0] = 0), j < total.  Empty segments share their
// successor's prefix, so the last one with pre[s] <= j is the one that holds j.  `top` = seg_top(nseg).
FZB_SEG_FN uint32_t seg_find(const uint32_t* pre, uint32_t nseg, uint32_t top, uint32_t j) {
    uint32_t s = 0;
#ifdef __HIP_DEVICE_COMPILE__  // (the scorer passes constants: straight-line code, so that independent searches interleave)
#pragma unroll
#endif
    for (uint32_t step = top; step; step >>= 1)
        if (s + step < nseg && pre[s + step] <= j) s += step;
    return s;
}

// ---- the scorer's work assignment: a direct round and a pool (see the top of this file) --------------------------------------------------
#define FZB_SEG_DIRECT 128u  // survivors of segment b that scorer workgroup b takes directly: one per thread of k2b_dp_short's workgroup

// d[s]: how many of segment s's c survivors the direct round takes on a scorer grid of G workgroups; r[s] = what is left to the pool
FZB_SEG_FN uint32_t seg_direct(uint32_t c, uint32_t s, uint32_t G) { return s < G ? (c < FZB_SEG_DIRECT ? c : FZB_SEG_DIRECT) : 0u; }
FZB_SEG_FN uint32_t seg_rest(uint32_t c, uint32_t s, uint32_t G) { return c - seg_direct(c, s, G); }
// d[s] of a segment that HAS pool items, without its count: such a segment has given the direct round all it takes (or is beyond the grid)
FZB_SEG_FN uint32_t seg_pool_first(uint32_t s, uint32_t G) { return s < G ? FZB_SEG_DIRECT : 0u; }

struct SegItem {
    uint32_t seg, slot, pos;  // list entry `slot` of segment `seg` goes to output position `pos`
};
// Pool item jp < sum(r).  pre / rpre = exclusive prefixes of the counts / of the rests over the nseg segments, top = seg_top(nseg).
FZB_SEG_FN SegItem seg_pool_item(const uint32_t* pre, const uint32_t* rpre, uint32_t nseg, uint32_t top, uint32_t G, uint32_t jp) {
    SegItem it;
    it.seg = seg_find(rpre, nseg, top, jp);
    it.slot = seg_pool_first(it.seg, G) + (jp - rpre[it.seg]);
    it.pos = pre[it.seg] + it.slot;
    return it;
}
