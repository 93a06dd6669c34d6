// The SEGMENTED survivor list of the signature filter (k1_dfa_sig<.., SEG>, kernels_filter.hip -> k2b_dp_short<.., SEG>, kernels_dp.hip).
// Workgroup b of the filter owns the contiguous run of tiles tile_compact.h gives it (tc_run, T = tc_tiles_per_run(ntiles, grid)), and lists the
// survivors of its run itself, in ascending order, at seg_list[b * T * FZB_TILE + k]; seg_counts[b] says how many.  Segment b starts at its
// first tile's first item, so segments cannot overlap and the list needs no more room than the range rounded up to a tile.  The scorer turns
// the <= FZB_SEG_MAX counts into an exclusive prefix in LDS and maps survivor j to (segment, slot) - no compaction launch in between.
//
// Pure functions, host and device: tests/test_seg_list_host.py compiles this header for the CPU.
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
