// TEST INFRASTRUCTURE: frizbee_amd/csrc/seg_list.h - the arithmetic of the segmented survivor list (a workgroup's run of tiles, the slot of a
// set bit in its tile - both tile_compact.h's -, the segment that holds survivor j) - compiled for the host.  tests/test_seg_list_host.py checks it against plain Python.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "seg_list.h"

extern "C" {

uint32_t sg_max(void) { return FZB_SEG_MAX; }
uint32_t sg_tiles_per_run(uint32_t ntiles, uint32_t grid) { return tc_tiles_per_run(ntiles, grid); }
void sg_run(uint32_t ntiles, uint32_t T, uint32_t b, uint32_t* out) { tc_run(ntiles, T, b, &out[0], &out[1]); }
uint32_t sg_top(uint32_t nseg) { return seg_top(nseg); }

// the scorer's side: exclusive prefix of the counts (as the kernel builds it), then every j in [0, total]: out_seg[j], out_slot[j];
// j = total is looked up too (the kernel never does: it maps to nothing, which the test checks through the returned prefix)
uint32_t sg_map_all(const uint32_t* counts, uint32_t nseg, uint32_t* pre, uint32_t* out_seg, uint32_t* out_slot) {
    uint32_t run = 0;
    for (uint32_t s = 0; s < nseg; s++) {
        pre[s] = run;
        run += counts[s];
    }
    const uint32_t top = seg_top(nseg);
    for (uint32_t j = 0; j <= run; j++) {
        const uint32_t s = seg_find(pre, nseg, top, j);
        out_seg[j] = s;
        out_slot[j] = j - pre[s];
    }
    return run;
}

// the filter's side: the slots of one tile's set bits from its 32 decision words (word popcounts scanned, tc_rank32 per bit), in the order
// the kernel's threads take the positions (p * 256 + tid); out_pos[slot] = position; returns the tile's count
uint32_t sg_rank_tile(const uint32_t* words, uint32_t* out_pos) {
    uint32_t excl[32], run = 0;
    for (int w = 0; w < 32; w++) {
        excl[w] = run;
        run += (uint32_t)__builtin_popcount(words[w]);
    }
    for (uint32_t p = 0; p < 4; p++)
        for (uint32_t tid = 0; tid < 256; tid++) {
            const uint32_t pos = p * 256 + tid, w = pos >> 5;
            if ((words[w] >> (pos & 31)) & 1) out_pos[tc_rank32(excl[w], words[w], pos & 31)] = pos;
        }
    return run;
}

}  // extern "C"
