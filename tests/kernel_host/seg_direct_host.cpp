// TEST INFRASTRUCTURE: frizbee_amd/csrc/seg_list.h - the scorer's work assignment over the segmented survivor list (a direct round and a
// pool) - compiled for the host.  tests/test_seg_direct_host.py checks it against brute-force enumeration in plain Python.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "seg_list.h"

extern "C" {

uint32_t sd_direct_max(void) { return FZB_SEG_DIRECT; }
uint32_t sd_direct(uint32_t c, uint32_t s, uint32_t G) { return seg_direct(c, s, G); }
uint32_t sd_rest(uint32_t c, uint32_t s, uint32_t G) { return seg_rest(c, s, G); }

// The scorer's side on a grid of G workgroups of `threads` threads, as the kernel walks it: both exclusive prefixes, then every workgroup's
// direct items (workgroup b < nseg, lane t < d[b]) and every pool item, grid-strided from each thread's first.  Each item is recorded as
// (segment, slot, output position, workgroup that scores it) in the order visited; returns the number of items, or -1 if more than `cap`.
// totals[0] = sum of the counts, totals[1] = the pool's size.  pre / rpre have FZB_SEG_MAX entries.  padded != 0: the kernel's form of the
// search - the entries at and beyond nseg hold the totals and the bisection runs over all FZB_SEG_MAX entries in eleven fixed steps.
int64_t sd_walk(const uint32_t* counts, uint32_t nseg, uint32_t G, uint32_t threads, int padded, uint32_t* pre, uint32_t* rpre, uint32_t* totals,
                uint32_t* out_seg, uint32_t* out_slot, uint32_t* out_pos, uint32_t* out_wg, uint64_t cap) {
    uint32_t run = 0, rrun = 0;
    for (uint32_t s = 0; s < nseg; s++) {
        pre[s] = run;
        rpre[s] = rrun;
        run += counts[s];
        rrun += seg_rest(counts[s], s, G);
    }
    totals[0] = run;
    totals[1] = rrun;
    for (uint32_t s = nseg; s < FZB_SEG_MAX; s++) {
        pre[s] = run;
        rpre[s] = rrun;
    }
    const uint32_t n_search = padded ? FZB_SEG_MAX : nseg, top = padded ? FZB_SEG_MAX / 2 : seg_top(nseg);
    uint64_t n = 0;
    for (uint32_t b = 0; b < G; b++) {
        if (b < nseg)
            for (uint32_t t = 0; t < threads && t < seg_direct(counts[b], b, G); t++) {
                if (n >= cap) return -1;
                out_seg[n] = b;
                out_slot[n] = t;
                out_pos[n] = pre[b] + t;
                out_wg[n++] = b;
            }
        for (uint32_t t = 0; t < threads; t++)
            for (uint64_t jp = (uint64_t)b * threads + t; jp < rrun; jp += (uint64_t)G * threads) {
                if (n >= cap) return -1;
                const SegItem it = seg_pool_item(pre, rpre, n_search, top, G, (uint32_t)jp);
                out_seg[n] = it.seg;
                out_slot[n] = it.slot;
                out_pos[n] = it.pos;
                out_wg[n++] = b;
            }
    }
    return (int64_t)n;
}

}  // extern "C"
