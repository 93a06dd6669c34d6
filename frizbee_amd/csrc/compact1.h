// Level-1 compaction, the body shared by k_compact1 (kernels_filter.hip) and the fused compaction + classification kernel of ragged ASCII lists
// (k_compact1_classify, kernels_dp.hip): see k_compact1 for the scheme.  `after_batch(first_position, survivors)` is called by the WHOLE workgroup
// (workgroup-uniform arguments) once the survivor indices [first_position, first_position + survivors) of a batch of this workgroup's tiles are in
// out_idx and visible to the workgroup; `at_end(total)` by thread 0 of the last workgroup with the list's total.
#pragma once
#include "fzb_internal.h"
#include "tile_compact.h"

template <class AfterBatch, class AtEnd>
__device__ __forceinline__ void compact1_body(const u64* __restrict__ bitmap, const u32* __restrict__ counts, u32 n_items_host, const u32* __restrict__ n_items_ptr,
                                              const u32* __restrict__ src, u32* __restrict__ out_idx, u32* __restrict__ total_out, u32* __restrict__ total_out2,
                                              AfterBatch after_batch, AtEnd at_end) {

    // n_items_ptr (device) overrides the host count; src, if given, maps a bit position to the value that is listed
    // (the item-list form of the filter: positions in a candidate list -> haystack indices)
    __shared__ u32 red[4];
    __shared__ u32 pre[TC_BATCH];
    const u32 n_items = n_items_ptr ? *n_items_ptr : n_items_host;
    const u32 tid = threadIdx.x;
    const u32 ntiles = (n_items + FZB_TILE - 1) / FZB_TILE;
    u32 t0, t1;
    tc_run(ntiles, tc_tiles_per_run(ntiles, gridDim.x), blockIdx.x, &t0, &t1);
    // Everything this workgroup reads is requested up front - its first batch of tile counts, the first 256 bitmap words of that batch and
    // the counts before its run - so that the three dependent round trips of the straightforward order (prefix, batch counts, words)
    // overlap into one; for the 10 M-haystack list a workgroup has ~10 tiles = 152 words, i.e. nothing is left to load afterwards.
    const u32 nwords = (n_items + 63) / 64;
    const u32 nt_first = min((u32)TC_BATCH, t1 - t0);
    const u32 c_first = tid < nt_first ? counts[t0 + tid] : 0u;
    const u32 w_first = t0 * (FZB_TILE / 64) + tid;
    const u64 bits_first = (w_first < (t0 + nt_first) * (FZB_TILE / 64) && w_first < nwords) ? bitmap[w_first] : 0ull;
    // survivors before tile t0 (tile_compact.h: the kernel's critical path)
    u32 base = tc_prefix(counts, t0, red);
    for (u32 tb = t0; tb < t1; tb += TC_BATCH) {  // batches of up to 256 tiles
        const u32 nt = min((u32)TC_BATCH, t1 - tb);
        const u32 batch_total = tc_batch_scan(tb == t0 ? c_first : (tid < nt ? counts[tb + tid] : 0u), base, pre, red);
        // expand the bitmap words of these tiles: the 16 words of a tile sit in 16 consecutive lanes (w0 is a multiple of 16),
        // so a word's offset inside its tile is a 16-lane segmented scan of the popcounts - no re-reading of the earlier words
        const u32 w0 = tb * (FZB_TILE / 64), w1 = (tb + nt) * (FZB_TILE / 64);
        for (u32 wb0 = w0; wb0 < w1; wb0 += 256) {  // uniform trip count: the shuffles below need every lane
            const u32 w = wb0 + tid;
            const bool live = w < w1 && w < nwords;
            u64 bits = (tb == t0 && wb0 == w0) ? bits_first : (live ? bitmap[w] : 0ull);
            const u32 c = (u32)__popcll(bits);
            const u32 incl = tc_scan16(c);
            if (!bits) continue;
            const u32 tile = w / (FZB_TILE / 64);
            u32 pos = pre[tile - tb] + incl - c;
            while (bits) {
                const int b = __builtin_ctzll(bits);
                bits &= bits - 1;
                out_idx[pos++] = src ? src[w * 64 + b] : w * 64 + b;
            }
        }
        after_batch(base, batch_total);
        base += batch_total;
        __syncthreads();
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {  // every earlier workgroup's tiles precede this one's
        *total_out = base;
        if (total_out2) *total_out2 = base;  // (a second counter that starts as the same number: the unicode path's "kept by the exact prefilter")
        at_end(base);
    }
}
