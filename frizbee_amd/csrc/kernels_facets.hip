// gfx950 kernels of the tag facets (facets.h): the per-tag match counts of a query, counted where the records and the tag column are.
// The reference has no such notion (its caller counts on the host).  Two forms live here - the record form for a producer's index-ordered
// records over a corpus with no active scope, the column form for the empty prompt's lists; the third, under an active scope, rides in
// the scope's flag pass (k_scope_flag_facets, kernels_topk.hip), which has the tag in a register.  All are grid-stride over 1024-item
// tiles, read their item count from device memory and publish through facets_publish: LDS, then at most FZB_FACET_WORDS vector atomicAdd
// per workgroup into a block the host cleared in stream order.  No workgroup waits for another.
#include "kernels_common.h"
#include "facets.h"

static_assert(sizeof(scope_rec) == sizeof(fzb_match_rec) && alignof(scope_rec) == alignof(fzb_match_rec), "the record form reads fzb_match_rec");

// ---- the record form: record j of count[0] index-ordered records (at most cap) belongs to haystack first + (index - index_offset).  One
// whole 8-byte record load (two dwords where the caller's array is only 4-byte aligned) and one 2-byte tag gather per record -
// near-coalesced, the records come in index order -, then the wave step.  (require, exclude) = (0, 0) where the corpus has no active
// scope: every record is visible.
__global__ __launch_bounds__(256) void k_facets_records(const scope_rec* __restrict__ recs, const u32* __restrict__ count, u32 cap, const uint16_t* __restrict__ tags, u64 n_tags, u64 first,
                                                        u32 index_offset, u32 require, u32 exclude, u32* __restrict__ block) {
    const u32 n = min(count[0], cap);
    const u32 ntiles = (n + (u32)SCOPE_TILE - 1u) / (u32)SCOPE_TILE;
    const bool wide = ((uintptr_t)recs & 7u) == 0;
    facet_acc acc;
    facets_clear(acc);
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
        for (u32 p = 0; p < SCOPE_TILE / 256; p++) {
            const u64 j = (u64)tile * SCOPE_TILE + p * 256u + threadIdx.x;
            const bool valid = j < n;
            u32 tag = 0;
            if (valid) {
                const u32 index = wide ? (*(const uint2*)(recs + j)).x : ((const u32*)(recs + j))[0];
                tag = scope_tag_of(tags, n_tags, first, index_offset, index);
            }
            facets_wave_step(acc, valid, tag, require, exclude);
        }
    }
    facets_publish(acc, block);
}

// ---- the column form: a thread per haystack of the range (items == nullptr, n_host of them from `first`) or per item of a candidate set,
// whose count is read HERE - after a _device capture the host does not know it (cap = the room the host knows of bounds it).  The tag
// column is read directly: the prompt's own producers never make records for hidden haystacks.  tags == nullptr: every tag 0.
__global__ __launch_bounds__(256) void k_facets_column(const u32* __restrict__ items, const u32* __restrict__ n_ptr, u32 n_host, u32 cap, const uint16_t* __restrict__ tags, u64 n_tags,
                                                       u64 first, u32 require, u32 exclude, u32* __restrict__ block) {
    const u32 n = items ? min(*n_ptr, cap) : n_host;
    const u32 ntiles = (n + (u32)SCOPE_TILE - 1u) / (u32)SCOPE_TILE;
    facet_acc acc;
    facets_clear(acc);
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll
        for (u32 p = 0; p < SCOPE_TILE / 256; p++) {
            const u64 k = (u64)tile * SCOPE_TILE + p * 256u + threadIdx.x;
            const bool valid = k < n;
            const u32 tag = valid ? facet_item_tag(items, k, tags, n_tags, first) : 0u;
            facets_wave_step(acc, valid, tag, require, exclude);
        }
    }
    facets_publish(acc, block);
}

// recs: count[0] index-ordered records (at most cap) numbered from index_offset over the range that starts at haystack `first`; tags may be
// null (n_tags 0).  The grid is sized from the capacity here and trimmed by the device-side count in the kernel.
void fzb_launch_facets_records(const fzb_match_rec* recs, const u32* count, u32 cap, const uint16_t* tags, u64 n_tags, u64 first, u32 index_offset, u32 require, u32 exclude, u32* block,
                               int grid_max, hipStream_t st) {
    const int grid = tc_grid(((u64)cap + SCOPE_TILE - 1) / SCOPE_TILE, grid_max);
    FZB_LAUNCH(k_facets_records, dim3(grid), dim3(256), 0, st, (const scope_rec*)recs, count, cap, tags, tags ? n_tags : 0, first, index_offset, require, exclude, block);
}

// items == nullptr: the n haystacks from `first`; else the candidate set (n_ptr: its count on the device, n = the room that bounds it, hint =
// what the host knows of its length - the grid's bound, not the loop's).
void fzb_launch_facets_column(const u32* items, const u32* n_ptr, u32 n, u32 hint, const uint16_t* tags, u64 n_tags, u64 first, u32 require, u32 exclude, u32* block, int grid_max,
                              hipStream_t st) {
    const int grid = tc_grid(((u64)(hint < n ? hint : n) + SCOPE_TILE - 1) / SCOPE_TILE, grid_max);
    FZB_LAUNCH(k_facets_column, dim3(grid), dim3(256), 0, st, items, n_ptr, n, n, tags, n_tags, first, require, exclude, block);
}
