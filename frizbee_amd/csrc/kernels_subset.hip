// gfx950 kernels of the candidate sets (fzb_subset, include/frizbee_hip.h): the capture of a query's match set and the flag pass of
// fzb_subset_from_scope.  The reference has no such notion: its `match_list` always takes the whole slice.
#include "kernels_common.h"
#include "scope.h"

// The match set of a query: the index-ordered records the scorers wrote (n = min(*n_ptr, cap) of them, numbered from index_offset) -> their
// haystack indices, ascending because the records are, and the count beside them.  k_records_to_items' sibling: it also publishes the
// count - into the subset and, for the host forms, into a word their one wait brings back (`mirror`, may be null).
__global__ __launch_bounds__(256) void k_subset_capture(const fzb_match_rec* __restrict__ recs, const u32* __restrict__ n_ptr, u32 cap, u32 index_offset, u32* __restrict__ items,
                                                        u32 items_cap, u32* __restrict__ count_out, u32* __restrict__ mirror) {
    const u32 n = min(min(*n_ptr, cap), items_cap);
    for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) items[j] = recs[j].index - index_offset;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *count_out = n;
        if (mirror) *mirror = n;
    }
}
void fzb_launch_subset_capture(const fzb_match_rec* recs, const u32* n_ptr, u32 cap, u32 index_offset, u32* items, u32 items_cap, u32* count_out, u32* mirror, int grid_max, hipStream_t st) {
    const u32 blocks = (cap + 255u) / 256u, most = grid_max > 0 ? (u32)grid_max : 1u;
    const int grid = (int)(blocks < most ? (blocks ? blocks : 1u) : most);
    FZB_LAUNCH(k_subset_capture, dim3(grid), dim3(256), 0, st, recs, n_ptr, cap, index_offset, items, items_cap, count_out, mirror);
}

// The flag pass of fzb_subset_from_scope, in the shape of k_scope_flag but over the HAYSTACKS 0 .. n - 1 instead of over records: one ballot
// word per 64 haystacks and the visible count per 1024-haystack tile; k_compact1 (kernels_filter.hip) then lists the set bits in order.
// tags == nullptr: a corpus without tags, every tag 0.  The predicate is scope.h's.
__global__ __launch_bounds__(256) void k_subset_scope_flag(const uint16_t* __restrict__ tags, u32 n, u32 require, u32 exclude, u64* __restrict__ bitmap, u32* __restrict__ tile_counts) {
    __shared__ u32 s_cnt;
    const u32 ntiles = (n + SCOPE_TILE - 1) / SCOPE_TILE;
    const int tid = threadIdx.x;
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        u32 cnt = 0;
        for (int p = 0; p < SCOPE_TILE / 256; p++) {
            const u32 i = tile * SCOPE_TILE + p * 256 + tid;
            const bool keep = i < n && scope_visible(tags ? (u32)tags[i] : 0u, require, exclude);
            const u64 b = __ballot(keep);
            if (lane_id() == 0) {
                bitmap[(u64)tile * SCOPE_WORDS + p * 4 + (tid >> 6)] = b;
                cnt += __popcll(b);
            }
        }
        if (lane_id() == 0 && cnt) atomicAdd(&s_cnt, cnt);
        __syncthreads();
        if (tid == 0) tile_counts[tile] = s_cnt;
        __syncthreads();
    }
}
// the visible haystacks of a list of n, ascending, into `out` (room for n) and their number into *count_out; bitmap: 16 words per 1024
// haystacks, tile_counts: one word per 1024 (padded to a multiple of four: k_compact1 sums them as 16-byte loads)
void fzb_launch_subset_from_scope(const uint16_t* tags, u32 n, u32 require, u32 exclude, u64* bitmap, u32* tile_counts, u32* out, u32* count_out, int grid_max, hipStream_t st) {
    const u32 tiles = (n + SCOPE_TILE - 1) / SCOPE_TILE, most = grid_max > 0 ? (u32)grid_max : 1u;
    const int grid = (int)(tiles < most ? (tiles ? tiles : 1u) : most);
    FZB_LAUNCH(k_subset_scope_flag, dim3(grid), dim3(256), 0, st, tags, n, require, exclude, bitmap, tile_counts);
    fzb_launch_compact1(bitmap, tile_counts, n, nullptr, nullptr, out, count_out, grid, st);
}
