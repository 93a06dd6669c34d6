// gfx950 kernels of the empty prompt (prompt_records.h): the index-ordered record list of an empty needle over a corpus with a score bias,
// an active scope or a candidate set, and its (written, found) pair, in device memory - the producer in front of the selection / ordering
// stage.  The reference's empty needle is closed-form host work (src/matcher/mod.rs:381-384: every index, score 0); with the list's terms
// the result depends on two per-haystack columns that live on the device.  Plain streaming kernels: no LDS beyond tile_compact.h's.
#include "kernels_common.h"
#include "prompt_records.h"

static_assert(SCOPE_TILE == FZB_TILE && sizeof(scope_rec) == sizeof(fzb_match_rec) && alignof(scope_rec) == alignof(fzb_match_rec), "the prompt writes fzb_match_rec");

// ---- the whole range, no active scope: haystack first + j is record j.  One thread per record, grid-stride: the 2-byte bias (or nothing)
// in, one 8-byte record out (two dwords where the caller's array is only 4-byte aligned).  What k_identity_records + k_bias_apply do in two
// launches and three passes over the records.
__global__ __launch_bounds__(256) void k_prompt_records(scope_rec* __restrict__ out, u32 n, u32 capacity, const int16_t* __restrict__ bias, u64 n_bias, u64 first, u32 index_offset,
                                                        u32* __restrict__ count_out) {
    const u32 m = min(n, capacity);
    const bool wide = ((uintptr_t)out & 7u) == 0;
    for (u32 j = blockIdx.x * 256u + threadIdx.x; j < m; j += gridDim.x * 256u) {
        const scope_rec r = prompt_record(bias, n_bias, first, index_offset, j);
        if (wide) *(uint2*)(out + j) = make_uint2(r.index, r.rest);
        else out[j] = r;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) scope_counts(n, capacity, count_out);
}

// ---- an active scope and / or a candidate set: flag pass + stable compaction (tile_compact.h).  The item list is the range (items ==
// nullptr, n_host items) or the set's ascending indices, whose count is read HERE: after a _device capture the host does not know it
// (cap = the room the host knows of bounds it).
__device__ __forceinline__ u32 prompt_items(const u32* __restrict__ items, const u32* __restrict__ n_ptr, u32 n_host, u32 cap) { return items ? min(*n_ptr, cap) : n_host; }

__global__ __launch_bounds__(256) void k_prompt_flag(const u32* __restrict__ items, const u32* __restrict__ n_ptr, u32 n_host, u32 cap, const uint16_t* __restrict__ tags, u64 n_tags,
                                                     u64 first, u32 require, u32 exclude, u64* __restrict__ bitmap, u32* __restrict__ tile_counts) {
    const u32 n = prompt_items(items, n_ptr, n_host, cap);
    tc_flag_pass(n, bitmap, tile_counts, [&](u32 tile, u32 slot) { return prompt_tile_keeps(items, n, tile, slot, tags, n_tags, first, require, exclude); });
}

// the compaction's `place` writes the finished record, the bias already added: no second buffer of records, no separate bias launch
__global__ __launch_bounds__(256) void k_prompt_compact(const u64* __restrict__ bitmap, const u32* __restrict__ counts, const u32* __restrict__ items, const u32* __restrict__ n_ptr,
                                                        u32 n_host, u32 cap, const int16_t* __restrict__ bias, u64 n_bias, u64 first, u32 index_offset, scope_rec* __restrict__ out,
                                                        u32 capacity, u32* __restrict__ count_out) {
    const u32 n = prompt_items(items, n_ptr, n_host, cap);
    const u32 kept = tc_compact_items(bitmap, counts, n, [&](u32 place, u64 k) { prompt_store(out, capacity, place, items, k, bias, n_bias, first, index_offset); });
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) scope_counts(kept, capacity, count_out);
}

// out: room for `capacity` records; count_out: (written, found = n).  bias may be null (score 0).
void fzb_launch_prompt_records(fzb_match_rec* out, u32 n, u32 capacity, const int16_t* bias, u64 n_bias, u64 first, u32 index_offset, u32* count_out, int grid_max, hipStream_t st) {
    const int grid = tc_grid(((u64)(n < capacity ? n : capacity) + 255u) / 256u, grid_max);
    FZB_LAUNCH(k_prompt_records, dim3(grid), dim3(256), 0, st, (scope_rec*)out, n, capacity, bias, n_bias, first, index_offset, count_out);
}

// items == nullptr: the n haystacks from `first`; else the candidate set (n_ptr: its count on the device, n = the room that bounds it,
// hint = what the host knows of its length - the grid's bound, not the loop's).  tags == nullptr: no active scope.  bitmap: 16 words per
// 1024 items of n, tile_counts: one word per 1024 (16-byte aligned).  count_out: (written, visible).
void fzb_launch_prompt_compact(const u32* items, const u32* n_ptr, u32 n, u32 hint, const uint16_t* tags, u64 n_tags, const int16_t* bias, u64 n_bias, u64 first, u32 index_offset,
                               u32 require, u32 exclude, u64* bitmap, u32* tile_counts, fzb_match_rec* out, u32 capacity, u32* count_out, int grid_max, hipStream_t st) {
    const int grid = tc_grid(((u64)(hint < n ? hint : n) + SCOPE_TILE - 1) / SCOPE_TILE, grid_max);
    FZB_LAUNCH(k_prompt_flag, dim3(grid), dim3(256), 0, st, items, n_ptr, n, n, tags, n_tags, first, require, exclude, bitmap, tile_counts);
    FZB_LAUNCH(k_prompt_compact, dim3(grid), dim3(256), 0, st, (const u64*)bitmap, (const u32*)tile_counts, items, n_ptr, n, n, bias, n_bias, first, index_offset, (scope_rec*)out,
               capacity, count_out);
}
