// gfx950 kernels, the selection stage of the top-`limit` queries (between the scorers and the ordering step, kernels_sort.hip).
//
// The reference has no such call: `match_list` returns every match and the caller truncates (src/matcher/mod.rs:215-221 reverse +
// src/sort.rs:6-40 stable radix sort).  This stage keeps, in record order, exactly the records that make up the first `limit` entries of
// that list (topk_select.h says which), so the reverse / stable sort that follows only sees `limit` records:
//   1. histogram of the scores: 256 bins of the low byte when every score is below 256 (OrderPlan::one_pass), otherwise TWO LEVELS - the
//      high byte over all records, then the low byte over the records of the high byte's bucket; per-workgroup histograms in LDS, one
//      atomic per non-empty bin and workgroup to HBM;
//   2. the cut (threshold T, number of ties kept) from the bins - one small workgroup, result in device memory;
//   3. per-tile counts of "above T" / "equal T" records, their exclusive scan, and a stable scatter (ranks inside a wave from ballots,
//      waves and 256-record slabs ordered through running counters - the shape of the radix pass).
// IndexAsc / IndexDesc: no histogram, the first / last `limit` records are copied.  found <= limit: every kernel reads the count and
// returns, the scatter is a plain copy.  The record count lives in device memory; grids are sized by the caller from the capacity.
#include "kernels_common.h"
#include "topk_select.h"
#include "score_bias.h"
#include "scope.h"
#include "facets.h"

#define TOPK_TILE 2048
// scratch layout (u32 words; the caller hands in the radix sort's histogram buffer, idle until the ordering step):
//   [0, 256) bins of the high byte   [256, 512) bins of the low byte   [512, 528) state   [528 + k * ntiles_cap ...) k = 0: tile counts
//   above T, 1: tile counts equal T, 2 / 3: their exclusive scans
#define TOPK_BINS_HI 0
#define TOPK_BINS_LO 256
#define TOPK_STATE 512
#define TOPK_TILES 528
// state words
#define TS_HI_BIN 0
#define TS_ABOVE_HI 1
#define TS_T 2
#define TS_GT 3
#define TS_TIES 4
#define TS_QUOTA 5
#define TS_LO 6
#define TS_KEEP_ALL 7

__device__ __forceinline__ u32 topk_count(const u32* __restrict__ in_count, u32 in_cap) { return min(in_count[0], in_cap); }

__device__ __forceinline__ TopkCut topk_load_cut(const u32* __restrict__ scratch) {
    const u32* s = scratch + TOPK_STATE;
    TopkCut c;
    c.T = s[TS_T]; c.gt = s[TS_GT]; c.ties = s[TS_TIES]; c.quota = s[TS_QUOTA]; c.lo = s[TS_LO]; c.keep_all = s[TS_KEEP_ALL];
    return c;
}

// level 0: bins of score >> 8 over all records; level 1: bins of score & 255 over the records whose high byte is the picked one
// (fixed_hi >= 0: known on the host - every score is below 256)
__global__ __launch_bounds__(256) void k_topk_hist(const fzb_match_rec* __restrict__ in, const u32* __restrict__ in_count, u32 in_cap, u32 limit, int level, int fixed_hi,
                                                   u32* __restrict__ scratch) {
    __shared__ u32 h[256];
    const u32 n = topk_count(in_count, in_cap);
    if (n <= limit || limit == 0) return;  // nothing to remove / nothing to keep: no threshold needed
    const u32 hi_bin = level == 0 ? 0u : fixed_hi >= 0 ? (u32)fixed_hi : scratch[TOPK_STATE + TS_HI_BIN];
    h[threadIdx.x] = 0;
    __syncthreads();
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const u32 s = in[i].score;
        if (level == 0) atomicAdd(&h[s >> 8], 1u);
        else if ((s >> 8) == hi_bin) atomicAdd(&h[s & 255u], 1u);
    }
    __syncthreads();
    const u32 c = h[threadIdx.x];
    if (c) atomicAdd(&scratch[(level == 0 ? TOPK_BINS_HI : TOPK_BINS_LO) + threadIdx.x], c);
}

// step 0: the high byte's bucket from its bins; step 1: the cut.  One workgroup; the bins are staged in LDS and one thread walks them
// with the functions the host tests fuzz.
__global__ __launch_bounds__(256) void k_topk_cut(const u32* __restrict__ in_count, u32 in_cap, u32 limit, int step, int by_score, int desc, int fixed_hi, u32* __restrict__ scratch) {
    __shared__ u32 bins[256];
    const u32 n = topk_count(in_count, in_cap);
    u32* const s = scratch + TOPK_STATE;
    const bool trivial = n <= limit || limit == 0 || !by_score;
    if (!trivial) bins[threadIdx.x] = scratch[(step == 0 ? TOPK_BINS_HI : TOPK_BINS_LO) + threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (step == 0) {
        u32 above = 0, b = 0;
        if (!trivial) b = topk_pick_bin(bins, limit, &above);
        s[TS_HI_BIN] = b;
        s[TS_ABOVE_HI] = above;
        return;
    }
    TopkCut c;
    if (n <= limit) c = topk_cut_keep_all(n);
    else if (!by_score) c = topk_cut_by_index(n, limit, desc);
    else if (limit == 0) c = topk_cut_by_score(0, 0, bins, 0, desc);
    else c = topk_cut_by_score(fixed_hi >= 0 ? (u32)fixed_hi : s[TS_HI_BIN], fixed_hi >= 0 ? 0u : s[TS_ABOVE_HI], bins, limit, desc);
    s[TS_T] = c.T; s[TS_GT] = c.gt; s[TS_TIES] = c.ties; s[TS_QUOTA] = c.quota; s[TS_LO] = c.lo; s[TS_KEEP_ALL] = c.keep_all;
}

// per tile: records above T, records equal T
__global__ __launch_bounds__(256) void k_topk_tile_counts(const fzb_match_rec* __restrict__ in, const u32* __restrict__ in_count, u32 in_cap, u32* __restrict__ scratch, u32 ntiles_cap) {
    __shared__ u32 acc[2];
    const TopkCut c = topk_load_cut(scratch);
    if (c.keep_all) return;
    const u32 n = topk_count(in_count, in_cap);
    const u32 ntiles = min((n + TOPK_TILE - 1) / TOPK_TILE, ntiles_cap);
    u32* const cnt_gt = scratch + TOPK_TILES;
    u32* const cnt_eq = cnt_gt + ntiles_cap;
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (threadIdx.x < 2) acc[threadIdx.x] = 0;
        __syncthreads();
        const u32 lo = tile * TOPK_TILE, hi = min(lo + TOPK_TILE, n);
        u32 g = 0, e = 0;
        for (u32 i = lo + threadIdx.x; i < hi; i += 256) {
            const u32 s = in[i].score;
            g += s > c.T;
            e += s == c.T;
        }
        for (int off = 32; off > 0; off >>= 1) {
            g += __shfl_down(g, off);
            e += __shfl_down(e, off);
        }
        if (lane_id() == 0) {
            if (g) atomicAdd(&acc[0], g);
            if (e) atomicAdd(&acc[1], e);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            cnt_gt[tile] = acc[0];
            cnt_eq[tile] = acc[1];
        }
        __syncthreads();
    }
}

// exclusive scans of the two tile-count rows: one workgroup of two waves, a row each
__global__ __launch_bounds__(128) void k_topk_scan(const u32* __restrict__ in_count, u32 in_cap, u32* __restrict__ scratch, u32 ntiles_cap) {
    if (scratch[TOPK_STATE + TS_KEEP_ALL]) return;
    const u32 n = topk_count(in_count, in_cap);
    const u32 ntiles = min((n + TOPK_TILE - 1) / TOPK_TILE, ntiles_cap);
    const int row = threadIdx.x >> 6, lane = lane_id();
    const u32* const cnt = scratch + TOPK_TILES + (size_t)row * ntiles_cap;
    u32* const off = scratch + TOPK_TILES + (size_t)(2 + row) * ntiles_cap;
    u32 carry = 0;
    for (u32 t0 = 0; t0 < ntiles; t0 += 64) {  // uniform trip count: every lane takes part in the shuffles
        const u32 t = t0 + lane;
        const u32 v = t < ntiles ? cnt[t] : 0u;
        u32 incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const u32 x = __shfl_up(incl, o);
            if (lane >= o) incl += x;
        }
        if (t < ntiles) off[t] = carry + incl - v;
        carry += __shfl(incl, 63);
    }
}

// the stable compaction (by score), or the copy of a slice (by index / nothing to remove); writes the two result words
__global__ __launch_bounds__(256) void k_topk_scatter(const fzb_match_rec* __restrict__ in, const u32* __restrict__ in_count, u32 in_cap, int by_score, fzb_match_rec* __restrict__ out,
                                                      u32 out_cap, u32* __restrict__ out_count, const u32* __restrict__ scratch, u32 ntiles_cap) {
    __shared__ u32 wave_gt[4], wave_eq[4];
    __shared__ u32 run[2];
    const TopkCut c = topk_load_cut(scratch);
    const u32 n = topk_count(in_count, in_cap);
    const u32 kept = min(c.keep_all ? n : c.gt + c.quota, out_cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out_count[0] = kept;
        out_count[1] = in_count[1];  // matches found
    }
    if (c.keep_all || !by_score) {  // records lo .. lo + kept - 1, as they are
        const u32 first = c.keep_all ? 0u : c.lo;
        for (u32 j = blockIdx.x * 256u + threadIdx.x; j < kept; j += gridDim.x * 256u)
            if (first + j < n) out[j] = in[first + j];
        return;
    }
    const u32 ntiles = min((n + TOPK_TILE - 1) / TOPK_TILE, ntiles_cap);
    const u32* const off_gt = scratch + TOPK_TILES + (size_t)2 * ntiles_cap;
    const u32* const off_eq = off_gt + ntiles_cap;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 below = ((u64)1 << lane) - 1;
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tid == 0) {
            run[0] = off_gt[tile];
            run[1] = off_eq[tile];
        }
        const u32 lo = tile * TOPK_TILE, hi = min(lo + TOPK_TILE, n);
        for (u32 base = lo; base < hi; base += 256) {
            const u32 i = base + tid;
            const bool valid = i < hi;
            fzb_match_rec r;
            r.index = 0; r.score = 0; r.exact = 0; r.valid = 0;
            if (valid) r = in[i];
            const u64 bg = __ballot(valid && r.score > c.T);
            const u64 be = __ballot(valid && r.score == c.T);
            if (lane == 0) {
                wave_gt[wave] = __popcll(bg);
                wave_eq[wave] = __popcll(be);
            }
            __syncthreads();
            u32 gt_before = run[0] + __popcll(bg & below), eq_before = run[1] + __popcll(be & below);
            u32 all_gt = 0, all_eq = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                if (w < wave) {
                    gt_before += wave_gt[w];
                    eq_before += wave_eq[w];
                }
                all_gt += wave_gt[w];
                all_eq += wave_eq[w];
            }
            if (valid) {
                const u32 d = topk_dest(c, 1, r.score, gt_before, eq_before);
                if (d != TOPK_NOT_KEPT && d < kept) out[d] = r;
            }
            __syncthreads();
            if (tid == 0) {
                run[0] += all_gt;
                run[1] += all_eq;
            }
            __syncthreads();
        }
    }
}

// Selected runs of contiguous shards -> one index-ordered list (the sharded top query's root): k_concat_runs for runs whose count pair is
// (records kept, matches found) - a run is never "cut", and the found words are summed.  total_out[0] = records, [1] = matches found.
__global__ __launch_bounds__(256) void k_topk_concat(RunSet rs, const u32* __restrict__ base_in, u32* __restrict__ total_out, fzb_match_rec* __restrict__ out, u32 capacity) {
    __shared__ u32 pre[FZB_MAX_RUNS + 1];
    __shared__ u32 found_s;
    const int tid = threadIdx.x;
    if (tid < 64) {
        const u32 c = tid < rs.n ? min(rs.count[tid][0], rs.cap[tid]) : 0u;
        u32 f = tid < rs.n ? rs.count[tid][1] : 0u;
        u32 incl = c;
        for (int off = 1; off < 64; off <<= 1) {
            const u32 t = __shfl_up(incl, off);
            if (tid >= off) incl += t;
        }
        for (int off = 32; off > 0; off >>= 1) f += __shfl_down(f, off);
        pre[tid + 1] = incl;
        if (tid == 0) {
            pre[0] = 0;
            found_s = f;
        }
    }
    __syncthreads();
    const u32 base = base_in ? base_in[0] : 0u;
    const u32 total = pre[rs.n];
    for (u32 i = blockIdx.x * 256u + tid; i < total; i += gridDim.x * 256u) {
        int lo = 0, hi = rs.n - 1;  // last run whose prefix is <= i
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (pre[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        if (base + i < capacity) out[base + i] = rs.run[lo][i - pre[lo]];
    }
    if (blockIdx.x == 0 && tid == 0) {
        total_out[0] = min(base + total, capacity);
        total_out[1] = (base_in ? base_in[1] : 0u) + found_s;
    }
}

void fzb_launch_topk_concat(const RunSet& rs, const u32* base_in, u32* total_out, fzb_match_rec* out, u32 capacity, int grid, hipStream_t st) {
    FZB_LAUNCH(k_topk_concat, dim3(grid), dim3(256), 0, st, rs, base_in, total_out, out, capacity);
}

// in: *in_count records (at most in_cap) in record order, in_count[1] = matches found.  out: the kept records in record order,
// out_count[0] = their number = min(limit, records), out_count[1] = matches found.  `scratch`: the radix sort's histogram buffer for
// >= in_cap records (ntiles_cap = its tile capacity); free again when the last kernel has run.  in and out must not overlap.  Returns the first
// error of the fill or the launches.
hipError_t fzb_launch_topk_select(const fzb_match_rec* in, const u32* in_count, u32 in_cap, u32 limit, int by_score, int desc, int one_pass, fzb_match_rec* out, u32 out_cap,
                            u32* out_count, u32* scratch, u32 ntiles_cap, int grid, hipStream_t st) {
    const int fixed_hi = one_pass ? 0 : -1;
    if (by_score) {
        const hipError_t e = hipMemsetAsync(scratch, 0, 512 * sizeof(u32), st);
        if (e != hipSuccess) return e;  // (nothing launched: the bins would hold the previous query's counts)
        if (!one_pass) {
            FZB_LAUNCH(k_topk_hist, dim3(grid), dim3(256), 0, st, in, in_count, in_cap, limit, 0, fixed_hi, scratch);
            FZB_LAUNCH(k_topk_cut, dim3(1), dim3(256), 0, st, in_count, in_cap, limit, 0, by_score, desc, fixed_hi, scratch);
        }
        FZB_LAUNCH(k_topk_hist, dim3(grid), dim3(256), 0, st, in, in_count, in_cap, limit, 1, fixed_hi, scratch);
    }
    FZB_LAUNCH(k_topk_cut, dim3(1), dim3(256), 0, st, in_count, in_cap, limit, 1, by_score, desc, fixed_hi, scratch);
    if (by_score) {
        FZB_LAUNCH(k_topk_tile_counts, dim3(grid), dim3(256), 0, st, in, in_count, in_cap, scratch, ntiles_cap);
        FZB_LAUNCH(k_topk_scan, dim3(1), dim3(128), 0, st, in_count, in_cap, scratch, ntiles_cap);
    }
    FZB_LAUNCH(k_topk_scatter, dim3(grid), dim3(256), 0, st, in, in_count, in_cap, by_score, out, out_cap, out_count, scratch, ntiles_cap);
    return hipGetLastError();
}

// ---- the corpus' per-haystack score bias (score_bias.h) ----------------------------------------------------------------------------
// Between the scorers and the selection / ordering stage: record k of an index-ordered run belongs to haystack
// first + (index - index_offset) of the corpus, and its score becomes clamp(score + bias[haystack], 0, 65535).  One thread per record,
// grid-stride; the whole 8-byte record is loaded and stored back (two dwords where the caller's array is only 4-byte aligned); the records
// come in index order, so the 2-byte gather is near-coalesced.  A record whose haystack lies outside the n_bias entries is left alone.
__global__ __launch_bounds__(256) void k_bias_apply(fzb_match_rec* __restrict__ recs, const u32* __restrict__ count, u32 cap, const int16_t* __restrict__ bias, u64 n_bias, u64 first,
                                                    u32 index_offset) {
    const u32 n = min(count[0], cap);
    const bool wide = ((uintptr_t)recs & 7u) == 0;
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        uint2 w;
        if (wide) w = *(const uint2*)(recs + i);
        else w = make_uint2(((const u32*)(recs + i))[0], ((const u32*)(recs + i))[1]);
        const u64 h = first + (u64)(w.x - index_offset);
        if (h >= n_bias) continue;
        w.y = (w.y & 0xFFFF0000u) | sbias_clamp_add(w.y & 0xFFFFu, (int32_t)bias[h]);
        if (wide) *(uint2*)(recs + i) = w;
        else ((u32*)(recs + i))[1] = w.y;
    }
}

// recs: up to `cap` index-ordered records, count[0] of them written; bias: the corpus' array of n_bias entries.  The grid is sized from
// the capacity here and trimmed by the device-side count in the kernel.
void fzb_launch_bias_apply(fzb_match_rec* recs, const u32* count, u32 cap, const int16_t* bias, u64 n_bias, u64 first, u32 index_offset, int grid_max, hipStream_t st) {
    if (!cap || !n_bias) return;
    const int grid = tc_grid((cap + 255u) / 256u, grid_max);
    FZB_LAUNCH(k_bias_apply, dim3(grid), dim3(256), 0, st, recs, count, cap, bias, n_bias, first, index_offset);
}

// ---- the corpus' visibility scope (scope.h): hidden haystacks' records are dropped ----------------------------------------------------
// Between the scorers (or the multi-pattern composition) and the bias / selection / ordering stage: `recs` holds count[0] index-ordered
// records (never truncated: the producer's scratch has room for one per haystack), record k belongs to haystack
// first + (index - index_offset), whose 2-byte tag is gathered - near-coalesced, the records come in index order.  Two launches, both
// sized on the host from the capacity and trimmed by the device-side count; the kept records go to a DIFFERENT buffer.
static_assert(SCOPE_TILE == FZB_TILE && sizeof(scope_rec) == sizeof(fzb_match_rec) && alignof(scope_rec) == alignof(fzb_match_rec), "the drop pass moves fzb_match_rec by the tile");

// the flag pass (tile_compact.h): 2-byte tag gathered per record.  FACETS: the tag facets of the records (facets.h) ride in the same pass -
// the tag is in a register here, so a sink attached to the matcher costs no second pass over the records under an active scope; the
// instantiation without a sink is the pass as it was.
template <bool FACETS>
__device__ __forceinline__ void scope_flag_pass(const scope_rec* __restrict__ recs, const u32* __restrict__ count, u32 cap, const uint16_t* __restrict__ tags, u64 n_tags, u64 first,
                                                u32 index_offset, u32 require, u32 exclude, u64* __restrict__ bitmap, u32* __restrict__ tile_counts, u32* __restrict__ facets) {
    const u32 n = min(count[0], cap);
    if constexpr (!FACETS) {
        tc_flag_pass(n, bitmap, tile_counts, [&](u32 tile, u32 slot) { return scope_tile_keeps(recs, n, tile, slot, tags, n_tags, first, index_offset, require, exclude); });
    } else {
        facet_acc acc;
        facets_clear(acc);
        tc_flag_pass(n, bitmap, tile_counts, [&](u32 tile, u32 slot) {
            const u64 j = (u64)tile * SCOPE_TILE + slot;
            const bool valid = j < n;
            const u32 tag = valid ? scope_tag_of(tags, n_tags, first, index_offset, recs[j].index) : 0u;
            facets_wave_step(acc, valid, tag, require, exclude);
            return facet_visible(valid, tag, require, exclude);
        });
        facets_publish(acc, facets);
    }
}
__global__ __launch_bounds__(256) void k_scope_flag(const scope_rec* __restrict__ recs, const u32* __restrict__ count, u32 cap, const uint16_t* __restrict__ tags, u64 n_tags, u64 first,
                                                    u32 index_offset, u32 require, u32 exclude, u64* __restrict__ bitmap, u32* __restrict__ tile_counts) {
    scope_flag_pass<false>(recs, count, cap, tags, n_tags, first, index_offset, require, exclude, bitmap, tile_counts, nullptr);
}
__global__ __launch_bounds__(256) void k_scope_flag_facets(const scope_rec* __restrict__ recs, const u32* __restrict__ count, u32 cap, const uint16_t* __restrict__ tags, u64 n_tags,
                                                           u64 first, u32 index_offset, u32 require, u32 exclude, u64* __restrict__ bitmap, u32* __restrict__ tile_counts,
                                                           u32* __restrict__ facets) {
    scope_flag_pass<true>(recs, count, cap, tags, n_tags, first, index_offset, require, exclude, bitmap, tile_counts, facets);
}

// The compaction: tile_compact.h's record compaction with a bounded destination (scope_store) and the (written, found) pair (scope_counts).
__global__ __launch_bounds__(256) void k_scope_compact(const u64* __restrict__ bitmap, const u32* __restrict__ counts, const u32* __restrict__ n_ptr, u32 in_cap,
                                                       const scope_rec* __restrict__ in, scope_rec* __restrict__ out, u32 capacity, u32* __restrict__ count_out) {
    const u32 kept = tc_compact_items(bitmap, counts, min(*n_ptr, in_cap), [&](u32 place, u64 j) { scope_store(out, capacity, place, in, j); });
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) scope_counts(kept, capacity, count_out);
}

// recs: count[0] index-ordered records (at most `cap`); out: room for `capacity`; count_out: (written, found).  bitmap: 16 words per tile of
// cap records, tile_counts: one word per tile.  facets != nullptr: the flag pass also counts the records' tag facets into that block
// (cleared in stream order by the caller); tags may then be null (n_tags 0: every tag 0).
void fzb_launch_scope_drop(const fzb_match_rec* recs, const u32* count, u32 cap, const uint16_t* tags, u64 n_tags, u64 first, u32 index_offset, u32 require, u32 exclude, u64* bitmap,
                           u32* tile_counts, fzb_match_rec* out, u32 capacity, u32* count_out, int grid_max, hipStream_t st, u32* facets) {
    const int grid = tc_grid((cap + SCOPE_TILE - 1) / SCOPE_TILE, grid_max);
    if (facets)
        FZB_LAUNCH(k_scope_flag_facets, dim3(grid), dim3(256), 0, st, (const scope_rec*)recs, count, cap, tags, tags ? n_tags : 0, first, index_offset, require, exclude, bitmap, tile_counts,
                   facets);
    else FZB_LAUNCH(k_scope_flag, dim3(grid), dim3(256), 0, st, (const scope_rec*)recs, count, cap, tags, n_tags, first, index_offset, require, exclude, bitmap, tile_counts);
    FZB_LAUNCH(k_scope_compact, dim3(grid), dim3(256), 0, st, (const u64*)bitmap, (const u32*)tile_counts, count, cap, (const scope_rec*)recs, (scope_rec*)out, capacity, count_out);
}
