// gfx950 kernels, the glue of the fused "top + matched positions" query (fzb_match_list_top_indices*): between the top stage's ordering
// step and the traced pipeline, and behind the traced pipeline.
//
// The reference has no such call: its caller truncates what `Matcher::match_list_indices` returns (src/matcher/mod.rs:234-275).  Here the
// sorted head of the top stage stays in HBM; k_top_items turns it into the item list (+ its length word) of the traced second pass, and
// the pack kernels turn that pass' strided positions into the caller's dense array (indices_pack.h says how) while holding every traced
// record to the head's record at its place.  Nothing is read back in between; the record count lives in device memory and the grids are
// sized by the caller from min(limit, haystacks).
//   * a head of up to IPACK_TILE records - the picker's case - is packed by ONE launch of one workgroup: every thread scans its share of
//     IPACK_SHARE consecutive records, the shares are scanned across the wave with shuffles and across the four waves through LDS, the
//     records are written, and then the threads walk the tile's DENSE positions (thread t takes position t, t + 256, ..: the stores are
//     coalesced, the loads are runs of one record's positions), finding each position's record by bisection of the begins kept in LDS;
//   * a longer head takes three launches, as the selection stage does (kernels_topk.hip): per-tile sums, their exclusive scan (one wave),
//     and the same scatter kernel with every tile starting at its scanned base.  No workgroup waits for another one, nothing is ordered by
//     an atomic.
// The multi-pattern form (fzb_multi_match_list_top_indices_device) traces every positive pattern over the one item list and puts a step
// between those passes and the pack: k_multi_union merges the patterns' records and positions per head record (indices_union.h says how),
// and the pack then sees one traced pass with a stride of U.  A matcher that has an any-of group (fzb_multi_match_list_top_indices_groups*)
// takes the k_gunion_* launches in that place: an alternative's traced pass returns only the head items it matches, so its rows are found
// first, and only each group's carrier contributes positions (indices_union_groups.h says how).
#include "kernels_common.h"
#include "indices_pack.h"
#include "indices_union.h"
#include "indices_union_groups.h"

#define IPACK_THREADS (IPACK_TILE / IPACK_SHARE)
static_assert(IPACK_THREADS == 256, "four waves scan a tile");

struct PackArgs {
    const fzb_match_rec* head;     // the sorted head and its pair (records, matches found)
    const u32* head_count;
    const fzb_match_rec* traced;   // the traced pass' records in item order and its pair
    const u32* traced_count;
    const u32* npos;               // per traced record: positions found; its positions at pos[k * stride ..]
    const u32* pos;
    u32 stride;
    fzb_indices_rec* out;          // the packed records, the dense positions, the four result words
    u32 out_cap;
    u32* dense;
    u32 dense_cap;
    u32* dev_count;
    u32* tiles;                    // [0, ntiles_cap) tile sums, [ntiles_cap, 2 ntiles_cap) their exclusive scan (heads beyond one tile)
    u32 ntiles_cap;
};

__device__ __forceinline__ u32 ipack_count(const PackArgs& a) { return min(a.head_count[0], a.out_cap); }

// exclusive scan of one value per thread over the workgroup (four waves); *total = the workgroup's sum.  Two barriers.
__device__ __forceinline__ u32 ipack_block_scan(u32 v, u32* s_wave, u32* total) {
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    u32 incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const u32 x = __shfl_up(incl, o);
        if (lane >= o) incl += x;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    u32 before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < IPACK_THREADS / 64; w++) {
        if (w < wave) before += s_wave[w];
        all += s_wave[w];
    }
    __syncthreads();  // (s_wave is written again by the next tile)
    *total = all;
    return before + incl - v;
}

// the head's corpus indices in head order + their number: the item list of the traced pass.  Clears the two result words the pack
// kernels only ever raise (positions written, inconsistency).
__global__ __launch_bounds__(256) void k_top_items(const fzb_match_rec* __restrict__ head, const u32* __restrict__ head_count, u32 cap, u32* __restrict__ items,
                                                   u32* __restrict__ n_items, u32* __restrict__ dev_count) {
    const u32 n = min(head_count[0], cap);
    for (u32 j = blockIdx.x * 256u + threadIdx.x; j < n; j += gridDim.x * 256u) items[j] = head[j].index;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        n_items[0] = n;
        dev_count[2] = 0;
        dev_count[3] = 0;
    }
}

// heads beyond one tile, first launch: positions per tile
__global__ __launch_bounds__(IPACK_THREADS) void k_ipack_tile_sums(const PackArgs a) {
    __shared__ u32 s_wave[IPACK_THREADS / 64];
    const u32 n = ipack_count(a);
    const u32 ntiles = min(ipack_ntiles(n), a.ntiles_cap);
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        u32 lo, hi;
        ipack_tile_range(tile, n, &lo, &hi);
        const u32 first = min(lo + threadIdx.x * IPACK_SHARE, hi);
        u32 begins[IPACK_SHARE];
        const u32 mine = ipack_scan_share(a.npos, first, min(hi - first, (u32)IPACK_SHARE), a.stride, begins);
        u32 total;
        (void)ipack_block_scan(mine, s_wave, &total);
        if (threadIdx.x == 0) a.tiles[tile] = total;
    }
}

// second launch: exclusive scan of the tile sums (one wave); the grand total is the number of position dwords
__global__ __launch_bounds__(64) void k_ipack_scan_tiles(const PackArgs a) {
    const u32 n = ipack_count(a);
    const u32 ntiles = min(ipack_ntiles(n), a.ntiles_cap);
    const int lane = lane_id();
    u32 carry = 0;
    for (u32 t0 = 0; t0 < ntiles; t0 += 64) {  // uniform trip count: every lane takes part in the shuffles
        const u32 t = t0 + lane;
        const u32 v = t < ntiles ? a.tiles[t] : 0u;
        u32 incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const u32 x = __shfl_up(incl, o);
            if (lane >= o) incl += x;
        }
        if (t < ntiles) a.tiles[a.ntiles_cap + t] = carry + incl - v;
        carry += __shfl(incl, 63);
    }
    if (lane == 0) a.dev_count[2] = min(carry, a.dense_cap);
}

// the scan inside a tile, the records, the gather of the positions and the check against the head.  MULTI: the tile's base comes from
// the scanned tile sums; otherwise there is one tile, its base is 0 and its total is the result's.
template <bool MULTI>
__global__ __launch_bounds__(IPACK_THREADS) void k_ipack_scatter(const PackArgs a) {
    __shared__ u32 s_begin[IPACK_TILE];
    __shared__ u32 s_wave[IPACK_THREADS / 64];
    const u32 n = ipack_count(a);
    const u32 ntiles = min(ipack_ntiles(n), MULTI ? a.ntiles_cap : 1u);
    u32 bad = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.dev_count[0] = n;
        a.dev_count[1] = a.head_count[1];  // matches found
        bad |= ipack_check_count(a.head_count[0], a.traced_count[0]);
    }
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        u32 lo, hi;
        ipack_tile_range(tile, n, &lo, &hi);
        const u32 first = min(lo + threadIdx.x * IPACK_SHARE, hi);
        const u32 cnt = min(hi - first, (u32)IPACK_SHARE);
        u32 begins[IPACK_SHARE];
        const u32 mine = ipack_scan_share(a.npos, first, cnt, a.stride, begins);
        u32 total;
        const u32 before = ipack_block_scan(mine, s_wave, &total);
        const u32 base = MULTI ? a.tiles[a.ntiles_cap + tile] : 0u;
#pragma unroll
        for (u32 r = 0; r < IPACK_SHARE; r++) {
            if (r >= cnt) break;
            const u32 k = first + r;
            const fzb_match_rec h = a.head[k], t = a.traced[k];
            bad |= ipack_check_record(h.index, h.score, h.exact, t.index, t.score, t.exact);
            s_begin[k - lo] = before + begins[r];
            fzb_indices_rec o;
            o.index = h.index;
            o.score = h.score;
            o.exact = h.exact;
            o._pad = 0;
            o.positions_begin = base + before + begins[r];
            o.positions_len = ipack_len(a.npos[k], a.stride);
            a.out[k] = o;
        }
        __syncthreads();
        for (u32 d = threadIdx.x; d < total; d += IPACK_THREADS) {
            const u32 r = ipack_find_record(s_begin, hi - lo, d);
            if (base + d < a.dense_cap) a.dense[base + d] = a.pos[(size_t)(lo + r) * a.stride + (d - s_begin[r])];
        }
        if (!MULTI && threadIdx.x == 0) a.dev_count[2] = min(total, a.dense_cap);
        __syncthreads();  // (s_begin is written again by the next tile)
    }
    if (bad) a.dev_count[3] = bad;  // (k_top_items cleared it; every writer stores a non-zero word)
}

static_assert(sizeof(IUnionRec) == sizeof(fzb_match_rec) && offsetof(IUnionRec, score) == offsetof(fzb_match_rec, score) && offsetof(IUnionRec, exact) == offsetof(fzb_match_rec, exact),
              "indices_union.h reads and writes fzb_match_rec");

struct UnionArgs {
    const fzb_match_rec* head;  // the sorted head, its pair (records, matches found) and the records it has room for
    const u32* head_count;
    u32 cap;
    u32 P;                      // positive patterns
    IUnionSrc src[IUNION_BY_VALUE];  // their traced passes (P <= IUNION_BY_VALUE) ..
    const IUnionSrc* more;      // .. or all P of them in device memory, with P cursors per record of the head
    u32* cursors;
    fzb_match_rec* out;         // the combined records and their pair; per record the union's length and, at pos_u[k * U ..], the union
    u32* out_count;
    u32* npos_u;
    u32* pos_u;
    u32 U;
};

// One thread per head record: a few dependent loads per position, no reuse between threads - latency-bound glue between the traced passes and
// the pack.  BY_VALUE: the sources are read from the argument block (wave-uniform scalar loads) and the cursors are the thread's own.
template <bool BY_VALUE>
__global__ __launch_bounds__(256) void k_multi_union(const UnionArgs a) {
    const u32 n = min(a.head_count[0], a.cap);
    const IUnionSrc* const src = BY_VALUE ? a.src : a.more;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.out_count[0] = iunion_count(src, a.P, a.head_count[0]);
        a.out_count[1] = a.head_count[1];
    }
    for (u32 k = blockIdx.x * 256u + threadIdx.x; k < n; k += gridDim.x * 256u) {
        const IUnionRec r = iunion_record(src, a.P, k, a.head[k].index);
        fzb_match_rec o;
        o.index = r.index;
        o.score = r.score;
        o.exact = r.exact;
        o.valid = 0;
        a.out[k] = o;
        u32 own[IUNION_BY_VALUE];
        u32* const cur = BY_VALUE ? own : a.cursors + (size_t)k * a.P;
        a.npos_u[k] = iunion_merge(src, a.P, k, cur, a.pos_u + (size_t)k * a.U, a.U);
    }
}

// src: P sources in host memory (copied into the argument block while P <= IUNION_BY_VALUE); src_dev / cursors: the same P sources and
// max_records x P words in device memory, read only beyond that
void fzb_launch_multi_union(const fzb_match_rec* head, const u32* head_count, u32 max_records, const IUnionSrc* src, u32 P, const IUnionSrc* src_dev, u32* cursors, fzb_match_rec* out,
                            u32* out_count, u32* npos_u, u32* pos_u, u32 U, int grid, hipStream_t st) {
    UnionArgs a{};
    a.head = head;
    a.head_count = head_count;
    a.cap = max_records;
    a.P = P;
    const bool by_value = P <= IUNION_BY_VALUE;
    for (u32 p = 0; by_value && p < P; p++) a.src[p] = src[p];
    a.more = src_dev;
    a.cursors = cursors;
    a.out = out;
    a.out_count = out_count;
    a.npos_u = npos_u;
    a.pos_u = pos_u;
    a.U = U;
    const int g = (int)std::max<u32>(1, std::min<u32>((u32)grid, (max_records + 255) / 256));
    if (by_value) FZB_LAUNCH((k_multi_union<true>), dim3(g), dim3(256), 0, st, a);
    else FZB_LAUNCH((k_multi_union<false>), dim3(g), dim3(256), 0, st, a);
}

// ---- the union of a matcher that has an any-of group (indices_union_groups.h) --------------------------------------------------------------
// An alternative's traced pass over the head's items returns only the items it matches, so its row of head record k has to be found:
//   k_gunion_slots  slot[head[k].index] = k - one word per haystack of the corpus, never cleared: it is read only at the indices of traced
//                   records, and those are head items, which this launch wrote;
//   k_gunion_clear  all the alternatives' `where` arrays at once (16-byte stores);
//   k_gunion_where  for traced record j of alternative a: where_a[slot[rec_a[j].index]] = j + 1 - one launch for all alternatives;
//   k_gunion_merge  k_multi_union's step with the carrier rule: one thread per head record.
// The same class as k_multi_union: latency-bound glue over at most `limit` records, dependent loads and no reuse.
struct GUnionArgs {
    const fzb_match_rec* head;
    const u32* head_count;
    u32 cap;
    u32 P;                           // sources: plain positive patterns and alternatives, the sources of a term adjacent
    GUnionSrc src[IUNION_BY_VALUE];  // P <= IUNION_BY_VALUE ..
    const GUnionSrc* more;           // .. or all P in device memory, with 3 P scratch words per record of the head (carriers, rows, cursors)
    u32* scratch;
    const u32* slots;                // haystack -> head position (k_gunion_where)
    u32 n_hay;
    fzb_match_rec* out;
    u32* out_count;
    u32* npos_u;
    u32* pos_u;
    u32 U;
};

__global__ __launch_bounds__(256) void k_gunion_slots(const fzb_match_rec* __restrict__ head, const u32* __restrict__ head_count, u32 cap, u32* __restrict__ slots, u32 n_hay) {
    const u32 n = min(head_count[0], cap);
    for (u32 k = blockIdx.x * 256u + threadIdx.x; k < n; k += gridDim.x * 256u) {
        const u32 h = head[k].index;
        if (h < n_hay) slots[h] = k;
    }
}

__global__ __launch_bounds__(256) void k_gunion_clear(uint4* __restrict__ where4, u32 n4) {
    for (u32 j = blockIdx.x * 256u + threadIdx.x; j < n4; j += gridDim.x * 256u) where4[j] = make_uint4(0, 0, 0, 0);
}

// A traced record whose haystack is not the head record its slot names (cannot happen: the pass ran over the head's items) is dropped, never
// written out of bounds: the alternative then counts as absent there.
template <bool BY_VALUE>
__global__ __launch_bounds__(256) void k_gunion_where(const GUnionArgs a) {
    const GUnionSrc* const src = BY_VALUE ? a.src : a.more;
    const u32 n = min(a.head_count[0], a.cap);
    const u64 total = (u64)a.P * a.cap;
    for (u64 t = (u64)blockIdx.x * 256u + threadIdx.x; t < total; t += (u64)gridDim.x * 256u) {
        const u32 p = (u32)(t / a.cap), j = (u32)(t % a.cap);
        u32* const where = const_cast<u32*>(src[p].where);
        if (!where || j >= min(src[p].s.count[0], a.cap)) continue;
        const u32 h = src[p].s.rec[j].index;
        if (h >= a.n_hay) continue;
        const u32 k = a.slots[h];
        if (k < n && a.head[k].index == h) where[k] = j + 1;
    }
}

template <bool BY_VALUE>
__global__ __launch_bounds__(256) void k_gunion_merge(const GUnionArgs a) {
    const u32 n = min(a.head_count[0], a.cap);
    const GUnionSrc* const src = BY_VALUE ? a.src : a.more;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.out_count[0] = gunion_count(src, a.P, a.head_count[0]);
        a.out_count[1] = a.head_count[1];
    }
    for (u32 k = blockIdx.x * 256u + threadIdx.x; k < n; k += gridDim.x * 256u) {
        u32 own[3 * IUNION_BY_VALUE];
        u32* const carrier = BY_VALUE ? own : a.scratch + (size_t)k * 3u * a.P;
        u32* const row = carrier + (BY_VALUE ? IUNION_BY_VALUE : a.P);
        u32* const cur = row + (BY_VALUE ? IUNION_BY_VALUE : a.P);
        bool missing = false;
        const u32 T = gunion_carriers(src, a.P, k, carrier, row, &missing);
        const IUnionRec r = gunion_record_of(src, T, carrier, row, missing, a.head[k].index);
        fzb_match_rec o;
        o.index = r.index;
        o.score = r.score;
        o.exact = r.exact;
        o.valid = 0;
        a.out[k] = o;
        a.npos_u[k] = gunion_merge(src, T, carrier, row, cur, a.pos_u + (size_t)k * a.U, a.U);
    }
}

// src: P sources in host memory (copied into the argument block while P <= IUNION_BY_VALUE); src_dev / scratch: the same P sources and
// max_records x 3 P words in device memory, read only beyond that.  where: the alternatives' maps, where_words of them (a multiple of four)
// in one array.  slots: n_hay words.
void fzb_launch_gunion(const fzb_match_rec* head, const u32* head_count, u32 max_records, const GUnionSrc* src, u32 P, const GUnionSrc* src_dev, u32* scratch, u32* slots, u32 n_hay,
                       u32* where, size_t where_words, fzb_match_rec* out, u32* out_count, u32* npos_u, u32* pos_u, u32 U, int grid, hipStream_t st) {
    GUnionArgs a{};
    a.head = head;
    a.head_count = head_count;
    a.cap = max_records;
    a.P = P;
    const bool by_value = P <= IUNION_BY_VALUE;
    for (u32 p = 0; by_value && p < P; p++) a.src[p] = src[p];
    a.more = src_dev;
    a.scratch = scratch;
    a.slots = slots;
    a.n_hay = n_hay;
    a.out = out;
    a.out_count = out_count;
    a.npos_u = npos_u;
    a.pos_u = pos_u;
    a.U = U;
    const auto blocks = [&](u64 work) { return (int)std::max<u64>(1, std::min<u64>((u64)grid, (work + 255) / 256)); };
    const int g = blocks(max_records);
    FZB_LAUNCH(k_gunion_slots, dim3(g), dim3(256), 0, st, head, head_count, max_records, slots, n_hay);
    FZB_LAUNCH(k_gunion_clear, dim3(blocks(where_words / 4)), dim3(256), 0, st, (uint4*)where, (u32)(where_words / 4));
    if (by_value) FZB_LAUNCH((k_gunion_where<true>), dim3(blocks((u64)P * max_records)), dim3(256), 0, st, a);
    else FZB_LAUNCH((k_gunion_where<false>), dim3(blocks((u64)P * max_records)), dim3(256), 0, st, a);
    if (by_value) FZB_LAUNCH((k_gunion_merge<true>), dim3(g), dim3(256), 0, st, a);
    else FZB_LAUNCH((k_gunion_merge<false>), dim3(g), dim3(256), 0, st, a);
}

void fzb_launch_top_items(const fzb_match_rec* head, const u32* head_count, u32 cap, u32* items, u32* n_items, u32* dev_count, int grid, hipStream_t st) {
    FZB_LAUNCH(k_top_items, dim3(grid), dim3(256), 0, st, head, head_count, cap, items, n_items, dev_count);
}

// u32 words of `tiles` the pack needs for heads of up to max_records records
size_t fzb_indices_pack_tile_words(size_t max_records) { return 2 * ((max_records + IPACK_TILE - 1) / IPACK_TILE + 1); }

// head / traced: max_records-record buffers with their count pairs; npos / pos: the traced pass' counts and strided positions.  out (room
// for out_cap >= max_records records), dense (dense_cap dwords) and dev_count (four words, [2] and [3] cleared by k_top_items) receive the
// result.  tiles: fzb_indices_pack_tile_words(max_records) words (not read for max_records <= IPACK_TILE).
void fzb_launch_indices_pack(const fzb_match_rec* head, const u32* head_count, const fzb_match_rec* traced, const u32* traced_count, const u32* npos, const u32* pos, u32 stride,
                             fzb_indices_rec* out, u32 out_cap, u32* dense, u32 dense_cap, u32* dev_count, u32* tiles, u32 max_records, int grid, hipStream_t st) {
    const u32 ntiles_cap = (max_records + IPACK_TILE - 1) / IPACK_TILE + 1;
    const PackArgs a{head, head_count, traced, traced_count, npos, pos, stride, out, std::min<u32>(out_cap, max_records), dense, dense_cap, dev_count, tiles, ntiles_cap};
    if (max_records <= IPACK_TILE) {
        FZB_LAUNCH((k_ipack_scatter<false>), dim3(1), dim3(IPACK_THREADS), 0, st, a);
        return;
    }
    const int g = (int)std::max<u32>(1, std::min<u32>((u32)grid, ntiles_cap));
    FZB_LAUNCH(k_ipack_tile_sums, dim3(g), dim3(IPACK_THREADS), 0, st, a);
    FZB_LAUNCH(k_ipack_scan_tiles, dim3(1), dim3(64), 0, st, a);
    FZB_LAUNCH((k_ipack_scatter<true>), dim3(g), dim3(IPACK_THREADS), 0, st, a);
}
