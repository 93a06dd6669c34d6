// The tile scheme: how every stage that drops items turns its decisions into an index-ordered list.  Stated once, used everywhere.
//   flag     one 64-bit word per 64 items (bit = the item is kept) and one kept count per 1024-item tile (tc_flag_pass);
//   run      workgroup b of a grid owns the contiguous tiles tc_run gives it, so that what lies in front of it is a prefix;
//   prefix   the kept items in front of the run = the sum of the earlier tiles' counts, re-derived by every workgroup (tc_prefix): the
//            array is small and L2-resident, and nothing is ordered between workgroups;
//   scan     the run's own counts, in batches of up to 256 tiles, into each tile's first place (tc_batch_scan);
//   rank     inside a tile a word's base is a 16-lane scan of the word popcounts (tc_scan16), inside a word a set bit's place is the
//            popcount below it (tc_rank64 / tc_rank32).
// No atomics between workgroups, no spin-waits, never in place.
//
// The first part is plain functions for the device AND the host (tests/kernel_host/tile_compact_host.cpp compiles them for the CPU and
// tests/test_tile_compact_host.py fuzzes them against numpy; scope.h, seg_list.h and score_bias.h build on them).  The second part, under
// __HIPCC__, is the workgroup-level code of the kernels: 256 threads, four waves.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FZB_TC_FN __host__ __device__ __forceinline__
#else
#define FZB_TC_FN inline
#endif

#define TC_TILE 1024  // items per tile (FZB_TILE, SCOPE_TILE)
#define TC_WORDS (TC_TILE / 64)
#define TC_BATCH 256  // tiles per batch of the scan: one per thread

// ---- run: tiles per run, and the run [*t0, *t1) of workgroup b (empty for the trailing workgroups when the grid does not divide ntiles).
// `per` travels separately because a producer and a consumer may have to agree on it (SegList::stride, seg_list.h).
FZB_TC_FN uint32_t tc_tiles_per_run(uint32_t ntiles, uint32_t grid) { return grid ? ntiles / grid + (ntiles % grid ? 1u : 0u) : 0u; }  // (no sum that could wrap)
FZB_TC_FN void tc_run(uint32_t ntiles, uint32_t per, uint32_t b, uint32_t* t0, uint32_t* t1) {
    const uint64_t lo = (uint64_t)b * per;
    *t0 = lo < ntiles ? (uint32_t)lo : ntiles;
    *t1 = lo + per < ntiles ? (uint32_t)(lo + per) : ntiles;
}

// ---- rank: the place of set bit `bit` of a decision word, `before` = kept items in front of the word
FZB_TC_FN uint32_t tc_rank64(uint32_t before, uint64_t word, uint32_t bit) { return before + (uint32_t)__builtin_popcountll(word & (((uint64_t)1 << bit) - 1)); }
FZB_TC_FN uint32_t tc_rank32(uint32_t before, uint32_t word, uint32_t bit) { return before + (uint32_t)__builtin_popcount(word & ((1u << bit) - 1u)); }

// ---- grid of a pass over `units` work units (tiles, 256-record blocks) under the caller's cap: at least one workgroup
FZB_TC_FN int tc_grid(uint64_t units, int grid_max) {
    const uint64_t most = grid_max > 0 ? (uint64_t)grid_max : 1u;
    return (int)(units < most ? (units ? units : 1u) : most);
}

#if defined(__HIPCC__)
// =====================================================================================================================================
// Workgroup-level code.  Every function here is called by ALL 256 threads of the workgroup with workgroup-uniform arguments.

// ---- flag: the grid-stride tile loop of a flag pass over n items.  keep(tile, slot) decides item tile * TC_TILE + slot (it tests the
// list's end itself); a ballot per wave and pass, lane 0 stores the word and accumulates, one LDS atomic per wave, thread 0 stores the
// tile's count.  ROLLED: the four passes of a tile stay a loop (`#pragma unroll 1`: predicates that are long loops themselves).
template <bool ROLLED = false, class Keep>
__device__ __forceinline__ void tc_flag_pass(uint32_t n, uint64_t* __restrict__ bitmap, uint32_t* __restrict__ tile_counts, Keep keep) {
    __shared__ uint32_t s_cnt;
    const uint32_t ntiles = (n + TC_TILE - 1) / TC_TILE;
    const uint32_t tid = threadIdx.x;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        uint32_t cnt = 0;
        auto pass = [&](uint32_t p) {
            const uint64_t b = __ballot(keep(tile, p * 256u + tid));
            if ((tid & 63u) == 0) {
                bitmap[(uint64_t)tile * TC_WORDS + p * 4u + (tid >> 6)] = b;
                cnt += (uint32_t)__popcll(b);
            }
        };
        if constexpr (ROLLED) {
#pragma unroll 1
            for (uint32_t p = 0; p < TC_TILE / 256; p++) pass(p);
        } else {
            for (uint32_t p = 0; p < TC_TILE / 256; p++) pass(p);
        }
        if ((tid & 63u) == 0 && cnt) atomicAdd(&s_cnt, cnt);
        __syncthreads();
        if (tid == 0) tile_counts[tile] = s_cnt;
        __syncthreads();
    }
}

// ---- prefix: the sum of counts[0 .. t0).  This sum is the critical path of every compaction - up to ntiles counts per workgroup: 16-byte
// loads, TWELVE in flight per thread, so that the 10 M-haystack list's 9766 counts are one round trip for every workgroup instead of
// three; then a scalar tail and the wave sums through `red` (four LDS words).  The vector loads stop at 4 * (t0 / 4), so nothing
// at or beyond counts[t0] is read: what they need of `counts` is its 16-byte alignment (every count array is an allocation of its own).
// Two barriers; `red` is free again on return.
__device__ __forceinline__ uint32_t tc_prefix(const uint32_t* __restrict__ counts, uint32_t t0, uint32_t* red) {
    const uint32_t tid = threadIdx.x;
    uint32_t part = 0;
    const uint4* c4 = (const uint4*)counts;
    const uint32_t n4 = t0 / 4;
    for (uint32_t i0 = 0; i0 < n4; i0 += 12 * 256) {
        uint4 v[12];
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const uint32_t i = i0 + k * 256 + tid;
            v[k] = i < n4 ? c4[i] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < 12; k++) part += v[k].x + v[k].y + v[k].z + v[k].w;
    }
    for (uint32_t k = 4 * n4 + tid; k < t0; k += 256) part += counts[k];
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    if ((tid & 63u) == 0) red[tid >> 6] = part;
    __syncthreads();
    const uint32_t base = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return base;
}

// ---- scan: a batch of up to BATCH <= 256 tile counts, c = the count of tile `tid` of the batch (0 at and beyond the batch's end), into
// pre[tid] = base + the counts in front of it; returns the batch's total.  Two barriers: pre is visible and `red` free again on return.
// A caller may rely on this order: `pre` is not written before the FIRST barrier, and `red` is written in front of it but last read in
// front of the previous call's second one - so a loop that reads `pre` until its next call of this function needs no barrier of its own
// between the reads and the call (tc_compact_items does that).
template <int BATCH = TC_BATCH>
__device__ __forceinline__ uint32_t tc_batch_scan(uint32_t c, uint32_t base, uint32_t* pre, uint32_t* red) {
    static_assert(BATCH >= 1 && BATCH <= 256, "one tile per thread");
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t incl = c;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off);
        if (lane >= (uint32_t)off) incl += v;
    }
    if (lane == 63) red[wave] = incl;
    __syncthreads();
    uint32_t wb = 0;
    for (uint32_t w = 0; w < wave; w++) wb += red[w];
    if (tid < (uint32_t)BATCH) pre[tid] = base + wb + incl - c;
    const uint32_t total = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return total;
}

// ---- rank, across the words of a tile: inclusive sum of c inside each row of 16 lanes - four row_shr steps, lanes without a source add
// 0: four VALU instructions instead of four dependent cross-lane reads through LDS.  A tile's 16 words in 16 consecutive lanes that start
// at a multiple of 16: incl - c is the word's base inside its tile, lane 15's incl the tile's count.
__device__ __forceinline__ uint32_t tc_scan16(uint32_t c) {
    uint32_t incl = c;
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xF, 0xF, false);
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xF, 0xF, false);
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xF, 0xF, false);
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xF, 0xF, false);
    return incl;
}

// ---- the record compaction: the items a bitmap keeps, order preserved, a thread per item - so the loads are coalesced and the stores
// nearly so.  run -> prefix -> scan; then, tile by tile, the tile's 16 words sit in lanes 0..15 of every wave (every word of a tile below
// ntiles was written by the flag pass), tc_scan16 gives the word bases, wave w takes words p * 4 + w, and a kept item's place is
// tc_rank64.  place(where, j) is called for kept item j of the list.  Returns the list's kept count in the LAST workgroup (every earlier
// workgroup's tiles precede its own; n == 0: no workgroup has tiles, the last one still returns 0), which publishes it.
template <class Place>
__device__ __forceinline__ uint32_t tc_compact_items(const uint64_t* __restrict__ bitmap, const uint32_t* __restrict__ counts, uint32_t n, Place place) {
    __shared__ uint32_t red[4];
    __shared__ uint32_t pre[TC_BATCH];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t ntiles = (n + TC_TILE - 1) / TC_TILE;
    uint32_t t0, t1;
    tc_run(ntiles, tc_tiles_per_run(ntiles, gridDim.x), blockIdx.x, &t0, &t1);
    uint32_t base = tc_prefix(counts, t0, red);
    for (uint32_t tb = t0; tb < t1; tb += TC_BATCH) {
        const uint32_t nt = min((uint32_t)TC_BATCH, t1 - tb);
        const uint32_t total = tc_batch_scan(tid < nt ? counts[tb + tid] : 0u, base, pre, red);
        for (uint32_t t = 0; t < nt; t++) {  // (workgroup-uniform trip counts: the cross-lane reads below need every lane)
            const uint64_t w0 = (uint64_t)(tb + t) * TC_WORDS;
            const uint64_t mine = lane < TC_WORDS ? bitmap[w0 + lane] : 0ull;
            const uint32_t pc = (uint32_t)__popcll(mine);
            const uint32_t excl = tc_scan16(pc) - pc;
            const uint32_t tile_base = pre[t];
#pragma unroll
            for (uint32_t p = 0; p < TC_TILE / 256; p++) {
                const int k = (int)(p * 4 + wave);
                const uint64_t bits = ((uint64_t)(uint32_t)__shfl((int)(mine >> 32), k) << 32) | (uint32_t)__shfl((int)(uint32_t)mine, k);
                const uint32_t word_base = (uint32_t)__shfl((int)excl, k);
                if ((bits >> lane) & 1) place(tc_rank64(tile_base + word_base, bits, lane), (w0 + (uint32_t)k) * 64 + lane);
            }
        }
        base += total;  // (the next batch's pre is written behind its scan's first barrier: no barrier of our own)
    }
    return base;
}
#endif  // __HIPCC__
