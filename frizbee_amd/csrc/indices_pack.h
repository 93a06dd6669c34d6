// Packing step of the fused "top + matched positions" query: the arithmetic, as plain functions for the device AND the host
// (kernels_indices.hip calls them; tests/kernel_host/pack_host.cpp compiles them for the CPU and tests/test_indices_pack_host.py fuzzes them
// against numpy).
//
// The reference has no such call: its caller truncates what `Matcher::match_list_indices` returns (src/matcher/mod.rs:234-275).  Behind the
// top stage the traced scorer leaves, for record k of the head, npos[k] positions at pos[k * stride ..] (`stride` = needle bytes, the most
// a record can have).  The caller's result is DENSE: record k owns positions[begin_k .. begin_k + len_k) with
//   len_k = min(npos_k, stride)   and   begin_k = len_0 + .. + len_(k-1),
// so packing is an exclusive scan and a gather.  Records are taken in tiles of IPACK_TILE (the project's tile: the radix sort's and the
// selection stage's): a head of one tile is scanned inside one workgroup, a longer one as tile sums -> scan of the sums -> per-tile scan
// from the tile's base.  The same pass holds the second pass to the first: traced record k must carry the index, score and exact flag of head
// record k, and there must be as many of them - what the accept decision and the scorers of the reference guarantee (src/matcher/algo.rs:78-103
// against :196-227) is checked on every query instead of assumed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IPACK_HD __host__ __device__ __forceinline__
#else
#define IPACK_HD inline
#endif

#define IPACK_TILE 2048
#define IPACK_SHARE 8  // consecutive records one thread scans: a tile is 256 shares
// bits of the inconsistency word (dev_count[3] of fzb_match_list_top_indices_device)
#define IPACK_BAD_COUNT 1u   // the traced pass produced another number of records than the head has
#define IPACK_BAD_RECORD 2u  // a traced record differs from the head's record at its place

// positions record k contributes: the traced scorer counts what it found and writes at most `stride`
IPACK_HD uint32_t ipack_len(uint32_t npos, uint32_t stride) { return npos < stride ? npos : stride; }

IPACK_HD uint32_t ipack_ntiles(uint32_t n) { return (n + IPACK_TILE - 1) / IPACK_TILE; }

// records [*lo, *hi) of tile `tile` among n
IPACK_HD void ipack_tile_range(uint32_t tile, uint32_t n, uint32_t* lo, uint32_t* hi) {
    const uint32_t a = tile * (uint32_t)IPACK_TILE;
    *lo = a < n ? a : n;
    *hi = n - *lo < (uint32_t)IPACK_TILE ? n : *lo + (uint32_t)IPACK_TILE;
}

// one thread's share of a tile's scan: cnt <= IPACK_SHARE consecutive lengths from npos[first ..] -> their exclusive sums relative to the
// share's start in begins[0 .. IPACK_SHARE) (entries from cnt on repeat the total); returns the share's total.  (A fixed trip count: the
// device keeps `begins` in registers.)
IPACK_HD uint32_t ipack_scan_share(const uint32_t* npos, uint32_t first, uint32_t cnt, uint32_t stride, uint32_t* begins) {
    uint32_t run = 0;
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (uint32_t r = 0; r < IPACK_SHARE; r++) {
        begins[r] = run;
        if (r < cnt) run += ipack_len(npos[first + r], stride);
    }
    return run;
}

// the record that owns dense position d of a tile: begins[0 .. cnt) = the tile's exclusive sums (ascending, equal for records without
// positions), d < the tile's total -> the LAST r with begins[r] <= d (every later record starts beyond d, so r's run covers d)
IPACK_HD uint32_t ipack_find_record(const uint32_t* begins, uint32_t cnt, uint32_t d) {
    uint32_t lo = 0, hi = cnt - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (begins[mid] <= d) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// 0, or why the second pass does not agree with the first
IPACK_HD uint32_t ipack_check_count(uint32_t head_count, uint32_t traced_count) { return head_count == traced_count ? 0u : IPACK_BAD_COUNT; }
IPACK_HD uint32_t ipack_check_record(uint32_t head_index, uint32_t head_score, uint32_t head_exact, uint32_t traced_index, uint32_t traced_score, uint32_t traced_exact) {
    return head_index == traced_index && head_score == traced_score && (head_exact != 0) == (traced_exact != 0) ? 0u : IPACK_BAD_RECORD;
}
