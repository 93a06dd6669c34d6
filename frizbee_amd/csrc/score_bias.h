// Per-haystack score bias of a resident corpus: the arithmetic, as plain functions for the device AND the host (kernels_topk.hip and
// host_upload.hip call them; tests/kernel_host/bias_host.cpp compiles them for the CPU and tests/test_score_bias_host.py fuzzes them
// against numpy).
//
// The reference has no such term: its `match_list` returns the whole Vec and the caller adds a per-item boost (frecency, "file is open")
// and sorts again on the host.  Here the corpus keeps one int16 per haystack and every record's score becomes
//   clamp(score + bias[i], 0, 65535)
// between the scorers and the selection / ordering stage, so the top-`limit` calls select on the ranking the user sees.
//   * sbias_clamp_add     the add;
//   * sbias_one_pass      whether the ordering may still take one radix pass / one histogram level: no biased score can reach 256;
//   * sbias_tile_keeps / sbias_tile_place   the per-tile body of the remove compaction of a per-haystack column (host_upload.hip, k_col_compact):
//     one workgroup per 1024-haystack source tile, a wave per 64 haystacks; a haystack is kept when it lies inside the list and its bit of
//     the pass' bitmap is clear, its rank inside the wave comes from the wave's kept mask (a ballot on the device, a loop over the lanes
//     on the host), the waves' totals go through LDS, and the tile's base is the scanned per-tile kept count - no atomics, nothing ordered
//     between workgroups.  The kernel and the host walk call the SAME two functions; only the ballot and the barrier between them differ.
#pragma once
#include <stdint.h>

#include "tile_compact.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FZB_SBIAS_FN __host__ __device__ __forceinline__
#else
#define FZB_SBIAS_FN inline
#endif

#define SBIAS_TILE 1024  // haystacks per compaction tile: the edit pass' tile (UP_TILE, host_upload.hip)
#define SBIAS_WAVES (SBIAS_TILE / 64)

// the reported score of a record: saturates at both ends, a score biased down to 0 stays in the result
FZB_SBIAS_FN uint32_t sbias_clamp_add(uint32_t score, int32_t bias) {
    const int32_t v = (int32_t)score + bias;
    return v < 0 ? 0u : v > 65535 ? 65535u : (uint32_t)v;
}

// score_bound = the largest unbiased score (score_ceiling + exact_match_bonus), bias_hi = the upper bound of the largest positive bias
FZB_SBIAS_FN bool sbias_one_pass(uint64_t score_bound, uint32_t bias_hi) { return score_bound + (uint64_t)bias_hi < 256; }

// haystack i survives the removal: bit i of the pass' bitmap (32-bit words, bit i & 31 of word i >> 5) marks a removed haystack
FZB_SBIAS_FN bool sbias_kept(const uint32_t* bitmap, uint64_t i) { return !((bitmap[i >> 5] >> (i & 31)) & 1u); }

// kept haystacks of the tile in front of wave `wave` (wave_totals[w] = popcount of wave w's kept mask)
FZB_SBIAS_FN uint32_t sbias_wave_base(const uint32_t* wave_totals, uint32_t wave) {
    uint32_t run = 0;
    for (uint32_t w = 0; w < wave; w++) run += wave_totals[w];
    return run;
}

// ---- the tile body: (wave, lane) of the tile that starts at haystack t0 of a list of n ----
// step 1, every lane: does my haystack survive?  (the wave's kept mask = the ballot of this; its popcount goes to wave_totals[wave])
FZB_SBIAS_FN bool sbias_tile_keeps(const uint32_t* bitmap, uint64_t n, uint64_t t0, uint32_t wave, uint32_t lane) {
    const uint64_t i = t0 + (uint64_t)wave * 64 + lane;
    return i < n && sbias_kept(bitmap, i);
}
// step 2, every KEPT lane, once every wave's total is known: the value goes to tile_base + kept in front of my wave + kept in front of my
// lane; out has room for out_cap entries (the suffix' length: a place beyond it cannot occur and is never written)
// (V: the array's 2-byte value type - int16_t for the bias, uint16_t for the corpus' tags, which follow a removal through the same pass)
template <typename V>
FZB_SBIAS_FN void sbias_tile_place(const V* values, uint64_t t0, uint32_t wave, uint32_t lane, uint64_t kept_mask, const uint32_t* wave_totals, uint64_t tile_base, V* out,
                                   uint64_t out_cap) {
    const uint64_t dst = tile_base + tc_rank64(sbias_wave_base(wave_totals, wave), kept_mask, lane);  // (kept_mask: bit l = lane l's haystack is kept)
    if (dst < out_cap) out[dst] = values[t0 + (uint64_t)wave * 64 + lane];
}
