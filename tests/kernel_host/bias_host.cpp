// TEST INFRASTRUCTURE: frizbee_amd/csrc/score_bias.h - the clamp-add of the per-haystack score bias, the "one radix pass / one histogram
// level" decision and the per-tile body of the remove compaction of the bias array - compiled for the host.  bh_compact_tile runs one
// 1024-haystack source tile through the two functions k_bias_compact (host_upload.hip) runs, sbias_tile_keeps and sbias_tile_place: a loop
// over the lanes stands in for the wave's ballot, an array for the LDS totals, the end of the first loop for the barrier.
// tests/test_score_bias_host.py fuzzes it against numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "score_bias.h"

extern "C" {

uint32_t bh_tile(void) { return SBIAS_TILE; }

// scores[k] + biases[k] for n pairs
void bh_clamp_add(const uint16_t* scores, const int16_t* biases, uint32_t n, uint16_t* out) {
    for (uint32_t k = 0; k < n; k++) out[k] = (uint16_t)sbias_clamp_add(scores[k], biases[k]);
}

int bh_one_pass(uint64_t score_bound, uint32_t bias_hi) { return sbias_one_pass(score_bound, bias_hi) ? 1 : 0; }

// One source tile: haystacks [t0, min(t0 + SBIAS_TILE, n)) of the list, bitmap = the pass' words from word 0 of the list on (bit i = haystack i
// is removed), values = the list's biases, tile_base = kept haystacks of the suffix in front of the tile (the pass' scanned count), out =
// the suffix' scratch of out_cap entries.  Returns the tile's kept count.
uint32_t bh_compact_tile(const uint32_t* bitmap, const int16_t* values, uint64_t n, uint64_t t0, uint64_t tile_base, int16_t* out, uint64_t out_cap) {
    uint64_t mask[SBIAS_WAVES];
    uint32_t total[SBIAS_WAVES];
    for (uint32_t wave = 0; wave < SBIAS_WAVES; wave++) {  // the ballots, and what lane 0 of every wave leaves in LDS
        mask[wave] = 0;
        for (uint32_t lane = 0; lane < 64; lane++)
            if (sbias_tile_keeps(bitmap, n, t0, wave, lane)) mask[wave] |= (uint64_t)1 << lane;
        total[wave] = (uint32_t)__builtin_popcountll(mask[wave]);
    }
    for (uint32_t wave = 0; wave < SBIAS_WAVES; wave++)  // behind the barrier: every kept lane
        for (uint32_t lane = 0; lane < 64; lane++)
            if ((mask[wave] >> lane) & 1) sbias_tile_place(values, t0, wave, lane, mask[wave], total, tile_base, out, out_cap);
    return sbias_wave_base(total, SBIAS_WAVES);
}

}  // extern "C"
