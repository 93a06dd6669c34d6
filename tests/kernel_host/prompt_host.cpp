// TEST INFRASTRUCTURE: frizbee_amd/csrc/prompt_records.h - the per-item rule of the empty prompt - compiled for the host.  ph_records walks
// a range the way k_prompt_records (kernels_prompt.hip) does, ph_compact an item list the way k_prompt_flag and k_prompt_compact do, through
// the SAME functions: prompt_tile_keeps per item of a tile (a loop over the lanes stands in for the wave's ballot), then, for every workgroup
// of a grid that is a PARAMETER here, tc_run (tile_compact.h), the sum of the counts in front of the run, the scan of the run's counts in
// batches of `batch` tiles, scope_place / prompt_store per kept item and scope_counts by the last workgroup.
// tests/test_prompt_records_host.py fuzzes both against numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "prompt_records.h"

extern "C" {

uint32_t ph_tile(void) { return SCOPE_TILE; }

// the n haystacks from `first`, numbered from index_offset, no scope; bias may be null; out: room for `capacity` records; pair: (written, found)
void ph_records(uint32_t* out_words, uint32_t n, uint32_t capacity, const int16_t* bias, uint64_t n_bias, uint64_t first, uint32_t index_offset, uint32_t* pair) {
    scope_rec* out = (scope_rec*)out_words;
    const uint32_t m = n < capacity ? n : capacity;
    for (uint32_t j = 0; j < m; j++) out[j] = prompt_record(bias, n_bias, first, index_offset, j);
    scope_counts(n, capacity, pair);
}

// items: n ascending local indices, or null (the range's n haystacks); tags may be null (no active scope); the workgroups run in the order
// `order` gives (grid entries)
void ph_compact(const uint32_t* items, uint32_t n, const uint16_t* tags, uint64_t n_tags, const int16_t* bias, uint64_t n_bias, uint64_t first, uint32_t index_offset, uint32_t require,
                uint32_t exclude, uint32_t grid, uint32_t batch, const uint32_t* order, uint32_t* out_words, uint32_t capacity, uint32_t* pair) {
    scope_rec* out = (scope_rec*)out_words;
    const uint32_t ntiles = (n + SCOPE_TILE - 1) / SCOPE_TILE;
    std::vector<uint64_t> bitmap((size_t)ntiles * SCOPE_WORDS + 1, 0);
    std::vector<uint32_t> counts(ntiles + 1, 0);
    for (uint32_t tile = 0; tile < ntiles; tile++)
        for (uint32_t w = 0; w < SCOPE_WORDS; w++) {
            uint64_t b = 0;
            for (uint32_t lane = 0; lane < 64; lane++)
                if (prompt_tile_keeps(items, n, tile, w * 64 + lane, tags, n_tags, first, require, exclude)) b |= (uint64_t)1 << lane;
            bitmap[(size_t)tile * SCOPE_WORDS + w] = b;
            counts[tile] += (uint32_t)__builtin_popcountll(b);
        }
    for (uint32_t g = 0; g < grid; g++) {
        const uint32_t block = order[g];
        uint32_t t0, t1;
        tc_run(ntiles, tc_tiles_per_run(ntiles, grid), block, &t0, &t1);
        uint32_t base = 0;
        for (uint32_t i = 0; i < t0; i++) base += counts[i];
        for (uint32_t tb = t0; tb < t1; tb += batch) {
            const uint32_t nt = t1 - tb < batch ? t1 - tb : batch;
            std::vector<uint32_t> pre(nt);
            uint32_t run = base;
            for (uint32_t t = 0; t < nt; t++) {
                pre[t] = run;
                run += counts[tb + t];
            }
            for (uint32_t t = 0; t < nt; t++) {
                const uint64_t w0 = (uint64_t)(tb + t) * SCOPE_WORDS;
                uint32_t word_base = 0;
                for (uint32_t k = 0; k < SCOPE_WORDS; k++) {
                    const uint64_t bits = bitmap[w0 + k];
                    for (uint32_t lane = 0; lane < 64; lane++)
                        if ((bits >> lane) & 1) prompt_store(out, capacity, scope_place(pre[t], word_base, bits, lane), items, (w0 + k) * 64 + lane, bias, n_bias, first, index_offset);
                    word_base += (uint32_t)__builtin_popcountll(bits);
                }
            }
            base = run;
        }
        if (block == grid - 1) scope_counts(base, capacity, pair);
    }
}

}  // extern "C"
