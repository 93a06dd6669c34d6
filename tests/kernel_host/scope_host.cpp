// TEST INFRASTRUCTURE: frizbee_amd/csrc/scope.h - the visibility predicate of a corpus' tags and the arithmetic of the drop pass - compiled
// for the host.  sh_drop walks a record list the way k_scope_flag and k_scope_compact (kernels_topk.hip) do, through the SAME functions:
// scope_tile_keeps per record of a tile (a loop over the lanes stands in for the wave's ballot), then, for every workgroup of a grid that is
// a PARAMETER here, tc_run (tile_compact.h), the sum of the counts in front of the run, the scan of the run's counts in batches of `batch` tiles
// (256 on the device; a parameter here, so that several tiles per workgroup and more than one batch are reached at small sizes), scope_place
// / scope_store per kept record and scope_counts by the last workgroup.  tests/test_scope_host.py fuzzes it against numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "scope.h"

extern "C" {

uint32_t sh_tile(void) { return SCOPE_TILE; }

void sh_visible(const uint16_t* tags, uint32_t n, uint32_t require, uint32_t exclude, uint8_t* out) {
    for (uint32_t k = 0; k < n; k++) out[k] = scope_visible(tags[k], require, exclude) ? 1 : 0;
}

// recs: n index-ordered records (two words each) of the range that starts at haystack `first`, numbered from index_offset; tags: n_tags
// entries; out: room for `capacity` records; pair: (written, found).  The workgroups run in the order `order` gives (grid entries).
void sh_drop(const uint32_t* rec_words, uint32_t n, const uint16_t* tags, uint64_t n_tags, uint64_t first, uint32_t index_offset, uint32_t require, uint32_t exclude, uint32_t grid,
             uint32_t batch, const uint32_t* order, uint32_t* out_words, uint32_t capacity, uint32_t* pair) {
    const scope_rec* recs = (const scope_rec*)rec_words;
    scope_rec* out = (scope_rec*)out_words;
    const uint32_t ntiles = (n + SCOPE_TILE - 1) / SCOPE_TILE;
    // the flag pass: one word per 64 records, one count per tile
    std::vector<uint64_t> bitmap((size_t)ntiles * SCOPE_WORDS + 1, 0);
    std::vector<uint32_t> counts(ntiles + 1, 0);
    for (uint32_t tile = 0; tile < ntiles; tile++)
        for (uint32_t w = 0; w < SCOPE_WORDS; w++) {
            uint64_t b = 0;
            for (uint32_t lane = 0; lane < 64; lane++)
                if (scope_tile_keeps(recs, n, tile, w * 64 + lane, tags, n_tags, first, index_offset, require, exclude)) b |= (uint64_t)1 << lane;
            bitmap[(size_t)tile * SCOPE_WORDS + w] = b;
            counts[tile] += (uint32_t)__builtin_popcountll(b);
        }
    // the compaction, workgroup by workgroup
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
                        if ((bits >> lane) & 1) scope_store(out, capacity, scope_place(pre[t], word_base, bits, lane), recs, (w0 + k) * 64 + lane);
                    word_base += (uint32_t)__builtin_popcountll(bits);
                }
            }
            base = run;
        }
        if (block == grid - 1) scope_counts(base, capacity, pair);
    }
}

}  // extern "C"
