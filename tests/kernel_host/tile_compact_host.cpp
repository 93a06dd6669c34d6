// TEST INFRASTRUCTURE: frizbee_amd/csrc/tile_compact.h - the tile scheme's plain functions (a workgroup's run of tiles, the rank of a set
// bit, the launchers' grid) - compiled for the host.  tch_walk compacts a bitmap the way tc_compact_items does on the device, through the
// SAME functions: for every workgroup of a grid that is a PARAMETER here, tc_run, the sum of the counts in front of the run, the scan of the
// run's counts in batches of `batch` tiles (256 on the device; a parameter here, so that more than one batch is reached at small sizes),
// then per tile the word bases and tc_rank64 per set bit.  tests/test_tile_compact_host.py fuzzes it against numpy.
// With -DTCH_MAIN the file is a stand-alone program that runs a fixed set of walks against a bit-by-bit count: the form built with
// -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>

#include <utility>
#include <vector>

#include "tile_compact.h"

extern "C" {

uint32_t tch_tile(void) { return TC_TILE; }
uint32_t tch_tiles_per_run(uint32_t ntiles, uint32_t grid) { return tc_tiles_per_run(ntiles, grid); }
void tch_run(uint32_t ntiles, uint32_t per, uint32_t b, uint32_t* out) { tc_run(ntiles, per, b, &out[0], &out[1]); }
int tch_grid(uint64_t units, int grid_max) { return tc_grid(units, grid_max); }

void tch_rank64(const uint64_t* words, const uint32_t* bits, const uint32_t* before, uint32_t n, uint32_t* out) {
    for (uint32_t k = 0; k < n; k++) out[k] = tc_rank64(before[k], words[k], bits[k]);
}
void tch_rank32(const uint32_t* words, const uint32_t* bits, const uint32_t* before, uint32_t n, uint32_t* out) {
    for (uint32_t k = 0; k < n; k++) out[k] = tc_rank32(before[k], words[k], bits[k]);
}

// bitmap: TC_WORDS words for each of the ntiles tiles of a list of n items (bits at and beyond n are clear); out: room for `capacity`
// item numbers - bounded != 0: the first `capacity` kept items are written and pair = (written, kept); bounded == 0: `capacity` is the
// room the caller gave, every kept item is written and pair[0] = kept (pair[1] untouched).  The workgroups run in the order `order` gives.
void tch_walk(const uint64_t* bitmap, uint32_t n, uint32_t grid, uint32_t batch, const uint32_t* order, int bounded, uint32_t* out, uint32_t capacity, uint32_t* pair) {
    const uint32_t ntiles = (n + TC_TILE - 1) / TC_TILE;
    std::vector<uint32_t> counts(ntiles, 0);  // the flag pass' second output
    for (uint32_t t = 0; t < ntiles; t++)
        for (uint32_t w = 0; w < TC_WORDS; w++) counts[t] += (uint32_t)__builtin_popcountll(bitmap[(size_t)t * TC_WORDS + w]);
    for (uint32_t g = 0; g < grid; g++) {
        const uint32_t block = order[g];
        uint32_t t0, t1;
        tc_run(ntiles, tc_tiles_per_run(ntiles, grid), block, &t0, &t1);
        uint32_t base = 0;  // prefix
        for (uint32_t i = 0; i < t0; i++) base += counts[i];
        for (uint32_t tb = t0; tb < t1; tb += batch) {
            const uint32_t nt = t1 - tb < batch ? t1 - tb : batch;
            std::vector<uint32_t> pre(nt);  // scan
            uint32_t run = base;
            for (uint32_t t = 0; t < nt; t++) {
                pre[t] = run;
                run += counts[tb + t];
            }
            for (uint32_t t = 0; t < nt; t++) {  // rank
                const uint64_t w0 = (uint64_t)(tb + t) * TC_WORDS;
                uint32_t word_base = 0;
                for (uint32_t k = 0; k < TC_WORDS; k++) {
                    const uint64_t bits = bitmap[w0 + k];
                    for (uint32_t lane = 0; lane < 64; lane++)
                        if ((bits >> lane) & 1) {
                            const uint32_t place = tc_rank64(pre[t] + word_base, bits, lane);
                            if (place < capacity) out[place] = (uint32_t)((w0 + k) * 64 + lane);
                        }
                    word_base += (uint32_t)__builtin_popcountll(bits);
                }
            }
            base = run;
        }
        if (block == grid - 1) {
            if (bounded) {
                pair[0] = base < capacity ? base : capacity;
                pair[1] = base;
            } else {
                pair[0] = base;
            }
        }
    }
}

}  // extern "C"

#ifdef TCH_MAIN
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

int main() {
    int bad = 0, cases = 0;
    const uint32_t lengths[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 7, 9 * 1024, 40 * 1024 - 1};
    const uint32_t grids[] = {1, 2, 3, 7, 64}, batches[] = {1, 3, 256};
    for (uint32_t n : lengths)
        for (int density = 0; density < 3; density++) {  // none, about half, all
            const uint32_t ntiles = (n + TC_TILE - 1) / TC_TILE;
            std::vector<uint64_t> bitmap((size_t)ntiles * TC_WORDS, 0);
            std::vector<uint32_t> want;
            for (uint32_t j = 0; j < n; j++)
                if (density == 2 || (density == 1 && (rng() & 1))) {
                    bitmap[j >> 6] |= (uint64_t)1 << (j & 63);
                    want.push_back(j);
                }
            for (uint32_t grid : grids)
                for (uint32_t batch : batches)
                    for (int bounded = 0; bounded < 2; bounded++) {
                        std::vector<uint32_t> order(grid);
                        for (uint32_t g = 0; g < grid; g++) order[g] = g;
                        for (uint32_t g = grid; g > 1; g--) std::swap(order[g - 1], order[rng() % g]);
                        const uint32_t kept = (uint32_t)want.size(), capacity = bounded ? kept / 2 : kept;
                        std::vector<uint32_t> out(capacity);  // exactly the room: a store beyond it is the sanitizer's to find
                        uint32_t pair[2] = {~0u, ~0u};
                        tch_walk(bitmap.data(), n, grid, batch, order.data(), bounded, out.data(), capacity, pair);
                        bool ok = bounded ? (pair[0] == capacity && pair[1] == kept) : pair[0] == kept;
                        for (uint32_t k = 0; k < capacity; k++) ok = ok && out[k] == want[k];
                        cases++;
                        if (!ok) {
                            bad++;
                            printf("MISMATCH n=%u density=%d grid=%u batch=%u bounded=%d\n", n, density, grid, batch, bounded);
                        }
                    }
        }
    // the partition where 32-bit products wrap
    const uint32_t big[] = {(1u << 22) + 1, 0x7FFFFFFFu, 0xFFFFFFFFu};
    for (uint32_t ntiles : big)
        for (uint32_t grid = 1; grid <= 70; grid++) {
            const uint32_t per = tc_tiles_per_run(ntiles, grid);
            uint64_t next = 0;
            for (uint32_t b = 0; b < grid; b++) {
                uint32_t t0, t1;
                tc_run(ntiles, per, b, &t0, &t1);
                cases++;
                if (t0 != next || t1 < t0 || t1 - t0 > per) bad++, printf("MISMATCH run ntiles=%u grid=%u b=%u\n", ntiles, grid, b);
                next = t1;
            }
            if (next != ntiles) bad++, printf("MISMATCH cover ntiles=%u grid=%u\n", ntiles, grid);
        }
    printf("%d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
