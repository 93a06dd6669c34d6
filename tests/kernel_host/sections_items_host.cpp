// TEST INFRASTRUCTURE: the placement arithmetic of frizbee_amd/csrc/sections.h - where the sectioned stage's slabs go in the ONE dense head of
// the form with matched positions - compiled for the host.  sih_items walks the S * limit slab slots the way k_sec_items does, through the SAME
// functions (sections_slab_kept, sections_head_base, sections_head_dest): the bases first, then slot by slot, then the words workgroup 0
// writes.  tests/test_sections_items_host.py holds it against a numpy concatenation; with SIH_MAIN the same source is a program of its own
// for the sanitizers.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "sections.h"

extern "C" {

uint32_t sih_no_slot(void) { return SECTIONS_NO_SLOT; }

// slabs: n_sections * limit records (two words each: index, rest); counts: the stage's 2S words; head / items: room for cap entries;
// dev_counts: 2S + 4 words of which [2S] and [2S + 1] are not written (the pack's); words: [0] = the item count, [1], [2] = the head's pair.
// Returns the number of slots that had a record but no room (0 whenever cap >= the sum of the kept counts).
uint32_t sih_items(const uint32_t* slabs, const uint32_t* counts, uint32_t n_sections, uint32_t limit, uint32_t cap, uint32_t* head, uint32_t* items, uint32_t* dev_counts,
                   uint32_t* words) {
    const uint32_t S = n_sections < SECTIONS_MAX ? n_sections : SECTIONS_MAX;
    uint32_t bases[SECTIONS_MAX + 1];
    for (uint32_t s = 0; s <= S; s++) bases[s] = sections_head_base(counts, s, limit);
    uint32_t dropped = 0;
    for (uint32_t k = 0; k < S * limit; k++) {
        const uint32_t d = sections_head_dest(counts, bases, limit, k);
        if (d == SECTIONS_NO_SLOT) continue;
        if (d >= cap) {
            dropped++;
            continue;
        }
        head[2 * (size_t)d] = slabs[2 * (size_t)k];
        head[2 * (size_t)d + 1] = slabs[2 * (size_t)k + 1];
        items[d] = slabs[2 * (size_t)k];
    }
    for (uint32_t w = 0; w < 2 * S; w++) dev_counts[w] = (w & 1u) ? counts[w] : sections_slab_kept(counts, w >> 1, limit);
    const uint32_t total = bases[S] < cap ? bases[S] : cap;
    words[0] = words[1] = words[2] = total;
    dev_counts[2 * S + 2] = 0;
    dev_counts[2 * S + 3] = 0;
    return dropped;
}

}  // extern "C"

#ifdef SIH_MAIN
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

int main() {
    int bad = 0, cases = 0;
    const uint32_t limits[] = {0, 1, 2, 255, 256, 257, 1024};
    for (uint32_t S = 0; S <= SECTIONS_MAX; S++)
        for (uint32_t limit : limits)
            for (int rep = 0; rep < 6; rep++) {
                // exactly sized arrays: a write or a read beyond them is the sanitizer's to find
                std::vector<uint32_t> counts(2 * S), slabs(2 * (size_t)S * limit), dev_counts(2 * S + 4, 0xABABABABu), words(3);
                std::vector<uint32_t> want_head, want_items;
                const uint32_t choice[4] = {0, 1, limit ? limit - 1 : 0, limit};
                for (uint32_t s = 0; s < S; s++) {
                    uint32_t kept = rep == 0 ? 0 : rep == 1 ? limit : choice[rng() % 4];
                    if (kept > limit) kept = limit;
                    counts[2 * s] = rep == 5 ? kept + (uint32_t)(rng() % 3) * limit : kept;  // (a count beyond the slab is clamped to the slab)
                    counts[2 * s + 1] = (uint32_t)rng();
                    kept = counts[2 * s] < limit ? counts[2 * s] : limit;
                    for (uint32_t j = 0; j < limit; j++) {
                        slabs[2 * ((size_t)s * limit + j)] = (uint32_t)rng();
                        slabs[2 * ((size_t)s * limit + j) + 1] = (uint32_t)rng();
                    }
                    for (uint32_t j = 0; j < kept; j++) {
                        want_head.push_back(slabs[2 * ((size_t)s * limit + j)]);
                        want_head.push_back(slabs[2 * ((size_t)s * limit + j) + 1]);
                        want_items.push_back(slabs[2 * ((size_t)s * limit + j)]);
                    }
                }
                const uint32_t cap = (uint32_t)want_items.size();
                std::vector<uint32_t> head(2 * (size_t)cap), items(cap);
                bad += sih_items(slabs.data(), counts.data(), S, limit, cap, head.data(), items.data(), dev_counts.data(), words.data()) != 0;
                bad += head != want_head;
                bad += items != want_items;
                bad += words[0] != cap || words[1] != cap || words[2] != cap;
                for (uint32_t s = 0; s < S; s++) bad += dev_counts[2 * s] != (counts[2 * s] < limit ? counts[2 * s] : limit) || dev_counts[2 * s + 1] != counts[2 * s + 1];
                bad += dev_counts[2 * S] != 0xABABABABu || dev_counts[2 * S + 1] != 0xABABABABu || dev_counts[2 * S + 2] != 0 || dev_counts[2 * S + 3] != 0;
                cases++;
            }
    printf("%d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
