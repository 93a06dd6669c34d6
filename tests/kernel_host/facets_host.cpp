// TEST INFRASTRUCTURE: frizbee_amd/csrc/facets.h - the tag facets' per-record rule and accumulation - compiled for the host.  fh_records
// walks a record list the way k_facets_records and k_scope_flag_facets do, through the SAME functions: tile by tile, 64 lanes at a time
// (facets_lane_step: the loop over the lanes that stands in for the wave's 34 ballots), the tag through scope_tag_of, visibility through
// scope_visible; fh_column walks a range or an item list the way k_facets_column does.  tests/test_facets_host.py holds both against
// numpy; with FH_MAIN the same source is a program of its own for the sanitizers.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "facets.h"

extern "C" {

uint32_t fh_words(void) { return FZB_FACET_WORDS; }

// recs: n index-ordered records (two words each) of the range that starts at haystack `first`, numbered from index_offset; tags: n_tags
// entries (may be null: n_tags 0); out: FZB_FACET_WORDS words
void fh_records(const uint32_t* rec_words, uint32_t n, const uint16_t* tags, uint64_t n_tags, uint64_t first, uint32_t index_offset, uint32_t require, uint32_t exclude, uint32_t* out) {
    const scope_rec* recs = (const scope_rec*)rec_words;
    const uint32_t ntiles = (n + SCOPE_TILE - 1) / SCOPE_TILE;
    facet_acc acc;
    facets_clear(acc);
    for (uint32_t tile = 0; tile < ntiles; tile++)
        for (uint32_t slot = 0; slot < SCOPE_TILE; slot++) {  // (the slots beyond the list's end are walked too, as the device's lanes are)
            const uint64_t j = (uint64_t)tile * SCOPE_TILE + slot;
            const bool valid = j < n;
            const uint32_t tag = valid ? scope_tag_of(tags, tags ? n_tags : 0, first, index_offset, recs[j].index) : 0u;
            facets_lane_step(acc, valid, tag, require, exclude);
        }
    for (int k = 0; k < FZB_FACET_WORDS; k++) out[k] = acc.w[k];
}

// items == nullptr: the n haystacks from `first`; else the n items of a candidate set
void fh_column(const uint32_t* items, uint32_t n, const uint16_t* tags, uint64_t n_tags, uint64_t first, uint32_t require, uint32_t exclude, uint32_t* out) {
    const uint32_t ntiles = (n + SCOPE_TILE - 1) / SCOPE_TILE;
    facet_acc acc;
    facets_clear(acc);
    for (uint32_t tile = 0; tile < ntiles; tile++)
        for (uint32_t slot = 0; slot < SCOPE_TILE; slot++) {
            const uint64_t k = (uint64_t)tile * SCOPE_TILE + slot;
            const bool valid = k < n;
            const uint32_t tag = valid ? facet_item_tag(items, k, tags, n_tags, first) : 0u;
            facets_lane_step(acc, valid, tag, require, exclude);
        }
    for (int k = 0; k < FZB_FACET_WORDS; k++) out[k] = acc.w[k];
}

}  // extern "C"

#ifdef FH_MAIN
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

// the counts by the definition, one haystack at a time
static void model(const std::vector<uint64_t>& hay, const std::vector<uint16_t>& tags, uint32_t require, uint32_t exclude, uint32_t* out) {
    for (int k = 0; k < FZB_FACET_WORDS; k++) out[k] = 0;
    for (uint64_t h : hay) {
        const uint32_t tag = h < tags.size() ? tags[h] : 0u;
        const bool vis = (tag & require) == require && (tag & exclude) == 0;
        out[0]++;
        out[1] += vis;
        for (int b = 0; b < 16; b++) {
            out[2 + b] += (tag >> b) & 1u;
            out[18 + b] += vis ? (tag >> b) & 1u : 0u;
        }
    }
}

int main() {
    int bad = 0, cases = 0;
    const uint32_t lengths[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 21 * 1024 + 37};
    const uint32_t scopes[][2] = {{0, 0}, {1, 0}, {0, 1}, {2, 1}, {0x8000, 0}, {0, 0x8000}, {3, 3}, {0xFFFF, 0}, {0, 0xFFFF}};
    for (uint32_t n : lengths)
        for (int rep = 0; rep < 2; rep++) {
            const uint64_t first = rep ? 37 : 0;
            const uint32_t index_offset = rep ? 4000000000u : 0u;
            const uint64_t span = (uint64_t)n + n / 3 + 5;
            const uint64_t n_tags = first + span - (rep ? 3 : 0);  // (rep 1: the last haystacks lie beyond the column: tag 0)
            std::vector<uint16_t> tags(n_tags);
            for (auto& t : tags) t = (rng() % 8 == 0) ? 0xFFFFu : (uint16_t)(rng() | ((rng() % 4 == 0) ? 0x8000u : 0u));
            std::vector<uint32_t> recs(2 * (size_t)n + 2), items(n + 1);
            std::vector<uint64_t> hay;
            uint64_t at = 0;
            for (uint32_t j = 0; j < n; j++) {  // n ascending haystacks out of span
                const uint64_t room = span - at - (n - j);
                at += room ? rng() % (room / (n - j) + 1) : 0;
                recs[2 * (size_t)j] = (uint32_t)(index_offset + at);
                recs[2 * (size_t)j + 1] = (uint32_t)rng();
                items[j] = (uint32_t)at;
                hay.push_back(first + at);
                at++;
            }
            for (const auto& sc : scopes) {
                uint32_t want[FZB_FACET_WORDS], got[FZB_FACET_WORDS];
                model(hay, tags, sc[0], sc[1], want);
                fh_records(recs.data(), n, tags.data(), n_tags, first, index_offset, sc[0], sc[1], got);
                for (int k = 0; k < FZB_FACET_WORDS; k++) bad += got[k] != want[k];
                fh_column(items.data(), n, tags.data(), n_tags, first, sc[0], sc[1], got);
                for (int k = 0; k < FZB_FACET_WORDS; k++) bad += got[k] != want[k];
                cases += 2;
            }
        }
    printf("%d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
