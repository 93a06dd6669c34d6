// TEST INFRASTRUCTURE: frizbee_amd/csrc/anyof.h - the arithmetic of an any-of group (key pack, max-combine, unpack, the saturating join,
// the search of a hit's slot) - compiled for the host.  aoh_group runs one group the way the device does, through the SAME functions: the
// slots cleared, every alternative's hits folded in by the accumulate loop (a grid-stride loop whose grid is a PARAMETER here), then the
// flag pass (a bit per non-zero slot, a count per tile) and the compaction of tile_compact.h's scheme (tc_run, the prefix, tc_rank64) whose
// `place` writes the group's record: a later group's candidate joined with the key, or the base group's (index_offset + haystack, score,
// exact).  tests/test_anyof_host.py fuzzes it against numpy.
// With -DAOH_MAIN the file is a stand-alone program over a fixed set of groups: the form built with -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "anyof.h"
#include "tile_compact.h"

struct aoh_rec {  // == fzb_match
    uint32_t index;
    uint16_t score;
    uint8_t exact, pad;
};

extern "C" {

uint32_t aoh_alts_max(void) { return ANYOF_ALTS_MAX; }
void aoh_pack(const uint32_t* score, const uint32_t* exact, uint32_t n, uint32_t* out) {
    for (uint32_t k = 0; k < n; k++) out[k] = anyof_pack(score[k], exact[k]);
}
void aoh_combine(const uint32_t* a, const uint32_t* b, uint32_t n, uint32_t* out) {
    for (uint32_t k = 0; k < n; k++) out[k] = anyof_combine(a[k], b[k]);
}
void aoh_unpack(const uint32_t* key, uint32_t n, uint32_t* hit, uint32_t* score, uint32_t* exact) {
    for (uint32_t k = 0; k < n; k++) {
        hit[k] = anyof_hit(key[k]) ? 1u : 0u;
        score[k] = anyof_score(key[k]);
        exact[k] = anyof_exact(key[k]);
    }
}
void aoh_join(const uint32_t* cand_score, const uint32_t* cand_exact, const uint32_t* key, uint32_t n, uint32_t* score, uint32_t* exact) {
    for (uint32_t k = 0; k < n; k++) anyof_join(cand_score[k], cand_exact[k], key[k], &score[k], &exact[k]);
}
void aoh_find(const uint32_t* list, uint32_t n, const uint32_t* values, uint32_t m, uint32_t* out) {
    for (uint32_t k = 0; k < m; k++) out[k] = anyof_find(list, n, values[k]);
}

// One group over n positions.  hits: the alternatives' records one after the other, alternative a has n_hits[a] of them (each index at
// most once per alternative, any order).  cand != nullptr: a later group - n index-ascending candidates, a hit's slot is its candidate's
// position; else items != nullptr: the base group over a candidate set - a hit's slot is the place of (index - index_offset) in the
// ascending item list; else the base group over a range - the slot is index - index_offset.  out: room for n records; returns the count.
uint32_t aoh_group(const aoh_rec* hits, const uint32_t* n_hits, uint32_t n_alts, uint32_t n, uint32_t index_offset, const uint32_t* items, const aoh_rec* cand, uint32_t grid,
                   aoh_rec* out) {
    std::vector<uint32_t> slots(n + 4, 0xDEADBEEFu);
    for (uint32_t j = 0; j < (n + 3) / 4 * 4 && j < slots.size(); j++) slots[j] = 0;  // k_anyof_clear: whole 16-byte words
    std::vector<uint32_t> cand_index(n);
    for (uint32_t j = 0; cand && j < n; j++) cand_index[j] = cand[j].index;
    const aoh_rec* h = hits;
    for (uint32_t a = 0; a < n_alts; a++) {  // k_anyof_accumulate: every thread of the grid takes hits j, j + threads, ..
        const uint32_t threads = grid * 256u;
        for (uint32_t t = 0; t < threads; t++)
            for (uint32_t j = t; j < n_hits[a]; j += threads) {
                const uint32_t p = cand ? anyof_find(cand_index.data(), n, h[j].index) : items ? anyof_find(items, n, h[j].index - index_offset) : h[j].index - index_offset;
                if (p < n) anyof_fold(&slots[p], h[j].score, h[j].exact);
            }
        h += n_hits[a];
    }
    const uint32_t ntiles = (n + TC_TILE - 1) / TC_TILE;  // k_anyof_flag
    std::vector<uint64_t> bitmap((size_t)ntiles * TC_WORDS, 0);
    std::vector<uint32_t> counts(ntiles, 0);
    for (uint32_t j = 0; j < n; j++)
        if (anyof_hit(slots[j])) {
            bitmap[j / 64] |= (uint64_t)1 << (j % 64);
            counts[j / TC_TILE]++;
        }
    uint32_t total = 0;  // k_anyof_compact
    for (uint32_t b = 0; b < grid; b++) {
        uint32_t t0, t1;
        tc_run(ntiles, tc_tiles_per_run(ntiles, grid), b, &t0, &t1);
        uint32_t base = 0;
        for (uint32_t i = 0; i < t0; i++) base += counts[i];
        for (uint32_t t = t0; t < t1; t++) {
            uint32_t word_base = 0;
            for (uint32_t k = 0; k < TC_WORDS; k++) {
                const uint64_t bits = bitmap[(size_t)t * TC_WORDS + k];
                for (uint32_t lane = 0; lane < 64; lane++)
                    if ((bits >> lane) & 1) {
                        const uint32_t j = (t * TC_WORDS + k) * 64 + lane, place = tc_rank64(base + word_base, bits, lane), key = slots[j];
                        aoh_rec r;
                        uint32_t score, exact;
                        if (cand) {
                            r = cand[j];
                            anyof_join(r.score, r.exact, key, &score, &exact);
                        } else {
                            r.index = index_offset + (items ? items[j] : j);
                            r.pad = 0;
                            score = anyof_score(key);
                            exact = anyof_exact(key);
                        }
                        r.score = (uint16_t)score;
                        r.exact = (uint8_t)exact;
                        out[place] = r;
                    }
                word_base += (uint32_t)__builtin_popcountll(bits);
            }
            base += counts[t];
        }
        if (b == grid - 1) total = base;
    }
    return total;
}

}  // extern "C"

#ifdef AOH_MAIN
int main() {
    const uint32_t sizes[] = {1, 63, 64, 65, 1023, 1024, 1025, 2049};
    uint64_t seed = 88172645463325252ull;
    auto next = [&]() {
        seed ^= seed << 13;
        seed ^= seed >> 7;
        seed ^= seed << 17;
        return (uint32_t)(seed >> 11);
    };
    for (uint32_t n : sizes)
        for (uint32_t grid : {1u, 2u, 5u})
            for (int form = 0; form < 3; form++) {
                std::vector<aoh_rec> cand(n), hits, out(n);
                std::vector<uint32_t> items(n), n_hits, want(n, 0);
                for (uint32_t j = 0; j < n; j++) {
                    items[j] = 3 * j + 1;
                    cand[j] = aoh_rec{7 + 2 * j, (uint16_t)(next() % 65536), (uint8_t)(next() & 1), 0};
                }
                for (uint32_t a = 0; a < ANYOF_ALTS_MAX; a++) {
                    uint32_t k = 0;
                    for (uint32_t j = 0; j < n; j++)
                        if (next() % 3 == 0) {
                            const uint32_t s = next() % 65536, e = next() & 1;
                            hits.push_back(aoh_rec{form == 0 ? 7 + 2 * j : form == 1 ? 100 + items[j] : 100 + j, (uint16_t)s, (uint8_t)e, 0});
                            want[j] = anyof_combine(want[j], anyof_pack(s, e));
                            k++;
                        }
                    n_hits.push_back(k);
                }
                const uint32_t got = aoh_group(hits.data(), n_hits.data(), ANYOF_ALTS_MAX, n, form == 0 ? 0 : 100, form == 1 ? items.data() : nullptr, form == 0 ? cand.data() : nullptr, grid,
                                               out.data());
                uint32_t k = 0;
                for (uint32_t j = 0; j < n; j++) {
                    if (!want[j]) continue;
                    uint32_t score = anyof_score(want[j]), exact = anyof_exact(want[j]);
                    if (form == 0) anyof_join(cand[j].score, cand[j].exact, want[j], &score, &exact);
                    const uint32_t index = form == 0 ? cand[j].index : form == 1 ? 100 + items[j] : 100 + j;
                    if (k >= got || out[k].index != index || out[k].score != score || out[k].exact != exact) {
                        printf("mismatch n=%u grid=%u form=%d at %u\n", n, grid, form, k);
                        return 1;
                    }
                    k++;
                }
                if (k != got) {
                    printf("count n=%u grid=%u form=%d: %u vs %u\n", n, grid, form, got, k);
                    return 1;
                }
            }
    printf("anyof_host ok\n");
    return 0;
}
#endif
