// TEST INFRASTRUCTURE: frizbee_amd/csrc/sections.h - the decisions of the sectioned top-`limit` stage - compiled for the host.  sec_walk
// walks a record list the way kernels_sections.hip does, through the SAME functions: per-section histograms (one level or two) -> cuts ->
// per-tile counts -> exclusive scans -> topk_dest per record and section -> the rank inside each slab.  A loop over the records of a tile
// stands in for the ballots and the running counters.  tests/test_sections_host.py holds it against numpy; with SEC_MAIN the same source is a
// program of its own for the sanitizers.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "sections.h"

extern "C" {

uint32_t sec_sections_max(void) { return SECTIONS_MAX; }
uint32_t sec_limit_max(void) { return SECTIONS_LIMIT_MAX; }
uint32_t sec_tile(void) { return SECTIONS_TILE; }
uint32_t sec_state_words(void) { return (uint32_t)(sizeof(sections_state) / 4); }

static sections_set make_set(const uint16_t* require, const uint16_t* exclude, uint32_t S) {
    sections_set ss;
    memset(&ss, 0, sizeof ss);
    ss.n = S;
    for (uint32_t s = 0; s < S && s < SECTIONS_MAX; s++) {
        ss.require[s] = require[s];
        ss.exclude[s] = exclude[s];
    }
    return ss;
}

// out[i] = the membership mask of tag i
void sec_masks(const uint16_t* tags, uint32_t n, const uint16_t* require, const uint16_t* exclude, uint32_t S, uint32_t* out) {
    const sections_set ss = make_set(require, exclude, S);
    for (uint32_t i = 0; i < n; i++) out[i] = sections_mask(ss, tags[i]);
}

// out[i] = where record i of the slab goes
void sec_ranks(const uint32_t* slab_words, uint32_t kept, int by_score, int desc, uint32_t* out) {
    for (uint32_t i = 0; i < kept; i++) out[i] = sections_rank((const sections_rec*)slab_words, kept, i, by_score, desc);
}

// rec_words: n index-ordered records (two words each) numbered from 0; tags: n_tags entries (may be null: n_tags 0).  out: S slabs of
// `limit` records; counts: 2S words (kept_s, n_s); cuts: 6 words per section (T, gt, ties, quota, lo, keep_all)
void sec_walk(const uint32_t* rec_words, uint32_t n, const uint16_t* tags, uint64_t n_tags, const uint16_t* require, const uint16_t* exclude, uint32_t S, uint32_t limit, int by_score,
              int desc, int one_pass, uint32_t* out_words, uint32_t* counts, uint32_t* cuts) {
    const sections_rec* recs = (const sections_rec*)rec_words;
    sections_rec* out = (sections_rec*)out_words;
    const sections_set ss = make_set(require, exclude, S);
    if (!tags) n_tags = 0;
    std::vector<sections_state> st(SECTIONS_MAX);
    memset(st.data(), 0, st.size() * sizeof(sections_state));
    std::vector<uint32_t> bins_a(SECTIONS_MAX * 256, 0), bins_b(SECTIONS_MAX * 256, 0);
    if (by_score) {
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t m = sections_mask(ss, scope_tag_of(tags, n_tags, 0, 0, recs[i].index));
            for (uint32_t s = 0; s < S; s++)
                if (m >> s & 1u) bins_a[s * 256 + sections_bin_first(sections_score(recs[i]), one_pass)]++;
        }
        if (!one_pass) {
            for (uint32_t s = 0; s < S; s++) sections_pick_hi(&bins_a[s * 256], limit, &st[s]);
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t m = sections_mask(ss, scope_tag_of(tags, n_tags, 0, 0, recs[i].index));
                for (uint32_t s = 0; s < S; s++)
                    if ((m >> s & 1u) && sections_in_lo(st[s], limit, sections_score(recs[i]))) bins_b[s * 256 + (sections_score(recs[i]) & 255u)]++;
            }
        }
        for (uint32_t s = 0; s < S; s++) {
            if (one_pass) {
                st[s].n = sections_sum(&bins_a[s * 256]);
                st[s].hi_bin = st[s].above_hi = 0;
            }
            st[s].cut = sections_cut_score(st[s].n, st[s].hi_bin, st[s].above_hi, one_pass ? &bins_a[s * 256] : &bins_b[s * 256], limit, desc);
            st[s].kept = sections_kept(st[s].cut, st[s].n, limit);
        }
    }
    const uint32_t ntiles = (n + SECTIONS_TILE - 1) / SECTIONS_TILE;
    std::vector<std::vector<uint32_t>> row(4 * SECTIONS_MAX, std::vector<uint32_t>(ntiles + 1, 0));  // [k * SECTIONS_MAX + s]: counts gt / eq, scans gt / eq
    for (uint32_t tile = 0; tile < ntiles; tile++)
        for (uint32_t i = tile * SECTIONS_TILE; i < n && i < (tile + 1) * SECTIONS_TILE; i++) {
            const uint32_t m = sections_mask(ss, scope_tag_of(tags, n_tags, 0, 0, recs[i].index));
            for (uint32_t s = 0; s < S; s++) {
                const uint32_t cls = (m >> s & 1u) ? sections_class(st[s].cut, by_score, sections_score(recs[i])) : 0u;
                if (cls == 1) row[s][tile]++;
                if (cls == 2) row[SECTIONS_MAX + s][tile]++;
            }
        }
    for (uint32_t s = 0; s < S; s++)
        for (int k = 0; k < 2; k++) {
            uint32_t carry = 0;
            for (uint32_t tile = 0; tile < ntiles; tile++) {
                row[(2 + k) * SECTIONS_MAX + s][tile] = carry;
                carry += row[k * SECTIONS_MAX + s][tile];
            }
            if (k == 0) st[s].tot_gt = carry;
            else st[s].tot_eq = carry;
        }
    if (!by_score)
        for (uint32_t s = 0; s < S; s++) {
            st[s].n = st[s].tot_eq;
            st[s].cut = topk_cut_by_index(st[s].n, limit, desc);
            st[s].kept = sections_kept(st[s].cut, st[s].n, limit);
        }
    for (uint32_t s = 0; s < S; s++) {
        counts[2 * s] = st[s].kept;
        counts[2 * s + 1] = st[s].n;
        const TopkCut& c = st[s].cut;
        const uint32_t w[6] = {c.T, c.gt, c.ties, c.quota, c.lo, c.keep_all};
        memcpy(cuts + 6 * s, w, sizeof w);
    }
    for (uint32_t tile = 0; tile < ntiles; tile++) {
        uint32_t run_gt[SECTIONS_MAX], run_eq[SECTIONS_MAX];
        for (uint32_t s = 0; s < S; s++) {
            run_gt[s] = row[2 * SECTIONS_MAX + s][tile];
            run_eq[s] = row[3 * SECTIONS_MAX + s][tile];
        }
        for (uint32_t i = tile * SECTIONS_TILE; i < n && i < (tile + 1) * SECTIONS_TILE; i++) {
            const uint32_t m = sections_mask(ss, scope_tag_of(tags, n_tags, 0, 0, recs[i].index));
            for (uint32_t s = 0; s < S; s++) {
                const uint32_t cls = (m >> s & 1u) ? sections_class(st[s].cut, by_score, sections_score(recs[i])) : 0u;
                if (!cls) continue;
                const uint32_t d = topk_dest(st[s].cut, by_score, sections_score(recs[i]), run_gt[s], run_eq[s]);
                if (d != TOPK_NOT_KEPT && d < st[s].kept) out[(size_t)s * limit + d] = recs[i];
                run_gt[s] += cls == 1;
                run_eq[s] += cls == 2;
            }
        }
    }
    std::vector<sections_rec> slab(SECTIONS_LIMIT_MAX);
    for (uint32_t s = 0; s < S; s++) {
        const uint32_t kept = st[s].kept;
        sections_rec* const dst = out + (size_t)s * limit;
        for (uint32_t i = 0; i < kept; i++) slab[i] = dst[i];
        for (uint32_t i = 0; i < kept; i++) dst[sections_rank(slab.data(), kept, i, by_score, desc)] = slab[i];
    }
}

}  // extern "C"

#ifdef SEC_MAIN
#include <stdio.h>

#include <algorithm>
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

// one section's head by the definition: the members, reversed for the *Desc strategies, stable sort by descending score, cut
static std::vector<sections_rec> model(const std::vector<sections_rec>& recs, const std::vector<uint16_t>& tags, uint16_t require, uint16_t exclude, uint32_t limit, int by_score,
                                       int desc, uint32_t* found) {
    std::vector<sections_rec> sel;
    for (const sections_rec& r : recs) {
        const uint32_t tag = r.index < tags.size() ? tags[r.index] : 0u;
        if ((tag & require) == require && (tag & exclude) == 0) sel.push_back(r);
    }
    *found = (uint32_t)sel.size();
    if (desc) std::reverse(sel.begin(), sel.end());
    if (by_score) std::stable_sort(sel.begin(), sel.end(), [](const sections_rec& a, const sections_rec& b) { return sections_score(a) > sections_score(b); });
    if (sel.size() > limit) sel.resize(limit);
    return sel;
}

int main() {
    int bad = 0, cases = 0;
    const uint16_t require[SECTIONS_MAX] = {1, 2, 0, 0xF0, 1, 1, 0xFFF, 0}, exclude[SECTIONS_MAX] = {0, 1, 0, 0, 1, 0, 0, 0x8000};
    const uint32_t lengths[] = {0, 1, 255, 256, 257, 2047, 2048, 2049, 5000};
    const uint32_t limits[] = {0, 1, 5, 100, 1023, 1024};
    for (uint32_t n : lengths)
        for (int kind = 0; kind < 3; kind++) {  // scores below 256 (one level), on both sides of 256, heavy ties
            const uint32_t n_hay = n + n / 2 + 3;
            std::vector<uint16_t> tags(n_hay - (kind == 1 ? 2 : 0));  // (kind 1: the last haystacks lie beyond the column: tag 0)
            for (auto& t : tags) t = (uint16_t)(rng() & (rng() % 3 ? 0xFFFFu : 0x00F3u));
            std::vector<sections_rec> recs(n);
            uint32_t at = 0;
            for (uint32_t j = 0; j < n; j++) {  // n ascending haystacks out of n_hay
                at += (uint32_t)(rng() % ((n_hay - at - (n - j)) / (n - j) + 1));
                const uint32_t score = kind == 0 ? (uint32_t)(rng() % 256) : kind == 1 ? (uint32_t)(rng() % 700) : (rng() % 4 ? 96u : 300u);
                recs[j].index = at++;
                recs[j].rest = score | ((uint32_t)(rng() & 1) << 16) | (1u << 24);
            }
            for (uint32_t limit : limits)
                for (int sort = 0; sort < 4; sort++) {
                    const int by_score = sort < 2, desc = sort & 1;
                    std::vector<sections_rec> out((size_t)SECTIONS_MAX * limit + 1);
                    uint32_t counts[2 * SECTIONS_MAX], cuts[6 * SECTIONS_MAX];
                    sec_walk((const uint32_t*)recs.data(), n, tags.data(), tags.size(), require, exclude, SECTIONS_MAX, limit, by_score, desc, by_score && kind == 0,
                             (uint32_t*)out.data(), counts, cuts);
                    for (uint32_t s = 0; s < SECTIONS_MAX; s++) {
                        uint32_t found = 0;
                        const std::vector<sections_rec> want = model(recs, tags, require[s], exclude[s], limit, by_score, desc, &found);
                        bad += counts[2 * s] != want.size() || counts[2 * s + 1] != found;
                        for (size_t k = 0; k < want.size() && k < counts[2 * s]; k++)
                            bad += out[(size_t)s * limit + k].index != want[k].index || out[(size_t)s * limit + k].rest != want[k].rest;
                        cases++;
                    }
                }
        }
    printf("%d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
