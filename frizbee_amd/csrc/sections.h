// Sectioned top-`limit`: the decisions of the stage, as plain functions for the device AND the host (kernels_sections.hip calls them;
// tests/kernel_host/sections_host.cpp compiles them for the CPU and tests/test_sections_host.py fuzzes the whole walk against numpy).
//
// The reference has no such call: a picker that shows its results in sections splits what `match_list` returned.  Here a section is a pair
// (require, exclude) over the haystacks' 16 tag bits - the predicate of the visibility scope, scope_visible, called and not restated - and
// element s of a sectioned call is what the top-`limit` selection (topk_select.h) and the ordering of `match_list` make of the records that
// belong to section s.  Sections are independent: they may overlap, repeat or be empty.  The stage runs where the selection runs, over the
// index-ordered records behind the corpus' own scope drop and the bias, and does for every section what topk_select.h says:
//   1. per-section histograms of the scores (first level: the high byte - or, when every score is below 256, the score itself -, whose sum is
//      the section's record count n_s; second level: the low byte within the section's own picked high bin);
//   2. per-section cut (TopkCut: topk_pick_bin / topk_cut_by_score / topk_cut_by_index / topk_cut_keep_all, unchanged), per-tile counts of
//      the members "above T_s" / "equal T_s", their exclusive scans (IndexAsc / IndexDesc: every member is a tie, n_s is the scan's total);
//   3. one stable scatter: topk_dest with the section's running counts, into the section's slab out[s * limit + d];
//   4. the order of a slab's <= SECTIONS_LIMIT_MAX kept records: a rank by (score desc, record position asc - desc for the *Desc strategies).
// The kernels and the host walk call the SAME functions; only the ballots, the shuffles, the LDS and the barriers between them differ.
#pragma once
#include <stdint.h>

#include "scope.h"
#include "topk_select.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FZB_SEC_FN __host__ __device__ __forceinline__
#else
#define FZB_SEC_FN inline
#endif

#define SECTIONS_MAX 8           // == FZB_SECTIONS_MAX (include/frizbee_hip.h)
#define SECTIONS_LIMIT_MAX 1024  // == FZB_SECTION_LIMIT_MAX: a slab is ordered in LDS by one workgroup
#define SECTIONS_TILE 2048       // records per tile of the counts / scan / scatter

// the sections as the kernels take them: by value, as a kernel argument
struct sections_set {
    uint32_t n;
    uint16_t require[SECTIONS_MAX], exclude[SECTIONS_MAX];
};

// a record as the ordering sees it: the haystack's index, then score (low 16 bits) / exact / valid - moved as a whole
struct sections_rec {
    uint32_t index, rest;
};
FZB_SEC_FN uint32_t sections_score(const sections_rec& r) { return r.rest & 0xFFFFu; }

// what the stage keeps per section in device memory (16 words)
struct sections_state {
    uint32_t n;                 // the section's records (found)
    uint32_t hi_bin, above_hi;  // two levels: the picked high bin and the records above it
    TopkCut cut;
    uint32_t kept;              // records of the head: min(limit, n)
    uint32_t tot_gt, tot_eq;    // totals of the two tile-count rows
    uint32_t pad[4];
};

// bit s: the haystack with this tag belongs to section s
FZB_SEC_FN uint32_t sections_mask(const sections_set& ss, uint32_t tag) {
    uint32_t m = 0;
    for (uint32_t s = 0; s < ss.n && s < SECTIONS_MAX; s++)
        if (scope_visible(tag, ss.require[s], ss.exclude[s])) m |= 1u << s;
    return m;
}

// the first-level bin of a score: its high byte, or the score itself when every score is below 256 (one level)
FZB_SEC_FN uint32_t sections_bin_first(uint32_t score, int one_pass) { return one_pass ? score & 255u : score >> 8; }

FZB_SEC_FN uint32_t sections_sum(const uint32_t* bins) {
    uint32_t n = 0;
    for (int b = 0; b < 256; b++) n += bins[b];
    return n;
}

// two levels, step 0: n_s and the high bin from the first-level bins (n_s <= limit or limit 0: no threshold is needed, bin 0)
FZB_SEC_FN void sections_pick_hi(const uint32_t* bins_first, uint32_t limit, sections_state* st) {
    st->n = sections_sum(bins_first);
    st->hi_bin = 0;
    st->above_hi = 0;
    if (limit != 0 && st->n > limit) st->hi_bin = topk_pick_bin(bins_first, limit, &st->above_hi);
}
// does a member's score count in its section's second-level histogram?
FZB_SEC_FN bool sections_in_lo(const sections_state& st, uint32_t limit, uint32_t score) { return limit != 0 && st.n > limit && (score >> 8) == st.hi_bin; }

// the cut of a section by score: n records, lo_bins = the second-level bins (one level: the first-level bins, hi_bin = above_hi = 0)
FZB_SEC_FN TopkCut sections_cut_score(uint32_t n, uint32_t hi_bin, uint32_t above_hi, const uint32_t* lo_bins, uint32_t limit, int desc) {
    if (n <= limit) return topk_cut_keep_all(n);
    return topk_cut_by_score(hi_bin, above_hi, lo_bins, limit, desc);
}
FZB_SEC_FN uint32_t sections_kept(const TopkCut& c, uint32_t n, uint32_t limit) {
    const uint32_t k = c.keep_all ? n : c.gt + c.quota;
    return k < limit ? k : limit;
}

// a member record of a section: 1 = above the threshold, 2 = a tie (every member when nothing is removed or the order is by index), 0 = below
FZB_SEC_FN uint32_t sections_class(const TopkCut& c, int by_score, uint32_t score) {
    if (!by_score || c.keep_all) return 2u;
    return score > c.T ? 1u : score == c.T ? 2u : 0u;
}

// ---- the order of a slab: kept records in record order -> the head of `match_list`'s order ----
// does the record at position j of the slab come before the one at position i?
FZB_SEC_FN bool sections_before(uint32_t score_j, uint32_t j, uint32_t score_i, uint32_t i, int by_score, int desc) {
    if (by_score && score_j != score_i) return score_j > score_i;
    return desc ? j > i : j < i;
}
// where the record at position i of a slab of `kept` records goes
FZB_SEC_FN uint32_t sections_rank(const sections_rec* slab, uint32_t kept, uint32_t i, int by_score, int desc) {
    const uint32_t si = sections_score(slab[i]);
    uint32_t r = 0;
    for (uint32_t j = 0; j < kept; j++) r += sections_before(sections_score(slab[j]), j, si, i, by_score, desc) ? 1u : 0u;
    return r;
}

// ---- the placement of the slabs in ONE dense head (sectioned top-`limit` with matched positions: k_sec_items) ----
// counts = the stage's 2S result words (counts[2s] = records of slab s); slab s holds its records at [s * limit, s * limit + kept_s).
// the records of slab s as the dense head takes them: never more than the slab has room for
FZB_SEC_FN uint32_t sections_slab_kept(const uint32_t* counts, uint32_t s, uint32_t limit) { return counts[2 * s] < limit ? counts[2 * s] : limit; }
// where head s begins in the dense head: the records of the sections in front of it (s == n_sections: the records in all)
FZB_SEC_FN uint32_t sections_head_base(const uint32_t* counts, uint32_t s, uint32_t limit) {
    uint32_t base = 0;
    for (uint32_t t = 0; t < s && t < SECTIONS_MAX; t++) base += sections_slab_kept(counts, t, limit);
    return base;
}
#define SECTIONS_NO_SLOT 0xFFFFFFFFu
// slab slot k (0 <= k < n_sections * limit; section k / limit, record k % limit) -> its place in the dense head, SECTIONS_NO_SLOT for a
// slot without a record.  bases[s] = sections_head_base(counts, s, limit).
FZB_SEC_FN uint32_t sections_head_dest(const uint32_t* counts, const uint32_t* bases, uint32_t limit, uint32_t k) {
    const uint32_t s = k / limit, j = k - s * limit;
    return j < sections_slab_kept(counts, s, limit) ? bases[s] + j : SECTIONS_NO_SLOT;
}
