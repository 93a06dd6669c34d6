// Top-`limit` selection: the two decisions of the stage, as plain functions for the device AND the host (kernels_topk.hip calls them;
// tests/kernel_host/topk_host.cpp compiles them for the CPU and fuzzes them against numpy).
//
// The reference has no such call: its `match_list` returns a Vec the caller truncates.  What is selected here is the PREFIX of that list:
// `match_list` reverses the index-ordered records for the *Desc strategies and then sorts them stably by descending score
// (src/matcher/mod.rs:215-221, src/sort.rs:6-40), so the first `limit` records of the result are
//   * every record with score > T, where T is the score with count(score > T) < limit <= count(score >= T), and
//   * of the records with score == T, the first (limit - count(score > T)) in record order - the LAST that many for the *Desc
//     strategies, whose reverse has not happened yet when the selection runs.
// The kept records stay in record order, so the reverse / stable sort of the kept records is the head of the sorted whole.
// For IndexAsc / IndexDesc every record is a "tie": the first / last `limit` records.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TOPK_HD __host__ __device__ __forceinline__
#else
#define TOPK_HD inline
#endif

#define TOPK_NOT_KEPT 0xFFFFFFFFu

struct TopkCut {
    uint32_t T;         // threshold score (0x10000: nothing is above or equal - limit 0)
    uint32_t gt;        // records with score > T (all kept)
    uint32_t ties;      // records with score == T
    uint32_t quota;     // of those, how many are kept: the ties of rank lo .. lo + quota - 1 (rank = position among the ties, in record order)
    uint32_t lo;
    uint32_t keep_all;  // found <= limit: nothing to remove
};

// bins[b] = number of records in bin b (256 bins, bin order = score order).  The bin B with count(bin > B) < need <= count(bin >= B);
// *above = count(bin > B).  Precondition: 1 <= need <= total.  (A `need` beyond the total - cannot happen behind the callers' checks -
// ends in bin 0 with above = total - bins[0]: still inside the table.)
TOPK_HD uint32_t topk_pick_bin(const uint32_t* bins, uint32_t need, uint32_t* above) {
    uint32_t acc = 0;
    int b = 255;
    for (; b > 0; b--) {
        if (acc + bins[b] >= need) break;
        acc += bins[b];
    }
    *above = acc;
    return (uint32_t)b;
}

TOPK_HD TopkCut topk_cut_keep_all(uint32_t n) {
    TopkCut c;
    c.T = 0; c.gt = 0; c.ties = n; c.quota = n; c.lo = 0; c.keep_all = 1;
    return c;
}

// IndexAsc / IndexDesc: the first / last min(limit, n) records
TOPK_HD TopkCut topk_cut_by_index(uint32_t n, uint32_t limit, int desc) {
    if (n <= limit) return topk_cut_keep_all(n);
    TopkCut c;
    c.T = 0; c.gt = 0; c.ties = n; c.quota = limit; c.lo = desc ? n - limit : 0; c.keep_all = 0;
    return c;
}

// Score strategies, n > limit.  hi_bin = topk_pick_bin(histogram of score >> 8, limit) and `above_hi` its count above; lo_bins =
// histogram of score & 255 over the records whose high byte is hi_bin (with every score below 256: hi_bin = 0, above_hi = 0).
TOPK_HD TopkCut topk_cut_by_score(uint32_t hi_bin, uint32_t above_hi, const uint32_t* lo_bins, uint32_t limit, int desc) {
    TopkCut c;
    c.keep_all = 0;
    if (limit == 0) {
        c.T = 0x10000u; c.gt = 0; c.ties = 0; c.quota = 0; c.lo = 0;
        return c;
    }
    uint32_t above_lo = 0;
    const uint32_t lo_bin = topk_pick_bin(lo_bins, limit - above_hi, &above_lo);
    c.T = (hi_bin << 8) | lo_bin;
    c.gt = above_hi + above_lo;
    c.ties = lo_bins[lo_bin];
    c.quota = limit - c.gt;
    if (c.quota > c.ties) c.quota = c.ties;
    c.lo = desc ? c.ties - c.quota : 0;
    return c;
}

// Where record i goes in the selected list, or TOPK_NOT_KEPT.  gt_before / eq_before = records before i (in record order) with
// score > T / score == T.  by_score = 0: every record is a tie.
TOPK_HD uint32_t topk_dest(const TopkCut& c, int by_score, uint32_t score, uint32_t gt_before, uint32_t eq_before) {
    if (c.keep_all) return gt_before + eq_before;
    const bool is_gt = by_score && score > c.T;
    const bool is_eq = !by_score || score == c.T;
    if (is_gt) {
        const uint32_t ties_kept_before = eq_before <= c.lo ? 0u : (eq_before - c.lo < c.quota ? eq_before - c.lo : c.quota);
        return gt_before + ties_kept_before;
    }
    if (is_eq && eq_before >= c.lo && eq_before - c.lo < c.quota) return gt_before + (eq_before - c.lo);
    return TOPK_NOT_KEPT;
}
