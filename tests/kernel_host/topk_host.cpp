// TEST INFRASTRUCTURE: frizbee_amd/csrc/topk_select.h - the two decisions of the top-`limit` selection stage ("which threshold, how many
// ties" from the histograms; "is record i kept, and where does it go") - compiled for the host.  th_select walks a score array the way
// kernels_topk.hip does (histogram of the high byte, bucket, histogram of the low byte inside it, cut, running counts of the records
// above / at the threshold) with every decision taken by the header's functions.  tests/test_topk_select_host.py fuzzes it against numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "topk_select.h"

extern "C" {

// scores[n] in record order -> dest[n] (position in the selected list, or 0xFFFFFFFF), cut_out[6] = {T, gt, ties, quota, lo, keep_all};
// returns the number of records kept.  one_pass: the caller knows every score is below 256 (the high-byte level is skipped).
uint32_t th_select(const uint16_t* scores, uint32_t n, uint32_t limit, int by_score, int desc, int one_pass, uint32_t* dest, uint32_t* cut_out) {
    TopkCut c;
    if (n <= limit) {
        c = topk_cut_keep_all(n);
    } else if (!by_score) {
        c = topk_cut_by_index(n, limit, desc);
    } else if (limit == 0) {
        uint32_t none[256];
        memset(none, 0, sizeof(none));
        c = topk_cut_by_score(0, 0, none, 0, desc);
    } else {
        uint32_t hi[256], lo[256];
        memset(hi, 0, sizeof(hi));
        memset(lo, 0, sizeof(lo));
        uint32_t hi_bin = 0, above_hi = 0;
        if (!one_pass) {
            for (uint32_t i = 0; i < n; i++) hi[scores[i] >> 8]++;
            hi_bin = topk_pick_bin(hi, limit, &above_hi);
        }
        for (uint32_t i = 0; i < n; i++)
            if ((uint32_t)(scores[i] >> 8) == hi_bin) lo[scores[i] & 255]++;
        c = topk_cut_by_score(hi_bin, above_hi, lo, limit, desc);
    }
    cut_out[0] = c.T; cut_out[1] = c.gt; cut_out[2] = c.ties; cut_out[3] = c.quota; cut_out[4] = c.lo; cut_out[5] = c.keep_all;
    uint32_t gt_before = 0, eq_before = 0, kept = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t s = scores[i];
        dest[i] = topk_dest(c, by_score, s, gt_before, eq_before);
        if (dest[i] != TOPK_NOT_KEPT) kept++;
        // the kernels' counters: records above T, records at T (every record when the order is by index; nothing is above T = 0 then)
        if (c.keep_all) eq_before++;
        else if (by_score && s > c.T) gt_before++;
        else if (!by_score || s == c.T) eq_before++;
    }
    return kept;
}

}  // extern "C"
