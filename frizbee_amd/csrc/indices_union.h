// Union step of the fused multi-pattern "top + matched positions" query: the arithmetic, as plain functions for the device AND the host
// (k_multi_union in kernels_indices.hip calls them; tests/kernel_host/union_host.cpp compiles them for the CPU and
// tests/test_indices_union_host.py fuzzes them against numpy).
//
// `match_one_indices_multi` (reference src/matcher/multi.rs:56-82): every non-negated pattern must match, the scores add with saturation, the
// exact flags OR, and the patterns' matched positions are put together, "reported in reverse order, and patterns may share matched chars":
// one strictly descending list without repeats.  Behind the multi top stage every positive pattern p runs the traced pipeline over the head's
// items and leaves, for head record k, a record rec_p[k] and min(npos_p[k], stride_p) positions at pos_p[k * stride_p ..].
//
// Each of these lists is STRICTLY DESCENDING already:
//   * the traced scorer's walk (trace_walk.h) reports position hidx + sp with hidx = col - SWL, and `col` never grows; after every reported
//     position the walk moves one column to the left (the match branch ends in `col--`), so the next one is smaller.  On the unicode path a
//     scalar's bytes are written from its last byte down to its first, and the next scalar reported starts in an earlier column;
//   * the literal modes write the needle's run from its last byte to its first (kernels_literal.hip: pos + (n - 1 - k)).
// So the union is a P-way merge over one cursor per list that takes the largest head and steps over values it has taken already.  The merge
// does not rely on the order for its bounds: every value written is smaller than the one before, every round moves a cursor, and no more
// than the lists' lengths together - at most U = sum of the strides - are written.
//
// The combined record is held to the head by the pack step's existing checks (indices_pack.h): patterns that do not agree on `index` give an
// index the head's record cannot have (IPACK_BAD_RECORD), a pattern whose traced pass produced another number of records than the head has
// gives that number as the combined count (IPACK_BAD_COUNT).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IUNION_HD __host__ __device__ __forceinline__
#else
#define IUNION_HD inline
#endif

#define IUNION_BY_VALUE 8  // sources a launch carries in its argument block; a matcher with more keeps them (and the cursors) in device memory

struct IUnionRec {  // fzb_match_rec
    uint32_t index;
    uint16_t score;
    uint8_t exact;
    uint8_t _pad;
};

// one positive pattern's traced pass: its records in head order and their number, the position counts, the strided positions
struct IUnionSrc {
    const IUnionRec* rec;
    const uint32_t* count;
    const uint32_t* npos;
    const uint32_t* pos;
    uint32_t stride;
    uint32_t _pad;
};

IUNION_HD uint32_t iunion_len(uint32_t npos, uint32_t stride) { return npos < stride ? npos : stride; }

// saturating u16 sum (`score.saturating_add`, multi.rs:45, 70; k_join_add of the multi stage)
IUNION_HD uint32_t iunion_add_score(uint32_t sum, uint32_t score) {
    const uint32_t s = sum + score;
    return s > 0xFFFFu ? 0xFFFFu : s;
}

// The combined traced record of head record k, whose index is head_index: the saturating sum, the OR of the exact flags, the patterns' common
// index - or, when they do not all carry the same one, the complement of the head's.  No positive pattern: the head's index, 0, 0.
IUNION_HD IUnionRec iunion_record(const IUnionSrc* src, uint32_t P, uint32_t k, uint32_t head_index) {
    IUnionRec o;
    o.index = head_index;
    o.score = 0;
    o.exact = 0;
    o._pad = 0;
    uint32_t sum = 0, exact = 0;
    bool same = true;
    for (uint32_t p = 0; p < P; p++) {
        const IUnionRec r = src[p].rec[k];
        if (p == 0) o.index = r.index;
        else same = same && r.index == o.index;
        sum = iunion_add_score(sum, r.score);
        exact |= r.exact != 0;
    }
    if (!same) o.index = ~head_index;
    o.score = (uint16_t)sum;
    o.exact = (uint8_t)exact;
    return o;
}

// The combined record count: the head's when every pattern's traced pass produced as many, else the first one that differs.
IUNION_HD uint32_t iunion_count(const IUnionSrc* src, uint32_t P, uint32_t head_count) {
    for (uint32_t p = 0; p < P; p++)
        if (src[p].count[0] != head_count) return src[p].count[0];
    return head_count;
}

// The union of head record k's P lists into out[0 .. cap): strictly descending, no repeats; returns its length.  cur[0 .. P): the cursors.
IUNION_HD uint32_t iunion_merge(const IUnionSrc* src, uint32_t P, uint32_t k, uint32_t* cur, uint32_t* out, uint32_t cap) {
    for (uint32_t p = 0; p < P; p++) cur[p] = 0;
    uint32_t n = 0, last = 0;
    while (n < cap) {
        uint32_t best = 0;
        bool found = false;
        for (uint32_t p = 0; p < P; p++) {
            const uint32_t len = iunion_len(src[p].npos[k], src[p].stride);
            const uint32_t* list = src[p].pos + (size_t)k * src[p].stride;
            uint32_t c = cur[p];
            while (n && c < len && list[c] >= last) c++;  // taken already (from this list or as another one's equal)
            cur[p] = c;
            if (c < len && (!found || list[c] > best)) {
                best = list[c];
                found = true;
            }
        }
        if (!found) break;
        out[n++] = best;
        last = best;
    }
    return n;
}
