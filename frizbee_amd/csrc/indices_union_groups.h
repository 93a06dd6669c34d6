// Union step of the fused "top + matched positions" query of a matcher that has an any-of group (`a | b`, anyof.h): the arithmetic, as plain
// functions for the device AND the host (k_gunion_merge in kernels_indices.hip calls them; tests/kernel_host/gunion_host.cpp compiles them for
// the CPU and tests/test_indices_union_groups_host.py fuzzes them against numpy).
//
// indices_union.h puts the positive patterns' traced records together under one assumption: every pattern matches every record of the head, so
// pattern p's traced record of head record k sits at row k.  An alternative of a group need not match: its traced pass over the head's items
// returns only the items it hits, and row k of its buffers is not head record k.  So a source here is an IUnionSrc plus
//   where: null for a plain pattern (the row is k); for an alternative a map from the head position k to the traced row + 1, 0 = the
//          alternative does not match head record k;
//   term:  the term of the query the source belongs to; the sources of one term are adjacent.
//
// The CARRIER of a term for head record k is, among its sources that are present at k, the one with the largest key
// anyof_pack(score, exact) = score << 1 | exact (anyof.h: the key whose maximum IS the group's record), the first in query order on equal
// keys.  A plain pattern is a term of one source and carries itself.  The carrier's record is the term's record - its exact flag equals the
// group's, because the key maximum prefers a set flag at equal scores - and ONLY the carrier's positions enter the union: an alternative that
// matches but does not carry contributes nothing.  The records add over the terms with saturation and the exact flags OR, as in
// indices_union.h; the positions are the same strictly descending union without repeats (`match_one_indices_multi`, reference
// src/matcher/multi.rs:56-82), each carrier's list read at its own row.
//
// Bounds, as indices_union.h argues them: every value written is smaller than the one before, every round of the merge moves a cursor, and no
// more than the carriers' lengths together - at most U_g = the plain patterns' strides + per group the largest stride among its alternatives -
// are written; never more than `cap`.
//
// The combined record is held to the head by the pack step's existing checks (indices_pack.h): a term with no present source, or a carrier
// whose record carries another index than the head's, gives the complement of the head's index (IPACK_BAD_RECORD); a plain pattern whose
// traced pass produced another number of records than the head has, or an alternative that produced more, gives that number as the combined
// count (IPACK_BAD_COUNT).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "anyof.h"
#include "indices_union.h"

#define GUNION_ABSENT 0xFFFFFFFFu  // gunion_row: the source does not match this head record

struct GUnionSrc {
    IUnionSrc s;
    const uint32_t* where;  // null: a plain pattern, the row is k; else head position -> traced row + 1, 0 = absent
    uint32_t term;          // sources of one term are adjacent
    uint32_t _pad;
};

// the row of source p that holds head record k, or GUNION_ABSENT
IUNION_HD uint32_t gunion_row(const GUnionSrc* src, uint32_t p, uint32_t k) {
    if (!src[p].where) return k;
    return src[p].where[k] - 1u;  // (0 - 1 == GUNION_ABSENT)
}

// the end of the term that begins at source b
IUNION_HD uint32_t gunion_term_end(const GUnionSrc* src, uint32_t P, uint32_t b) {
    uint32_t e = b + 1;
    while (e < P && src[e].term == src[b].term) e++;
    return e;
}

// Over the sources [b, e) of one term: the source with the largest key among those present at head record k, the first on a tie; e when none
// is present.  *row: the carrier's row.
IUNION_HD uint32_t gunion_carrier(const GUnionSrc* src, uint32_t b, uint32_t e, uint32_t k, uint32_t* row) {
    uint32_t best = e, best_key = 0;
    for (uint32_t p = b; p < e; p++) {
        const uint32_t r = gunion_row(src, p, k);
        if (r == GUNION_ABSENT) continue;
        const IUnionRec rec = src[p].s.rec[r];
        const uint32_t key = anyof_pack(rec.score, rec.exact);  // (never 0: ANYOF_HIT is set)
        if (key > best_key) {
            best = p;
            best_key = key;
            if (row) *row = r;
        }
    }
    return best;
}

// The carriers of head record k, one per term that has a present source, in query order: carrier[t] = the source, row[t] = its row.  Returns
// their number (<= P); *missing = a term had no present source.
IUNION_HD uint32_t gunion_carriers(const GUnionSrc* src, uint32_t P, uint32_t k, uint32_t* carrier, uint32_t* row, bool* missing) {
    uint32_t T = 0;
    bool miss = false;
    for (uint32_t b = 0; b < P;) {
        const uint32_t e = gunion_term_end(src, P, b);
        uint32_t r = 0;
        const uint32_t c = gunion_carrier(src, b, e, k, &r);
        if (c == e) miss = true;
        else {
            carrier[T] = c;
            row[T] = r;
            T++;
        }
        b = e;
    }
    if (missing) *missing = miss;
    return T;
}

// The combined record of head record k from its T carriers: the saturating sum, the OR of the exact flags, the head's index - or its complement
// when a term is missing or a carrier's record carries another index.  No source at all: the head's index, 0, 0.
IUNION_HD IUnionRec gunion_record_of(const GUnionSrc* src, uint32_t T, const uint32_t* carrier, const uint32_t* row, bool missing, uint32_t head_index) {
    IUnionRec o;
    o._pad = 0;
    uint32_t sum = 0, exact = 0;
    bool same = !missing;
    for (uint32_t t = 0; t < T; t++) {
        const IUnionRec r = src[carrier[t]].s.rec[row[t]];
        same = same && r.index == head_index;
        sum = iunion_add_score(sum, r.score);
        exact |= r.exact != 0;
    }
    o.index = same ? head_index : ~head_index;
    o.score = (uint16_t)sum;
    o.exact = (uint8_t)exact;
    return o;
}

// the same from the sources alone (P <= IUNION_BY_VALUE x ANYOF_ALTS_MAX is not required: the carriers are found term by term)
IUNION_HD IUnionRec gunion_record(const GUnionSrc* src, uint32_t P, uint32_t k, uint32_t head_index) {
    IUnionRec o;
    o._pad = 0;
    uint32_t sum = 0, exact = 0;
    bool same = true;
    for (uint32_t b = 0; b < P;) {
        const uint32_t e = gunion_term_end(src, P, b);
        uint32_t row = 0;
        const uint32_t c = gunion_carrier(src, b, e, k, &row);
        if (c == e) same = false;
        else {
            const IUnionRec r = src[c].s.rec[row];
            same = same && r.index == head_index;
            sum = iunion_add_score(sum, r.score);
            exact |= r.exact != 0;
        }
        b = e;
    }
    o.index = same ? head_index : ~head_index;
    o.score = (uint16_t)sum;
    o.exact = (uint8_t)exact;
    return o;
}

// The combined record count: the head's, unless a plain pattern's traced pass produced another number of records or an alternative's more than
// the head has - then the first such number.
IUNION_HD uint32_t gunion_count(const GUnionSrc* src, uint32_t P, uint32_t head_count) {
    for (uint32_t p = 0; p < P; p++) {
        const uint32_t c = src[p].s.count[0];
        if (src[p].where ? c > head_count : c != head_count) return c;
    }
    return head_count;
}

// The union of the T carriers' lists into out[0 .. cap): iunion_merge's P-way descending merge, each list read at its own row; returns its
// length.  cur[0 .. T): the cursors.
IUNION_HD uint32_t gunion_merge(const GUnionSrc* src, uint32_t T, const uint32_t* carrier, const uint32_t* row, uint32_t* cur, uint32_t* out, uint32_t cap) {
    for (uint32_t t = 0; t < T; t++) cur[t] = 0;
    uint32_t n = 0, last = 0;
    while (n < cap) {
        uint32_t best = 0;
        bool found = false;
        for (uint32_t t = 0; t < T; t++) {
            const IUnionSrc& s = src[carrier[t]].s;
            const uint32_t len = iunion_len(s.npos[row[t]], s.stride);
            const uint32_t* list = s.pos + (size_t)row[t] * s.stride;
            uint32_t c = cur[t];
            while (n && c < len && list[c] >= last) c++;  // taken already (from this list or as another one's equal)
            cur[t] = c;
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
