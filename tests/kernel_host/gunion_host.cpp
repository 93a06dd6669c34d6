// TEST INFRASTRUCTURE: frizbee_amd/csrc/indices_union_groups.h - the arithmetic of the grouped top + matched-positions query's union step
// (rows through the `where` maps, the carrier of a term, the combined record and record count, the merge over the carriers' lists) - compiled
// for the host without any HIP header.  gh_union walks the head the way k_gunion_merge does, one record per "thread", with every decision taken
// by the header's functions; gh_where fills the maps the way k_gunion_slots + k_gunion_where do; gh_check holds the combined records to the head
// with indices_pack.h's checks, as the pack kernels do.  tests/test_indices_union_groups_host.py fuzzes them against numpy.
#include <stdint.h>

#include <vector>

#include "indices_pack.h"
#include "indices_union_groups.h"

extern "C" {

uint32_t gh_by_value(void) { return IUNION_BY_VALUE; }
uint32_t gh_absent(void) { return GUNION_ABSENT; }

static std::vector<GUnionSrc> sources(uint32_t P, const IUnionRec* const* recs, const uint32_t* counts, const uint32_t* const* npos, const uint32_t* const* pos, const uint32_t* strides,
                                      const uint32_t* const* where, const uint32_t* terms) {
    std::vector<GUnionSrc> src(P);
    for (uint32_t p = 0; p < P; p++) src[p] = GUnionSrc{IUnionSrc{recs[p], &counts[p], npos[p], pos[p], strides[p], 0}, where[p], terms[p], 0};
    return src;
}

// the maps of the sources that have one: slot[head[k].index] = k, then where_p[slot[rec_p[j].index]] = j + 1 (where_p: n words, cleared here)
void gh_where(uint32_t P, const IUnionRec* const* recs, const uint32_t* counts, uint32_t* const* where, const IUnionRec* head, uint32_t n, uint32_t n_hay) {
    std::vector<uint32_t> slot(n_hay, 0xDEADBEEFu);  // (never cleared on the device either)
    for (uint32_t k = 0; k < n; k++) slot[head[k].index] = k;
    for (uint32_t p = 0; p < P; p++) {
        if (!where[p]) continue;
        for (uint32_t k = 0; k < n; k++) where[p][k] = 0;
        for (uint32_t j = 0; j < counts[p] && j < n; j++) {
            const uint32_t h = recs[p][j].index;
            if (h >= n_hay) continue;
            const uint32_t k = slot[h];
            if (k < n && head[k].index == h) where[p][k] = j + 1;
        }
    }
}

// P sources (where[p] null: a plain pattern) -> out[n] combined records, npos_u[n], pos_u[n * U], *out_count; carrier_of[n * P]: per record and
// source index b of a term's first source, the term's carrier (the term's end when none is present), 0xFFFFFFFF elsewhere.  Returns n.
uint32_t gh_union(uint32_t P, const IUnionRec* const* recs, const uint32_t* counts, const uint32_t* const* npos, const uint32_t* const* pos, const uint32_t* strides,
                  const uint32_t* const* where, const uint32_t* terms, const IUnionRec* head, uint32_t head_count, uint32_t max_records, uint32_t U, IUnionRec* out, uint32_t* out_count,
                  uint32_t* npos_u, uint32_t* pos_u, uint32_t* carrier_of) {
    const std::vector<GUnionSrc> src = sources(P, recs, counts, npos, pos, strides, where, terms);
    const uint32_t n = head_count < max_records ? head_count : max_records;
    *out_count = gunion_count(src.data(), P, head_count);
    std::vector<uint32_t> carrier(P + 1), row(P + 1), cur(P + 1);
    for (uint32_t k = 0; k < n; k++) {
        bool missing = false;
        const uint32_t T = gunion_carriers(src.data(), P, k, carrier.data(), row.data(), &missing);
        out[k] = gunion_record_of(src.data(), T, carrier.data(), row.data(), missing, head[k].index);
        const IUnionRec again = gunion_record(src.data(), P, k, head[k].index);  // the two forms of the record agree
        if (again.index != out[k].index || again.score != out[k].score || again.exact != out[k].exact) out[k].index = 0x7FFFFFFFu;
        npos_u[k] = gunion_merge(src.data(), T, carrier.data(), row.data(), cur.data(), pos_u + (size_t)k * U, U);
        for (uint32_t b = 0; b < P;) {
            const uint32_t e = gunion_term_end(src.data(), P, b);
            carrier_of[(size_t)k * P + b] = gunion_carrier(src.data(), b, e, k, nullptr);
            for (uint32_t p = b + 1; p < e; p++) carrier_of[(size_t)k * P + p] = 0xFFFFFFFFu;
            b = e;
        }
    }
    return n;
}

uint32_t gh_check(const IUnionRec* head, uint32_t head_count, const IUnionRec* comb, uint32_t comb_count, uint32_t n) {
    uint32_t bad = ipack_check_count(head_count, comb_count);
    for (uint32_t k = 0; k < n; k++) bad |= ipack_check_record(head[k].index, head[k].score, head[k].exact, comb[k].index, comb[k].score, comb[k].exact);
    return bad;
}

}  // extern "C"
