// TEST INFRASTRUCTURE: frizbee_amd/csrc/indices_union.h - the arithmetic of the fused multi-pattern top + matched-positions query's union
// step (the P-way merge of the patterns' descending position lists, the combined record and record count) - compiled for the host.  uh_union
// walks the head the way k_multi_union does, one record per "thread", with every decision taken by the header's functions; uh_check holds the
// combined records to the head with indices_pack.h's checks, as the pack kernels do.  tests/test_indices_union_host.py fuzzes both against numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "indices_pack.h"
#include "indices_union.h"

extern "C" {

uint32_t uh_by_value(void) { return IUNION_BY_VALUE; }

// P sources: recs[p] / counts[p] / npos[p] / pos[p] (strides[p] per record); head[head_count] records, max_records = the room of the head ->
// out[n] combined records, npos_u[n], pos_u[n * U], *out_count = the combined record count.  Returns n = the records walked.
uint32_t uh_union(uint32_t P, const IUnionRec* const* recs, const uint32_t* counts, const uint32_t* const* npos, const uint32_t* const* pos, const uint32_t* strides,
                  const IUnionRec* head, uint32_t head_count, uint32_t max_records, uint32_t U, IUnionRec* out, uint32_t* out_count, uint32_t* npos_u, uint32_t* pos_u) {
    std::vector<IUnionSrc> src(P);
    for (uint32_t p = 0; p < P; p++) src[p] = IUnionSrc{recs[p], &counts[p], npos[p], pos[p], strides[p], 0};
    const uint32_t n = head_count < max_records ? head_count : max_records;
    *out_count = iunion_count(src.data(), P, head_count);
    std::vector<uint32_t> cur(P + 1);
    for (uint32_t k = 0; k < n; k++) {
        out[k] = iunion_record(src.data(), P, k, head[k].index);
        npos_u[k] = iunion_merge(src.data(), P, k, cur.data(), pos_u + (size_t)k * U, U);
    }
    return n;
}

// the inconsistency word the pack step raises for (head, combined)
uint32_t uh_check(const IUnionRec* head, uint32_t head_count, const IUnionRec* comb, uint32_t comb_count, uint32_t n) {
    uint32_t bad = ipack_check_count(head_count, comb_count);
    for (uint32_t k = 0; k < n; k++) bad |= ipack_check_record(head[k].index, head[k].score, head[k].exact, comb[k].index, comb[k].score, comb[k].exact);
    return bad;
}

}  // extern "C"
