// TEST INFRASTRUCTURE: frizbee_amd/csrc/indices_pack.h - the arithmetic of the fused top + matched-positions query's packing step (clamped
// lengths, the per-share / per-tile decomposition of the exclusive scan, the owner of a dense position, the check of the traced records
// against the head) - compiled for the host.  ph_pack walks the records the way kernels_indices.hip does: shares of IPACK_SHARE records,
// IPACK_TILE / IPACK_SHARE shares per tile, one tile directly or tile sums -> scan of the sums -> per-tile scatter, with every decision taken
// by the header's functions.  tests/test_indices_pack_host.py fuzzes it against numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "indices_pack.h"

extern "C" {

struct ph_rec {  // == fzb_match (head / traced records)
    uint32_t index;
    uint16_t score;
    uint8_t exact;
    uint8_t pad;
};
struct ph_out {  // == fzb_match_indices
    uint32_t index;
    uint16_t score;
    uint8_t exact;
    uint8_t pad;
    uint32_t positions_begin;
    uint32_t positions_len;
};

uint32_t ph_tile(void) { return IPACK_TILE; }

// head[head_count] / traced[traced_count] records, npos / pos (stride per record) of the traced pass, max_records = what the launcher
// sizes its decomposition from (<= IPACK_TILE: one tile) -> out[head_count], dense[], counts[4] = {records, found (passed through),
// position dwords, inconsistency word}.  Returns the number of tiles walked.
uint32_t ph_pack(const ph_rec* head, uint32_t head_count, uint32_t found, const ph_rec* traced, uint32_t traced_count, const uint32_t* npos, const uint32_t* pos, uint32_t stride,
                 uint32_t max_records, ph_out* out, uint32_t* dense, uint32_t* counts) {
    const uint32_t n = head_count < max_records ? head_count : max_records;
    const bool multi = max_records > IPACK_TILE;
    const uint32_t ntiles = ipack_ntiles(n);  // (one tile at most when max_records fits one: n <= max_records)
    const uint32_t shares = IPACK_TILE / IPACK_SHARE;
    uint32_t bad = ipack_check_count(head_count, traced_count);
    std::vector<uint32_t> tile_sum(ntiles + 1, 0), tile_off(ntiles + 1, 0);
    uint32_t begins[IPACK_SHARE];
    if (multi) {  // launches 1 and 2: tile sums, their exclusive scan
        for (uint32_t tile = 0; tile < ntiles; tile++) {
            uint32_t lo, hi;
            ipack_tile_range(tile, n, &lo, &hi);
            for (uint32_t t = 0; t < shares; t++) {
                const uint32_t first = lo + t * IPACK_SHARE < hi ? lo + t * IPACK_SHARE : hi;
                const uint32_t cnt = hi - first < IPACK_SHARE ? hi - first : IPACK_SHARE;
                tile_sum[tile] += ipack_scan_share(npos, first, cnt, stride, begins);
            }
        }
        uint32_t run = 0;
        for (uint32_t tile = 0; tile < ntiles; tile++) {
            tile_off[tile] = run;
            run += tile_sum[tile];
        }
        counts[2] = run;
    } else {
        counts[2] = 0;
    }
    std::vector<uint32_t> s_begin(IPACK_TILE);
    for (uint32_t tile = 0; tile < ntiles; tile++) {  // the scatter launch
        uint32_t lo, hi;
        ipack_tile_range(tile, n, &lo, &hi);
        const uint32_t base = multi ? tile_off[tile] : 0u;
        uint32_t before = 0;  // (the workgroup scan: shares in thread order)
        for (uint32_t t = 0; t < shares; t++) {
            const uint32_t first = lo + t * IPACK_SHARE < hi ? lo + t * IPACK_SHARE : hi;
            const uint32_t cnt = hi - first < IPACK_SHARE ? hi - first : IPACK_SHARE;
            const uint32_t mine = ipack_scan_share(npos, first, cnt, stride, begins);
            for (uint32_t r = 0; r < cnt; r++) {
                const uint32_t k = first + r;
                bad |= ipack_check_record(head[k].index, head[k].score, head[k].exact, traced[k].index, traced[k].score, traced[k].exact);
                s_begin[k - lo] = before + begins[r];
                out[k].index = head[k].index;
                out[k].score = head[k].score;
                out[k].exact = head[k].exact;
                out[k].pad = 0;
                out[k].positions_begin = base + before + begins[r];
                out[k].positions_len = ipack_len(npos[k], stride);
            }
            before += mine;
        }
        const uint32_t total = before;
        for (uint32_t d = 0; d < total; d++) {
            const uint32_t r = ipack_find_record(s_begin.data(), hi - lo, d);
            dense[base + d] = pos[(size_t)(lo + r) * stride + (d - s_begin[r])];
        }
        if (!multi) counts[2] = total;
    }
    counts[0] = n;
    counts[1] = found;
    counts[3] = bad;
    return ntiles;
}

}  // extern "C"
