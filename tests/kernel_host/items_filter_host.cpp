// TEST INFRASTRUCTURE: frizbee_amd/csrc/items_filter.h - the per-item decision of the item-list filter for large candidate sets
// (k1_items_dfa) - compiled for the host, the automaton's step a plain lookup in a (rows + 1) x 256 table.
// tests/test_items_filter_host.py fuzzes it against the oracle's 0-typo prefilter and sig_filter.h's own signature builder.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "items_filter.h"

extern "C" {

int ifh_wants_row(int use_sig, uint32_t sig, uint32_t needle_sig_, uint32_t len, uint32_t min_len) { return items_wants_row(use_sig != 0, sig, needle_sig_, len, min_len) ? 1 : 0; }
uint32_t ifh_vecs(uint32_t len) { return items_vecs(len); }
uint32_t ifh_vec_bytes(uint32_t len, uint32_t v) { return items_vec_bytes(len, v); }
uint32_t ifh_sig_of_bytes(const uint8_t* p, size_t n) { return sig_of_bytes(p, n); }
uint32_t ifh_needle_sig(const uint8_t* p, size_t n) { return needle_sig(p, n); }
int ifh_sig_passes(uint32_t sig, uint32_t nsig) { return sig_passes(sig, nsig) ? 1 : 0; }
// one vector (four little-endian dwords), its first nbytes bytes
uint32_t ifh_chain_vec(uint32_t st, const uint32_t* w4, uint32_t nbytes, const uint8_t* dfa) {
    const uint32_t w[4] = {w4[0], w4[1], w4[2], w4[3]};
    return items_chain_vec(st, w, nbytes, [dfa](uint32_t s, uint32_t b) { return (uint32_t)dfa[(size_t)s * 256 + b]; });
}
// the whole decision; `row` has at least roundup16(len) readable bytes
int ifh_decide(int use_sig, uint32_t sig, uint32_t needle_sig_, const uint8_t* row, uint32_t len, uint32_t min_len, uint32_t acc_lo, const uint8_t* dfa) {
    return items_decide(use_sig != 0, sig, needle_sig_, row, len, min_len, acc_lo, [dfa](uint32_t s, uint32_t b) { return (uint32_t)dfa[(size_t)s * 256 + b]; }) ? 1 : 0;
}

}  // extern "C"
