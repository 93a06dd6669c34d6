// TEST INFRASTRUCTURE: the bit-plane layout of frizbee_amd/csrc/sig_filter.h - index function, reference transposition, valid-bit mask and
// the AND of a needle's planes - compiled for the host.  tests/test_sig_planes_host.py checks it against a plain Python transposition.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sig_filter.h"

extern "C" {

uint64_t sp_tiles(uint64_t n) { return sig_plane_tiles(n); }
uint64_t sp_words(uint64_t n) { return sig_plane_words(n); }
uint64_t sp_index(uint64_t tile, uint32_t bit, uint32_t word) { return sig_plane_index(tile, bit, word); }
uint64_t sp_valid(uint64_t tile, uint32_t word, uint64_t count) { return sig_plane_valid(tile, word, count); }
void sp_transpose(const uint32_t* sig, uint64_t n, uint64_t* planes) { sig_planes_transpose_ref(sig, n, planes); }
uint64_t sp_candidates(const uint64_t* planes, uint64_t tile, uint32_t word, uint32_t nsig) { return sig_plane_candidates(planes, tile, word, nsig); }
int sp_passes(uint32_t sig, uint32_t nsig) { return sig_passes(sig, nsig) ? 1 : 0; }
uint32_t sp_needle_sig(const uint8_t* p, size_t n) { return needle_sig(p, n); }
uint32_t sp_batch_tiles(void) { return FZB_SIG_BATCH_TILES; }

}  // extern "C"
