// TEST INFRASTRUCTURE: the REPEAT signature of frizbee_amd/csrc/sig_filter.h - which signature bits a haystack / a needle holds at least
// twice, the reference transposition of the repeat planes and the candidates under both tests - compiled for the host.
// tests/test_sig_repeat_host.py checks it against plain Python counts.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sig_filter.h"

extern "C" {

uint32_t sr_sig_of_bytes(const uint8_t* p, size_t n) { return sig_of_bytes(p, n); }
uint32_t sr_sig2_of_bytes(const uint8_t* p, size_t n) { return sig2_of_bytes(p, n); }
uint32_t sr_sig2_of_words(const uint32_t* w, size_t n) {  // the device build's way: four bytes at a time
    uint32_t once = 0, twice = 0;
    for (size_t i = 0; i < n; i++) sig2_accum_word(w[i], once, twice);
    return twice;
}
uint32_t sr_needle_sig(const uint8_t* p, size_t n) { return needle_sig(p, n); }
uint32_t sr_needle_sig2(const uint8_t* p, size_t n) { return needle_sig2(p, n); }
int sr_passes(uint32_t sig, uint32_t sig2, uint32_t nsig, uint32_t nsig2) { return sig2_passes(sig, sig2, nsig, nsig2) ? 1 : 0; }
void sr_transpose(const uint32_t* sig2, uint64_t n, uint64_t* planes2) { sig_planes2_transpose_ref(sig2, n, planes2); }
uint64_t sr_candidates(const uint64_t* planes, const uint64_t* planes2, uint64_t tile, uint32_t word, uint32_t nsig, uint32_t nsig2) {
    return sig_plane_candidates2(planes, planes2, tile, word, nsig, nsig2);
}

}  // extern "C"
