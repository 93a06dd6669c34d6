// TEST INFRASTRUCTURE: frizbee_amd/csrc/sig_filter.h - the letter signature of a haystack, of a needle, and which needles may use it -
// compiled for the host.  tests/test_signature_host.py checks it against a plain Python restatement and the oracle's 0-typo prefilter.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "sig_filter.h"

extern "C" {

uint32_t sh_sig_bit(uint32_t b) { return sig_bit(b); }
uint32_t sh_sig_of_byte(uint32_t b) { return sig_of_byte(b); }
uint32_t sh_sig_of_bytes(const uint8_t* p, size_t n) { return sig_of_bytes(p, n); }
uint32_t sh_sig_of_word(uint32_t w) { return sig_of_word(w); }
uint32_t sh_needle_sig(const uint8_t* p, size_t n) { return needle_sig(p, n); }
int sh_eligible(const uint8_t* p, size_t n, int max_typos, int literal_mode) { return needle_sig_eligible(p, n, max_typos, literal_mode) ? 1 : 0; }
uint32_t sh_gather_max(void) { return FZB_SIG_GATHER_MAX; }

}  // extern "C"
