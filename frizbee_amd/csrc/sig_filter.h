// The LETTER SIGNATURE of a haystack: one u32 that says which letters (either case) and which classes of other bytes occur in it.
// It depends on the haystack alone, so a resident list computes it once (k_sig_build, host_upload.hip) and every 0-typo ASCII query
// reads 4 bytes per haystack to learn which rows CAN match before it touches their 32 (k1_dfa_sig, kernels_filter.hip).
//
// The one property everything rests on: the ordered-subsequence automaton of an eligible needle advances on byte b only if b is a needle
// byte or its ASCII case flip, and both have the same sig_bit.  So   accepted  =>  (sig & needle_sig) == needle_sig.
// The converse does not hold (order, repeats, bytes that share a bit): every row the signature passes still goes through the automaton.
//
// Pure functions, host and device: tests/test_signature_host.py compiles this header for the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef FZB_SIG_FN
#define FZB_SIG_FN __host__ __device__ inline
#endif

// 0..25: the letter's index, either case; 26..31: every other non-zero byte, by b % 6.  (Call with b != 0: a zero byte sets no bit.)
FZB_SIG_FN uint32_t sig_bit(uint32_t b) {
    const uint32_t l = (b | 0x20u) - 'a';
    return l < 26u ? l : 26u + b % 6u;
}
FZB_SIG_FN uint32_t sig_of_byte(uint32_t b) { return b ? 1u << sig_bit(b) : 0u; }
FZB_SIG_FN uint32_t sig_of_word(uint32_t w) { return sig_of_byte(w & 0xFF) | sig_of_byte((w >> 8) & 0xFF) | sig_of_byte((w >> 16) & 0xFF) | sig_of_byte(w >> 24); }
FZB_SIG_FN uint32_t sig_of_bytes(const uint8_t* p, size_t n) {
    uint32_t s = 0;
    for (size_t i = 0; i < n; i++) s |= sig_of_byte(p[i]);
    return s;
}
FZB_SIG_FN uint32_t needle_sig(const uint8_t* needle, size_t n) { return sig_of_bytes(needle, n); }
// the test itself: may a haystack with signature `sig` be accepted by the needle with signature `nsig`?  (k1_dfa_sig, k1_items_dfa)
FZB_SIG_FN bool sig_passes(uint32_t sig, uint32_t nsig) { return (sig & nsig) == nsig; }

// The queries the signature may decide for: fuzzy matching with max_typos = 0 (the stream stage is the ordered-subsequence automaton) of
// an ASCII needle without a NUL byte.  literal_mode: 0 = fuzzy (fzb_config::matching).
FZB_SIG_FN bool needle_sig_eligible(const uint8_t* needle, size_t n, int max_typos, int literal_mode) {
    if (literal_mode != 0 || max_typos != 0 || n == 0) return false;
    for (size_t i = 0; i < n; i++)
        if (needle[i] == 0 || needle[i] >= 0x80) return false;
    return true;
}

// The signatures a SECOND time, transposed into BIT-PLANES: one 64-bit word per (tile of 1024 haystacks, signature bit, 64 haystacks).
// Bit i of word w of plane b of tile t = bit b of the signature of item 1024 t + 64 w + i, zero at and beyond the corpus' item count.
// Tile-major: a (tile, bit) is one 128-byte line, a tile is 4 KB (the same 4 bytes per haystack as the u32 array).  A query ANDs the
// planes of its needle's letters: 16 words per tile and letter are the tile's candidates, ready-made (k1_dfa_sig's plane form).
#define FZB_SIG_PLANE_TILE 1024u
#define FZB_SIG_PLANE_WORDS 16u  // 64-bit words per (tile, bit)
FZB_SIG_FN uint64_t sig_plane_tiles(uint64_t n_items) { return (n_items + FZB_SIG_PLANE_TILE - 1) / FZB_SIG_PLANE_TILE; }
FZB_SIG_FN uint64_t sig_plane_words(uint64_t n_items) { return sig_plane_tiles(n_items) * 32u * FZB_SIG_PLANE_WORDS; }
FZB_SIG_FN uint64_t sig_plane_index(uint64_t tile, uint32_t bit, uint32_t word) { return (tile * 32u + bit) * FZB_SIG_PLANE_WORDS + word; }
// valid bits of word w of tile t in a list (or range) of `count` items: the mask the filter applies, and what the build leaves set
FZB_SIG_FN uint64_t sig_plane_valid(uint64_t tile, uint32_t word, uint64_t count) {
    const uint64_t base = tile * FZB_SIG_PLANE_TILE + 64u * word;
    return base >= count ? 0ull : count - base >= 64u ? ~0ull : (1ull << (count - base)) - 1ull;
}
// reference transposition (host tests; the device build is k_sig_planes_build): planes holds sig_plane_words(n) words
FZB_SIG_FN void sig_planes_transpose_ref(const uint32_t* sig, uint64_t n, uint64_t* planes) {
    const uint64_t words = sig_plane_words(n);
    for (uint64_t k = 0; k < words; k++) planes[k] = 0;
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t b = 0; b < 32; b++)
            if ((sig[i] >> b) & 1u) planes[sig_plane_index(i / FZB_SIG_PLANE_TILE, b, (uint32_t)(i % FZB_SIG_PLANE_TILE) / 64u)] |= 1ull << (i % 64u);
}
// the candidates of word w of tile t for a needle: the AND of its letters' planes (nsig != 0); bit i set <=> sig_passes(sig[item], nsig)
FZB_SIG_FN uint64_t sig_plane_candidates(const uint64_t* planes, uint64_t tile, uint32_t word, uint32_t nsig) {
    uint64_t c = ~0ull;
    for (uint32_t m = nsig; m; m &= m - 1u) c &= planes[sig_plane_index(tile, (uint32_t)__builtin_ctz(m), word)];
    return c;
}
// The REPEAT SIGNATURE: which signature bits occur at least TWICE.  An accepted haystack holds the needle's bytes (or their case flips) at
// DISTINCT positions, and a byte and its flip share a bit, so with c_n(b) / c_h(b) = the needle's / haystack's non-zero bytes of bit b
//   accepted  =>  c_h(b) >= min(c_n(b), 2) for every b  <=>  (sig & nsig) == nsig && (sig2 & nsig2) == nsig2
// - the same letter twice (`deadbe`), a letter and its flip (`dD`), two bytes of one other-byte class (`1` and `7`).  The u32 signature
// does not carry counts: the repeat signature is made from the haystack's bytes (within its length) and kept as bit-planes only
// (CorpusDev::sig_planes2, k_sig_planes2_build).  "At least three" (`deadbeef` has three `e`) is not built: counts cap at two.
FZB_SIG_FN void sig2_accum_byte(uint32_t b, uint32_t& once, uint32_t& twice) {
    const uint32_t s = sig_of_byte(b);
    twice |= once & s;
    once |= s;
}
FZB_SIG_FN void sig2_accum_word(uint32_t w, uint32_t& once, uint32_t& twice) {
    sig2_accum_byte(w & 0xFF, once, twice);
    sig2_accum_byte((w >> 8) & 0xFF, once, twice);
    sig2_accum_byte((w >> 16) & 0xFF, once, twice);
    sig2_accum_byte(w >> 24, once, twice);
}
// repeat signature of a haystack (its n bytes; zero bytes count for nothing): bit b set <=> c_h(b) >= 2
FZB_SIG_FN uint32_t sig2_of_bytes(const uint8_t* p, size_t n) {
    uint32_t once = 0, twice = 0;
    for (size_t i = 0; i < n; i++) sig2_accum_byte(p[i], once, twice);
    return twice;
}
// repeat signature of a needle: bit b set <=> c_n(b) >= 2.  0 for a needle without a repeat: the filter then reads no repeat plane.
FZB_SIG_FN uint32_t needle_sig2(const uint8_t* needle, size_t n) { return sig2_of_bytes(needle, n); }
FZB_SIG_FN bool sig2_passes(uint32_t sig, uint32_t sig2, uint32_t nsig, uint32_t nsig2) { return sig_passes(sig, nsig) && (sig2 & nsig2) == nsig2; }
// reference transposition of the repeat planes (the layout of the planes above; the device build is k_sig_planes2_build)
FZB_SIG_FN void sig_planes2_transpose_ref(const uint32_t* sig2, uint64_t n, uint64_t* planes2) { sig_planes_transpose_ref(sig2, n, planes2); }
// the candidates under both tests: bit i set <=> sig2_passes(sig[item], sig2[item], nsig, nsig2)  (nsig != 0; planes2 is not read when nsig2 == 0)
FZB_SIG_FN uint64_t sig_plane_candidates2(const uint64_t* planes, const uint64_t* planes2, uint64_t tile, uint32_t word, uint32_t nsig, uint32_t nsig2) {
    uint64_t c = sig_plane_candidates(planes, tile, word, nsig);
    for (uint32_t m = nsig2; m; m &= m - 1u) c &= planes2[sig_plane_index(tile, (uint32_t)__builtin_ctz(m), word)];
    return c;
}

// Tiles of one batch of the plane form (a workgroup's run is taken in batches of at most this many tiles; one batch covers the run of 5
// that 10 M haystacks give on 256 compute units)
#ifndef FZB_SIG_BATCH_TILES
#define FZB_SIG_BATCH_TILES 8u
#endif

// Tiles of k1_dfa_sig with more passing rows than this stream the whole tile (coalesced loads, four chains per thread) instead of
// gathering the passing rows one chain per thread.
#ifndef FZB_SIG_GATHER_MAX
#define FZB_SIG_GATHER_MAX 384u
#endif
