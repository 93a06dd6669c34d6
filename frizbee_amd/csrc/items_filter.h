// The per-item decision of the item-list filter for LARGE candidate sets (k1_items_dfa, kernels_filter.hip): the 0-typo ASCII accept test of
// a fuzzy query - the ordered-subsequence automaton k1_dfa runs over a contiguous range - for ONE haystack of an item list.  Plain functions
// for the device AND the host: the kernel calls them with its LDS lookup as `step`, tests/kernel_host/items_filter_host.cpp compiles them for
// the CPU with a table lookup and tests/test_items_filter_host.py fuzzes the decision against the oracle's prefilter.
//
// The reference has no counterpart (its `match_list` always walks the whole slice); the decision itself is its 0-typo prefilter
// (src/prefilter/algo/mod.rs): every needle byte occurs, in order, either case - and the haystack is at least min_haystack_len long.
//   * the signature pre-test (sig_filter.h, a list with signatures and an eligible needle): a row whose letter signature lacks a needle
//     letter cannot be accepted, so its bytes are never requested;
//   * the length test: k1_dfa's `L >= min_len`;
//   * the chain over a row's 16-byte vectors: vector v holds items_vec_bytes(len, v) bytes of the row - 16 but for the tail's -, and only
//     those go through the automaton (what follows a row in the padded-16 layout is never looked at, so a NUL byte inside a row and the
//     zero fill behind it cannot be confused).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FZB_ITEMS_FN __host__ __device__ __forceinline__
#else
#define FZB_ITEMS_FN inline
#ifndef FZB_SIG_FN
#define FZB_SIG_FN inline
#endif
#endif
#include "sig_filter.h"

// is the row requested at all?  use_sig: the list has signatures and the needle is eligible (fzb_filter_sig_applies)
FZB_ITEMS_FN bool items_wants_row(bool use_sig, uint32_t sig, uint32_t needle_sig, uint32_t len, uint32_t min_len) {
    return len >= min_len && (!use_sig || sig_passes(sig, needle_sig));
}
// 16-byte vectors of a row of `len` bytes, and how many of vector v's bytes belong to the row (0 beyond the last)
FZB_ITEMS_FN uint32_t items_vecs(uint32_t len) { return (len + 15u) >> 4; }
FZB_ITEMS_FN uint32_t items_vec_bytes(uint32_t len, uint32_t v) { return len > 16u * v ? (len - 16u * v < 16u ? len - 16u * v : 16u) : 0u; }
// the first `nbytes` (<= 16) bytes of one vector, given as its four little-endian dwords, through the automaton: step(state, byte) -> state
template <class Step>
FZB_ITEMS_FN uint32_t items_chain_vec(uint32_t st, const uint32_t (&w)[4], uint32_t nbytes, Step step) {
    for (uint32_t k = 0; k < nbytes; k++) st = step(st, (w[k >> 2] >> (8u * (k & 3u))) & 0xFFu);
    return st;
}
// the whole decision for a row in memory (the host model; the kernel's ragged loop is this loop with the next vector requested one ahead):
// start state 0, accept in the states >= acc_lo
template <class Step>
FZB_ITEMS_FN bool items_decide(bool use_sig, uint32_t sig, uint32_t needle_sig, const uint8_t* row, uint32_t len, uint32_t min_len, uint32_t acc_lo, Step step) {
    if (!items_wants_row(use_sig, sig, needle_sig, len, min_len)) return false;
    uint32_t st = 0;
    for (uint32_t v = 0; v < items_vecs(len); v++) {
        const uint32_t nb = items_vec_bytes(len, v);
        uint32_t w[4] = {0, 0, 0, 0};
        for (uint32_t k = 0; k < nb; k++) w[k >> 2] |= (uint32_t)row[16u * v + k] << (8u * (k & 3u));
        st = items_chain_vec(st, w, nb, step);
    }
    return st >= acc_lo;
}
