// Any-of groups of the query syntax (`a | b`): the arithmetic of a group, as plain functions for the device AND the host
// (kernels_multi.hip calls them; tests/kernel_host/anyof_host.cpp compiles them for the CPU and tests/test_anyof_host.py fuzzes them
// against numpy).
//
// The reference has no such operator.  A group G of 2..ANYOF_ALTS_MAX non-negated alternatives matches a haystack h iff at least one
// alternative matches h; score_G(h) is the maximum of the matching alternatives' scores and exact_G(h) the OR of the `exact` flags of the
// alternatives whose score equals that maximum.  Packed as  key = 0x80000000 | score << 1 | exact  that rule IS the unsigned maximum of
// the keys: a larger score wins whatever the flags, at equal scores a set flag wins.  max is commutative and associative, so the result
// does not depend on the alternatives' order.  Key 0 means "no alternative hit this haystack" (every real key has bit 31 set).
//
// On the device there is one u32 slot per candidate position: cleared once per group, folded after every alternative's pipeline
// (anyof_fold: read, max, write - the alternatives are serialised by the stream and one alternative hits a position at most once, so no
// atomics), and kept by tile_compact.h's flag + compact pass where the slot is non-zero.  In the composition the group then behaves as
// one non-negated pattern with those hits: anyof_join is k_join_add's arithmetic (saturating u16 sum, exact flags ORed).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FZB_ANYOF_FN __host__ __device__ __forceinline__
#else
#define FZB_ANYOF_FN inline
#endif

#define ANYOF_ALTS_MAX 8  // == FZB_GROUP_ALTS_MAX (include/frizbee_hip.h)
#define ANYOF_HIT 0x80000000u

FZB_ANYOF_FN uint32_t anyof_pack(uint32_t score, uint32_t exact) { return ANYOF_HIT | ((score & 0xFFFFu) << 1) | (exact ? 1u : 0u); }
FZB_ANYOF_FN uint32_t anyof_combine(uint32_t a, uint32_t b) { return a > b ? a : b; }
FZB_ANYOF_FN bool anyof_hit(uint32_t key) { return key != 0; }
FZB_ANYOF_FN uint32_t anyof_score(uint32_t key) { return (key >> 1) & 0xFFFFu; }
FZB_ANYOF_FN uint32_t anyof_exact(uint32_t key) { return key & 1u; }

// one alternative's hit folded into its slot
FZB_ANYOF_FN void anyof_fold(uint32_t* slot, uint32_t score, uint32_t exact) { *slot = anyof_combine(*slot, anyof_pack(score, exact)); }

// the group's key joined into a candidate (score, exact): score.saturating_add, exact |= (multi.rs:45, 70; k_join_add)
FZB_ANYOF_FN void anyof_join(uint32_t cand_score, uint32_t cand_exact, uint32_t key, uint32_t* score, uint32_t* exact) {
    const uint32_t s = (cand_score & 0xFFFFu) + anyof_score(key);
    *score = s > 0xFFFFu ? 0xFFFFu : s;
    *exact = (cand_exact ? 1u : 0u) | anyof_exact(key);
}

// position of `value` in the ascending list, or n if absent (the slot of a hit over a candidate set: its place in the set's item list)
FZB_ANYOF_FN uint32_t anyof_find(const uint32_t* list, uint32_t n, uint32_t value) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (list[mid] < value) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && list[lo] == value) ? lo : n;
}
