// Tag facets - the per-tag match counts of a query: the per-record rule and the accumulation, as plain functions for the device AND the
// host (kernels_facets.hip and k_scope_flag_facets call them; tests/kernel_host/facets_host.cpp compiles them for the CPU and
// tests/test_facets_host.py holds them against numpy).
//
// The reference has no such notion: a picker that shows filter chips ("tests 1 204 - docs 87 - ignored 312") counts on the host, over a
// list it copied back.  Here the counts are taken where the records and the tag column already are.  For a query, A = the haystacks of the
// input the matcher accepts - before scope, bias, selection, limit and ordering - and the block of FZB_FACET_WORDS words holds
//   [0]       matched          |A|
//   [1]       visible          the members of A that are visible under the corpus' scope (the call's `found`)
//   [2 + b]   all_by_bit[b]    the members of A whose tag has bit b, b = 0 .. 15 - hidden ones included: a chip for an excluded bit
//                              shows what it hides
//   [18 + b]  visible_by_bit   the same over the visible members
// The tag comes through scope_tag_of, visibility through scope_visible (scope.h); neither is restated.
//   * facet_all_bits / facet_visible_bits   the rule per record: the bits it is counted under in either row;
//   * facets_wave_step   the device's step: 34 ballots (a record, a visible record, 16 tag bits, 16 tag bits of visible records), their
//                        popcounts into 34 wave-uniform accumulators that live across the trips of a grid-stride loop;
//   * facets_lane_step   the host's form of the same step: a loop over the lanes;
//   * facets_publish     wave totals -> one total per workgroup through LDS -> at most FZB_FACET_WORDS vector atomicAdd per workgroup.
#pragma once
#include <stdint.h>

#include "scope.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FZB_FACET_FN __host__ __device__ __forceinline__
#else
#define FZB_FACET_FN inline
#endif

#define FZB_FACET_BITS 16
#define FZB_FACET_MATCHED 0
#define FZB_FACET_VISIBLE 1
#define FZB_FACET_ALL_BY_BIT 2
#define FZB_FACET_VISIBLE_BY_BIT (FZB_FACET_ALL_BY_BIT + FZB_FACET_BITS)
#ifndef FZB_FACET_WORDS
#define FZB_FACET_WORDS (FZB_FACET_VISIBLE_BY_BIT + FZB_FACET_BITS)
#endif
static_assert(FZB_FACET_WORDS == 34, "the block's layout is part of the boundary (include/frizbee_hip.h)");

// the accumulators of one wave (device: wave-uniform values) or of one walk (host)
struct facet_acc {
    uint32_t w[FZB_FACET_WORDS];
};
FZB_FACET_FN void facets_clear(facet_acc& a) {
    for (int k = 0; k < FZB_FACET_WORDS; k++) a.w[k] = 0;
}

// ---- the rule per record: `valid` = the slot holds a record of A, `tag` = its haystack's tag ----
FZB_FACET_FN bool facet_visible(bool valid, uint32_t tag, uint32_t require, uint32_t exclude) { return valid && scope_visible(tag, require, exclude); }
// the bits the record is counted under: over all of A, and over its visible members
FZB_FACET_FN uint32_t facet_all_bits(bool valid, uint32_t tag) { return valid ? (tag & 0xFFFFu) : 0u; }
FZB_FACET_FN uint32_t facet_visible_bits(bool visible, uint32_t tag) { return visible ? (tag & 0xFFFFu) : 0u; }

// the tag of item k of a list of haystacks - the range (items == nullptr: haystack first + k) or a candidate set (first + items[k]);
// tags == nullptr: a corpus without tags, every tag 0
FZB_FACET_FN uint32_t facet_item_tag(const uint32_t* items, uint64_t k, const uint16_t* tags, uint64_t n_tags, uint64_t first) {
    return scope_tag_of(tags, tags ? n_tags : 0, first, 0u, items ? items[k] : (uint32_t)k);
}

// ---- the host's step: one lane at a time ----
FZB_FACET_FN void facets_lane_step(facet_acc& a, bool valid, uint32_t tag, uint32_t require, uint32_t exclude) {
    const bool vis = facet_visible(valid, tag, require, exclude);
    const uint32_t all = facet_all_bits(valid, tag), seen = facet_visible_bits(vis, tag);
    a.w[FZB_FACET_MATCHED] += valid ? 1u : 0u;
    a.w[FZB_FACET_VISIBLE] += vis ? 1u : 0u;
    for (int b = 0; b < FZB_FACET_BITS; b++) {
        a.w[FZB_FACET_ALL_BY_BIT + b] += (all >> b) & 1u;
        a.w[FZB_FACET_VISIBLE_BY_BIT + b] += (seen >> b) & 1u;
    }
}

#if defined(__HIPCC__)
// ---- the wave's step: called by every lane of the wave (uniform trip counts), 34 ballots, nothing leaves the wave ----
__device__ __forceinline__ void facets_wave_step(facet_acc& a, bool valid, uint32_t tag, uint32_t require, uint32_t exclude) {
    const bool vis = facet_visible(valid, tag, require, exclude);
    const uint32_t all = facet_all_bits(valid, tag), seen = facet_visible_bits(vis, tag);
    a.w[FZB_FACET_MATCHED] += (uint32_t)__popcll(__ballot(valid));
    a.w[FZB_FACET_VISIBLE] += (uint32_t)__popcll(__ballot(vis));
#pragma unroll
    for (int b = 0; b < FZB_FACET_BITS; b++) {
        a.w[FZB_FACET_ALL_BY_BIT + b] += (uint32_t)__popcll(__ballot((all >> b) & 1u));
        a.w[FZB_FACET_VISIBLE_BY_BIT + b] += (uint32_t)__popcll(__ballot((seen >> b) & 1u));
    }
}

// ---- across waves and workgroups: called ONCE per launch by all 256 threads.  Lane 0 of every wave adds its non-zero totals into LDS,
// thread k < FZB_FACET_WORDS adds the workgroup's word k into the block (cleared in stream order ahead of the launch).  Integer sums: the
// result does not depend on the order the workgroups run in, and nothing waits for another workgroup.
__device__ __forceinline__ void facets_publish(const facet_acc& a, uint32_t* __restrict__ block) {
    __shared__ uint32_t s_facets[FZB_FACET_WORDS];
    const uint32_t tid = threadIdx.x;
    if (tid < FZB_FACET_WORDS) s_facets[tid] = 0;
    __syncthreads();
    if ((tid & 63u) == 0) {
#pragma unroll
        for (int k = 0; k < FZB_FACET_WORDS; k++)
            if (a.w[k]) atomicAdd(&s_facets[k], a.w[k]);
    }
    __syncthreads();
    if (tid < FZB_FACET_WORDS && s_facets[tid]) atomicAdd(&block[tid], s_facets[tid]);
}
#endif  // __HIPCC__
