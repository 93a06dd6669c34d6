// Every environment switch of the library, in ONE place, parsed once on first use (fzb_knobs(); no launch path calls getenv).  What is left
// after round 6's prune are debugging aids and switches that force a SHIPPING alternative - the older form of a stage that still serves the
// scorings, needles or corpora outside the fast form's preconditions - so that tests can run it against the oracle on ordinary inputs
// (tests/test_gpu_knobs.py, through fzb_debug_reload_knobs()).  Measured-and-rejected variants are not kept behind switches: profiles/HISTORY.md.
#pragma once
#include <stdint.h>

struct FzbKnobs {
    // --- debugging aids ---
    bool debug_sync = false;         // FZB_DEBUG_SYNC=1        synchronise and report after every stage of the pipeline
    bool typo_exact_window = false;  // FZB_TYPO_EXACT_WINDOW=1 no typo fast path: every survivor of a typo query re-decided at the exact lane width (nothing rests on DESIGN.md "Typo configurations")
    bool no_filter_view = false;     // FZB_FILTER_VIEW=0       no interleaved filter view (not built at upload - saves a second copy of the bytes in HBM -, not used by the filter)
    bool no_signature = false;       // FZB_NO_SIGNATURE=1      no letter signatures (not built with the corpus - saves 4 bytes per haystack in HBM -, not used by the filter: k1_dfa reads every row instead of k1_dfa_sig)
    int debug_cus = 0;               // FZB_DEBUG_CUS=n         behave as on a device of n compute units (0: the device's own): every grid, the scratch sized by a grid and the thresholds written in CUs follow fzb_effective_cus(); while set, each launch's grid is recorded (fzb_debug_launch_grids)
    bool verify_promises = true;     // FZB_VERIFY_PROMISES=0   fzb_corpus_set_uniform_len / _set_max_len on BORROWED memory accepted without the device pass over the end offsets
    // --- force the form that serves inputs outside the fast form's preconditions ---
    bool no_lcs_dfa = false;         // FZB_NO_LCS_DFA=1        typo filter: the bit-vector kernel k1_filter (needles whose LCS automaton has more than 226 states) instead of the automaton in k1_dfa
    bool no_cdfa = false;            // FZB_NO_CDFA=1           ragged filter: the byte automaton (automata whose class-composite table exceeds 16 KB) instead of the composite one
    bool no_dp_classes = false;      // FZB_NO_DP_CLASSES=1     ASCII scorer: per-wave choice of computed lanes (k2b_dp: scorings outside dp_cf.h) instead of classified scoring
    bool no_fused_classify = false;  // FZB_NO_FUSED_CLASSIFY=1 ragged ASCII lists: k_compact1 + k2w_classify as two launches (the form typo queries and item lists take) instead of k_compact1_classify
    bool no_seg_list = false;        // FZB_NO_SEG_LIST=1       short lists with signatures: filter -> k_compact1 -> scorer as three launches (the form sub-32-lane scorings, typo / unicode queries and item lists take) instead of the filter listing its survivors
    bool no_sig_planes = false;      // FZB_NO_SIG_PLANES=1     the signature filter that lists its survivors reads the u32 signatures tile by tile (the form unaligned sub-ranges and corpora without room for the planes take) instead of the bit-planes in batches; the planes are still built
    bool no_items_dfa = false;      // FZB_NO_ITEMS_DFA=1      item lists of a candidate set (fzb_subset): the bit-vector thread-per-item filter k1_items (what the multi-pattern narrowing and every other filter mode take) instead of k1_items_dfa
    bool no_dp_cfm = false;          // FZB_NO_DP_CFM=1         multi-chunk scorer in its first form (dp_body.h: scorings outside dp_cfm.h)
    bool no_dp_cfu = false;          // FZB_NO_DP_CFU=1         unicode scorer in its first form (scorings outside dp_unicode.h's biased form)
    int unicode_multi = -1;          // FZB_UNICODE_MULTI=0|1   unicode windows of 65..1024 bytes: never / always thread per haystack (k2u_dp_unicode_multi); default: by the queue's length, on the device
    int coop_below = -1;             // FZB_COOP_BELOW=n        multi-chunk ASCII windows of a ragged list: four lanes per window (dp_quad.h) when fewer than n are queued (0: never; default: 48 per workgroup of the slice = 49 152 on 256 CUs; below 32 768 windows of any kind the single-chunk ones too)
    int park_lds_kb = 37;            // FZB_PARK_LDS_KB         multi-chunk scorer: parked rows in LDS when they fit this many KB per workgroup (0: always the global slab, as for needles of many rows)
    int spin_wait_us = 1000;         // FZB_SPIN_WAIT_US=n      synchronous entry points poll the stream for up to n us before they block (0: block at once, as hipStreamSynchronize does)
    int edit_chunk_items = 1 << 20;  // FZB_EDIT_CHUNK_ITEMS=n  fzb_corpus_remove / _replace: source haystacks per chunk of the edit pass (a multiple of 1024, at least 1024): bounds its scratch
    // --- multi-device form ---
    bool shard_gather_copy = false;  // FZB_SHARD_GATHER=copy   counts to the host + hipMemcpyPeerAsync even when every shard shares the root device (the form shards on other devices take)
    int shard_inline = -1;           // FZB_SHARD_INLINE=0|1    shards on the root device: 0 = through the worker threads, 1 = enqueued by the caller
};

const FzbKnobs& fzb_knobs();

// The ONE place the library learns how many compute units it runs on: the current device's own count unless FZB_DEBUG_CUS overrides it.
// Every grid (and what is sized by one) derives from this number; nothing else reads the device's count.
int fzb_effective_cus(int* out);  // 0, or the hipError_t of the device query
// min(want, effective CUs * per_cu), at least 1: the grid of a grid-stride pass over `want` units of work
unsigned fzb_grid_cap(uint64_t want, unsigned per_cu);

// Every kernel launch of the library goes through FZB_LAUNCH: hipLaunchKernelGGL, and - only while FZB_DEBUG_CUS is set - a record of the
// kernel's name and grid, so that tests can prove how many trips a grid-stride loop took (fzb_debug_launch_grids).
// (a plain bool: written by fzb_debug_reload_knobs() alone, which the tests call between queries, never while a launch is in flight)
extern bool g_fzb_record_grids;
void fzb_record_grid(const char* kernel, unsigned grid);
#define FZB_LAUNCH(kernel, grid, ...)                                  \
    do {                                                               \
        const dim3 fzb_grid_ = (grid);                                 \
        if (g_fzb_record_grids) fzb_record_grid(#kernel, fzb_grid_.x); \
        hipLaunchKernelGGL(kernel, fzb_grid_, __VA_ARGS__);            \
    } while (0)
