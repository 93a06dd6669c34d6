// gfx950 kernels, stage 1: the streaming filter over the whole haystack list (HBM-bound) and the small
// order-preserving compaction kernels (scan / map) that turn its bitmap into a dense survivor list.
//
// Reference semantics being implemented:
//   * `match_list_into_impl` outer loop: length check + prefilter accept (src/matcher/algo.rs:78-103)
//   * 0-typo ASCII accept  == needle is a case-folded ordered subsequence (src/prefilter/algo/ascii.rs:6-54)
//   * k-typo accept        is implied by LCS(needle, haystack) + k >= rows (src/prefilter/mod.rs:1013-1084);
//     the converse does not hold at every lane width (oracle/selfcheck.cpp), so with typos - and on the unicode
//     path, where this stage only looks at each scalar's LAST byte - this stage is a conservative superset
//     and the lane-exact prefilter (kernels_window.hip) re-decides every survivor.
#include "kernels_common.h"
#include "compact1.h"
#include "dfa_lds.h"
#include "sig_filter.h"
#include "items_filter.h"
#include "seg_list.h"
#include <algorithm>
#include <cstdlib>

// ---------------------------------------------------------------------------------------------------
// K1: one thread per haystack.  Bytes are streamed from HBM as aligned 16-byte vectors (padded-16 layout),
// each byte indexes a 256-entry table in LDS whose entry is the bitmask of needle rows that byte can
// match (either case); the per-thread state is one machine word:
//   MODE 1 (ordered subsequence): st is one-hot at the next row to match; `st += st & T[b]` advances it.
//   MODE 2 (bit-vector LCS, Allison-Dix/Hyyro): V' = (V + (V & M)) | (V & ~M); LCS = #zero bits.
// Output: 1 bit per haystack (wave ballot -> one u64 store per wave) + a count per 1024-haystack tile.
// ---------------------------------------------------------------------------------------------------
template <typename TW, int MODE>
__device__ __forceinline__ void filter_step(TW& st, u32 b, const TW* T) {
    TW t = T[b];
    if (MODE == 1) {
        st += st & t;
    } else {
        TW u = st & t;
        st = (st + u) | (st & ~t);
    }
}

template <typename TW, int MODE>
__device__ __forceinline__ void filter_word(TW& st, u32 w, u32 nbytes, const TW* T) {
    if (nbytes >= 4) {
        filter_step<TW, MODE>(st, w & 0xFF, T);
        filter_step<TW, MODE>(st, (w >> 8) & 0xFF, T);
        filter_step<TW, MODE>(st, (w >> 16) & 0xFF, T);
        filter_step<TW, MODE>(st, w >> 24, T);
    } else {
        for (u32 k = 0; k < nbytes; k++) filter_step<TW, MODE>(st, (w >> (8 * k)) & 0xFF, T);
    }
}

// MARG (MODE 2 only): a second bit per haystack, "accepted with nothing to spare" (LCS == need exactly), with its own per-tile
// counts - the only inputs on which the reference's chunked typo prefilter can differ from the LCS criterion
// (tests/test_oracle_reference_properties.py), so only those are re-decided at the exact lane width (k2a_window, decide form).
// The kernel also clears the per-haystack reject bits / per-tile reject counts that the decide pass sets.
struct MargOut {
    u64* bitmap_m;
    u32* tile_counts_m;
    u64* reject_bits;
    u32* tile_rejects;
};
template <typename TW, int MODE, typename ET, bool MARG = false>
__global__ __launch_bounds__(256) void k1_filter(const u8* __restrict__ bytes, const ET* __restrict__ ends, u64 first, u32 count,
                                                 const u64* __restrict__ Tg, int rows, int need, u32 min_len,
                                                 u64* __restrict__ bitmap, u32* __restrict__ tile_counts, u32* __restrict__ reset_counters, MargOut mo = MargOut{}, u32 ulen = 0) {
    // the per-call counter block is cleared here (first workgroup) instead of by a separate memset launch: nothing before the
    // compaction kernel reads it
    if (blockIdx.x == 0 && threadIdx.x < 16) reset_counters[threadIdx.x] = 0;
    __shared__ TW T[256];
    __shared__ u32 s_cnt, s_cnt_m;
    const int tid = threadIdx.x;
    T[tid] = (TW)Tg[tid];
    const u32 ntiles = (count + FZB_TILE - 1) / FZB_TILE;
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tid == 0) s_cnt = 0, s_cnt_m = 0;
        __syncthreads();
        u32 cnt = 0, cnt_m = 0;
#pragma unroll 1
        for (int p = 0; p < FZB_TILE / 256; p++) {
            const u32 li = tile * FZB_TILE + p * 256 + tid;
            bool matched = false, marginal = false;
            if (li < count) {
                u64 s;
                u32 L;
                haystack_span_u(ends, ulen, first + li, s, L);
                if (L >= min_len) {
                    const uint4* vp = (const uint4*)(bytes + s);
                    TW st = (MODE == 1) ? (TW)1 : (TW)~(TW)0;
                    const u32 nvec = (L + 15) >> 4;
                    for (u32 v = 0; v < nvec; v++) {
                        const uint4 q = vp[v];
                        const u32 rem = L - 16 * v;
                        filter_word<TW, MODE>(st, q.x, rem, T);
                        if (rem > 4) filter_word<TW, MODE>(st, q.y, rem - 4, T);
                        if (rem > 8) filter_word<TW, MODE>(st, q.z, rem - 8, T);
                        if (rem > 12) filter_word<TW, MODE>(st, q.w, rem - 12, T);
                    }
                    if (MODE == 1) {
                        matched = (st >> rows) & 1;
                    } else {
                        const TW low = rows >= (int)(8 * sizeof(TW)) ? (TW)~(TW)0 : (((TW)1 << rows) - 1);
                        const TW z = ~st & low;
                        const int lcs = sizeof(TW) == 8 ? __popcll((u64)z) : __popc((u32)z);
                        matched = lcs >= need;
                        marginal = lcs == need;
                    }
                }
            }
            const u64 b = __ballot(matched);
            if (lane_id() == 0) {
                bitmap[(tile * FZB_TILE + p * 256) / 64 + (tid >> 6)] = b;
                cnt += __popcll(b);
            }
            if (MARG) {
                const u64 bm = __ballot(marginal);
                if (lane_id() == 0) {
                    mo.bitmap_m[(tile * FZB_TILE + p * 256) / 64 + (tid >> 6)] = bm;
                    mo.reject_bits[(tile * FZB_TILE + p * 256) / 64 + (tid >> 6)] = 0;
                    cnt_m += __popcll(bm);
                }
            }
        }
        if (lane_id() == 0 && cnt) atomicAdd(&s_cnt, cnt);
        if (MARG && lane_id() == 0 && cnt_m) atomicAdd(&s_cnt_m, cnt_m);
        __syncthreads();
        if (tid == 0) {
            tile_counts[tile] = s_cnt;
            if (MARG) mo.tile_counts_m[tile] = s_cnt_m, mo.tile_rejects[tile] = 0;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// K1-DFA: the ordered-subsequence test (MODE 1) as a table-driven DFA.  State s = number of needle rows
// already matched; dfa[s * 256 + b] = s + 1 if byte b matches row s (either case), else s; state `rows`
// is absorbing.  One step is ONE v_perm_b32 (builds the LDS address (s << 8) | byte) + ONE ds_read_u8,
// instead of extract / lookup / and / add.  The lookup chain is serial per haystack, so every thread runs
// the 4 haystacks it owns in a tile as 4 interleaved chains, with all their 16-byte vectors requested
// from HBM up front.  The table has (rows + 1) * 256 bytes; 4 byte values share a dword, so the
// alphanumerics of one state row spread over distinct LDS banks.
// ---------------------------------------------------------------------------------------------------
// (Round 5 measured an instantiation without per-lane lengths for uniform 32-byte lists and the table at a 256-byte row pitch - 7.5 M instead of
// 10.7 M VALU instructions per launch, the same 57 us, more LDS bank conflicts; round 6 closed the topic: profiles/r06_corun.txt, profiles/HISTORY.md.)
// One tile of k1_dfa: the four haystacks thread `tid` owns (positions p * 256 + tid), decided and written to the bitmap; returns the
// lane's share of the tile's count (non-zero in lane 0 of every wave only).  Shared by k1_dfa and by k1_dfa_sig's dense tiles.
// lds_bits (k1_dfa_sig listing its survivors): the tile's 32 decision words in LDS get the ballots too.
template <typename ET, bool LDS_BITS = false>
__device__ __forceinline__ u32 dfa_stream_tile(const u8* __restrict__ bytes, const ET* __restrict__ ends, u64 first, u32 count, u32 tile, int tid, u32 ulen, u32 min_len,
                                               u32 acc_lo, const u8* dfa, u64* __restrict__ bitmap, u32* lds_bits = nullptr) {
    u64 hs[4];
    u32 hl[4];
    uint4 v0[4], v1[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const u32 li = tile * FZB_TILE + p * 256 + tid;
        hs[p] = 0;
        hl[p] = 0;
        if (li < count) haystack_span_u(ends, ulen, first + li, hs[p], hl[p]);
    }
#pragma unroll
    for (int p = 0; p < 4; p++) {
        v0[p] = make_uint4(0, 0, 0, 0);
        v1[p] = make_uint4(0, 0, 0, 0);
        const uint4* vp = (const uint4*)(bytes + hs[p]);
        // (plain loads: with the non-temporal hint the second vector's request finds the line gone from the vector cache - a wave's two
        // load instructions share every line of a 32-byte-record list - and the kernel takes 62 us instead of 57)
        if (hl[p] > 0) v0[p] = vp[0];
        if (hl[p] > 16) v1[p] = vp[1];
    }
    u32 st[4] = {0, 0, 0, 0};
    // short haystacks (<= 32 bytes): both vectors are already in flight
    if (hl[0] >= 16 && hl[1] >= 16 && hl[2] >= 16 && hl[3] >= 16) {
        { const u32 w[4] = {v0[0].x, v0[1].x, v0[2].x, v0[3].x}; dfa_word4<true>(st, w, dfa); }
        { const u32 w[4] = {v0[0].y, v0[1].y, v0[2].y, v0[3].y}; dfa_word4<true>(st, w, dfa); }
        { const u32 w[4] = {v0[0].z, v0[1].z, v0[2].z, v0[3].z}; dfa_word4<true>(st, w, dfa); }
        { const u32 w[4] = {v0[0].w, v0[1].w, v0[2].w, v0[3].w}; dfa_word4<true>(st, w, dfa); }
    } else {
#pragma unroll
        for (int p = 0; p < 4; p++) st[p] = dfa_partial<true>(st[p], v0[p], hl[p] >= 16 ? 16u : hl[p], dfa);
    }
    if (hl[0] >= 32 && hl[1] >= 32 && hl[2] >= 32 && hl[3] >= 32) {
        { const u32 w[4] = {v1[0].x, v1[1].x, v1[2].x, v1[3].x}; dfa_word4<true>(st, w, dfa); }
        { const u32 w[4] = {v1[0].y, v1[1].y, v1[2].y, v1[3].y}; dfa_word4<true>(st, w, dfa); }
        { const u32 w[4] = {v1[0].z, v1[1].z, v1[2].z, v1[3].z}; dfa_word4<true>(st, w, dfa); }
        { const u32 w[4] = {v1[0].w, v1[1].w, v1[2].w, v1[3].w}; dfa_word4<true>(st, w, dfa); }
    } else {
#pragma unroll
        for (int p = 0; p < 4; p++)
            if (hl[p] > 16) st[p] = dfa_partial<true>(st[p], v1[p], hl[p] >= 32 ? 16u : hl[p] - 16, dfa);
    }
    u32 cnt = 0;
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const u32 L = hl[p];
        const u32 li = tile * FZB_TILE + p * 256 + tid;
        const bool matched = li < count && L >= min_len && st[p] >= acc_lo;
        const u64 b = __ballot(matched);
        if (lane_id() == 0) {
            bitmap[(tile * FZB_TILE + p * 256) / 64 + (tid >> 6)] = b;
            cnt += __popcll(b);
            if constexpr (LDS_BITS) {
                lds_bits[p * 8 + 2 * (tid >> 6)] = (u32)b;
                lds_bits[p * 8 + 2 * (tid >> 6) + 1] = (u32)(b >> 32);
            }
        }
    }
    return cnt;
}

template <typename ET>
__global__ __launch_bounds__(256) void k1_dfa(const u8* __restrict__ bytes, const ET* __restrict__ ends, u64 first, u32 count,
                                              const u8* __restrict__ dfa_g, int rows, u32 min_len, u32 dead, u32 acc_lo, u64* __restrict__ bitmap,
                                              u32* __restrict__ tile_counts, u32* __restrict__ reset_counters, u32 ulen) {
    // the per-call counter block is cleared here (first workgroup) instead of by a separate memset launch: nothing before the
    // compaction kernel reads it
    if (blockIdx.x == 0 && threadIdx.x < 16) reset_counters[threadIdx.x] = 0;
    // the table is the ONLY LDS object of the kernel and therefore sits at LDS address 0: a lookup's address is the v_perm result itself
    // (behind a static __shared__ variable every lookup paid a v_add of the table's offset); the tile counter lives behind the table
    extern __shared__ __attribute__((aligned(16))) u8 dfa[];
    u32& s_cnt = *(u32*)(dfa + FZB_DFA_LDS_BYTES(rows));
    const int tid = threadIdx.x;
    dfa_require_lds_base0(dfa);
    dfa_load_lds(dfa, dfa_g, rows);
    const u32 ntiles = (count + FZB_TILE - 1) / FZB_TILE;
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        const u32 cnt = dfa_stream_tile<ET>(bytes, ends, first, count, tile, tid, ulen, min_len, acc_lo, dfa, bitmap);
        if (lane_id() == 0 && cnt) atomicAdd(&s_cnt, cnt);
        __syncthreads();
        if (tid == 0) tile_counts[tile] = s_cnt;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// K1-DFA behind the corpus' letter signatures (sig_filter.h): the same automaton, the same table at LDS address 0, the same persistent
// grid and the same outputs (bitmap word per 64 haystacks, count per tile, counter reset) - but a tile first reads its 1024 signatures
// (4 KB instead of 32 KB) and only the rows whose signature holds every needle letter are looked at.  Their positions go into an LDS
// queue (one LDS atomic per wave); a tile with few of them (<= gather_max) GATHERS them - thread t runs queued row t, t + 256, .. as one
// chain and sets its bit in an LDS bitmap - and a tile with many runs k1_dfa's streaming body, so the worst case is the 4 extra bytes per
// haystack.  (Requesting the next tile's signatures before the gather - four registers, one of the two load latencies hidden - measured
// slower: 70.8 against 67.8 us per step, profiles/sig_filter.txt; not kept.)
// Only for needles sig_filter.h calls eligible: a zero byte then matches no row, and rows are masked to their length before the chain.
// No spin-waits, no ordering between workgroups.
// SEG (contiguous ranges in front of k2b_dp_short: host.hip, pipe_filter_stage): the kernel also LISTS its survivors, so that no compaction
// launch follows.  A workgroup then owns a contiguous run of tiles instead of a grid-strided set (seg_list.h: the partition k_compact1
// uses), every tile's decisions - a dense tile's ballots too - end in the LDS bitmap, and after each tile all four waves rank its set bits
// (32 word popcounts scanned in every wave, position p * 256 + tid per thread: a dense tile's stores are coalesced) and store the
// range-relative indices in ascending order behind the run's earlier ones at seg.list[b * seg.stride + k]; seg.counts[b] = the run's
// survivors.  Bitmap words and tile counts are written as before: every consumer outside that path still reads them.
// Tiles are still taken one at a time (the signatures of several tiles requested in one round trip and their queues gathered together is
// not built: profiles/sig_batched.txt).
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 sig_mask_vec(uint4 q, u32 nbytes) {  // bytes [nbytes, 16) -> 0
    u32 w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const u32 nvb = nbytes > 4u * j ? nbytes - 4u * j : 0u;
        w[j] = nvb >= 4 ? w[j] : (w[j] & ((1u << (8 * nvb)) - 1));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ u32 dfa_chain16(u32 st, const uint4& q, const u8* dfa) {
    const u32 w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        st = dfa_step<0>(st, w[j], dfa);
        st = dfa_step<1>(st, w[j], dfa);
        st = dfa_step<2>(st, w[j], dfa);
        st = dfa_step<3>(st, w[j], dfa);
    }
    return st;
}
// Listing one tile from its 32 decision words in LDS (SEG): tile count, the bitmap words (write_words: a gathered tile's - a dense tile's
// were written by dfa_stream_tile) and the survivors' range-relative indices, ascending, at seg_out[seg_n ..].  Returns the tile's count.
// Every wave scans the 32 word popcounts itself (lanes 32..63 mirror 0..31): no prefix array in LDS, no barrier for one.
__device__ __forceinline__ u32 seg_list_tile(const u32* s_bits, u32 t, u32 tile, bool write_words, u64* __restrict__ bitmap, u32* __restrict__ tile_counts, u32* __restrict__ seg_out, u32 seg_n) {
    const u32 l32 = t & 31u;
    const u32 wl = s_bits[l32];
    const u32 c = (u32)__popc(wl);
    // (inclusive scan of the 32 counts: inside each row of 16 lanes (tc_scan16), then row 0's sum into row 1: some ten VALU instructions
    // instead of five dependent cross-lane reads through LDS)
    u32 incl = tc_scan16(c);
    incl += (l32 & 16u) ? (u32)__builtin_amdgcn_readlane((int)incl, 15) : 0u;
    const u32 excl = incl - c, total = (u32)__builtin_amdgcn_readlane((int)incl, 31);
    if (t == 0) tile_counts[tile] = total;
    if (write_words && t < FZB_TILE / 64) bitmap[(size_t)tile * (FZB_TILE / 64) + t] = (u64)s_bits[2 * t] | ((u64)s_bits[2 * t + 1] << 32);
    if (total) {  // workgroup-uniform
#pragma unroll
        for (int p = 0; p < FZB_TILE / 256; p++) {
            const u32 pos = (u32)(p * 256) + t, w = pos >> 5;  // (one of two words per wave)
            const u32 word = (u32)__builtin_amdgcn_ds_bpermute((int)(w << 2), (int)wl), before = (u32)__builtin_amdgcn_ds_bpermute((int)(w << 2), (int)excl);
            if ((word >> (pos & 31)) & 1) seg_out[tc_rank32(seg_n + before, word, pos & 31)] = tile * FZB_TILE + pos;
        }
    }
    return total;
}

// The PLANE form of k1_dfa_sig<.., SEG> (sig_filter.h, "bit-planes"; `first` a multiple of the tile): the workgroup's run in batches of at
// most FZB_SIG_BATCH_TILES tiles, and per batch TWO dependent round trips instead of two per tile -
//   1. thread (tile, word) ANDs the plane words of the needle's letters (nsig's set bits: uniform) - the batch's candidates, 128 B per
//      tile, in LDS; nothing of a signature stays in registers;
//   2. one popcount scan (a tile = a row of 16 lanes) gives every tile its count and every candidate of a tile within gather_max its slot
//      in ONE queue of batch-relative positions; tiles beyond it stream as in the u32 form;
//   3. the queue is gathered two rows per thread and round of 512: all row loads first, then the two chains interleaved; decisions by LDS
//      atomic-or into the batch's decision words;
//   4. the tiles are listed one by one from LDS, exactly as in the u32 form (seg_list_tile).
// LDS behind the table: candidate words [B][16] u64, decision words [B][32], tile counts [B], queue [B * gather_max] u16 - 8 224 B for B = 8.
#ifndef FZB_SIG_CAND_INFLIGHT
#define FZB_SIG_CAND_INFLIGHT 8  // plane words of one thread requested before the first is used (sig_planes_run, step 1)
#endif
template <typename ET>
__device__ __forceinline__ void sig_planes_run(const u8* __restrict__ bytes, const ET* __restrict__ ends, const u64* __restrict__ planes, u32 nsig, const u64* __restrict__ planes2, u32 nsig2, u64 first, u32 count, u32 rows,
                                               u32 min_len, u32 acc_lo, u64* __restrict__ bitmap, u32* __restrict__ tile_counts, u32 ulen, u32 gather_max, const SegList& seg, u8* dfa, const u8* __restrict__ dfa_g) {
    constexpr u32 B = FZB_SIG_BATCH_TILES;
    static_assert(B * 16 <= 256 && B * 32 <= 256 && B * FZB_TILE <= 65536, "a batch's words are one per thread, its positions fit the queue's u16");
    u8* const behind = dfa + FZB_DFA_LDS_BYTES(rows);
    u64* const s_cand = (u64*)behind;                          // (the table's rows are multiples of 32 bytes)
    u32* const s_dec = (u32*)(behind + 128 * B);
    u32* const s_tq = (u32*)(behind + 256 * B);                // candidates per tile of the batch
    u16* const queue = (u16*)(behind + 256 * B + 4 * B);
    const u32 tid = threadIdx.x;
    const u32 ntiles = (count + FZB_TILE - 1) / FZB_TILE;
    const u64 tile0 = first / FZB_TILE;
    u32 t_begin, t_end, seg_n = 0;
    tc_run(ntiles, seg.stride / FZB_TILE, blockIdx.x, &t_begin, &t_end);
    u32* const seg_out = seg.list + (size_t)blockIdx.x * seg.stride;
    const u32 j = tid >> 4, w = tid & 15u;  // my (tile of the batch, word)
    // 1. a batch's candidate words.  The plane words are requested eight at a time and only then AND-ed (the masks are uniform: scalar
    // branches), so that a needle of up to eight plane words is ONE round trip - as a plain loop every load waited for the one before it.
    // The REPEAT planes (sig_filter.h) are the upper half of one 64-bit mask: bit 32 + b = word of planes2's bit b, at the same index -
    // a uniform distance from the thread's word of `planes`.  nsig2 == 0 (no repeat in the needle, or a corpus without repeat planes):
    // the loop is the one over nsig alone.
    const u64 need = (u64)nsig | ((u64)nsig2 << 32);
    const ptrdiff_t to2 = nsig2 ? (ptrdiff_t)((uintptr_t)planes2 - (uintptr_t)planes) : 0;
    auto load_cand = [&](u32 tb, u32 nb) -> u64 {
        if (tid >= nb * 16) return 0;
        u64 cand = sig_plane_valid(tb + j, w, count);
        const u8* pl = (const u8*)(planes + sig_plane_index(tile0 + tb + j, 0, w));
        u64 m = need;
        while (m) {
            u64 v[FZB_SIG_CAND_INFLIGHT];
#pragma unroll
            for (int q = 0; q < FZB_SIG_CAND_INFLIGHT; q++) {
                v[q] = ~0ull;
                if (m) {
                    const u32 k = (u32)__builtin_ctzll(m);
                    v[q] = *(const u64*)(pl + (k < 32u ? (ptrdiff_t)(k * FZB_SIG_PLANE_WORDS * 8u) : to2 + (ptrdiff_t)((k - 32u) * FZB_SIG_PLANE_WORDS * 8u)));
                    m &= m - 1u;
                }
            }
#pragma unroll
            for (int q = 0; q < FZB_SIG_CAND_INFLIGHT; q++) cand &= v[q];
        }
        return cand;
    };
    // (the first batch's words are requested BEFORE the table is copied into LDS: both arrive in one round trip)
    u64 cand = t_begin < t_end ? load_cand(t_begin, min(B, t_end - t_begin)) : 0;
    dfa_load_lds(dfa, dfa_g, (int)rows);
    for (u32 tb = t_begin; tb < t_end; tb += B) {
        const u32 nb = min(B, t_end - tb);
        if (tb != t_begin) cand = load_cand(tb, nb);
        if (tid < B * 32) s_dec[tid] = 0;
        // 2. counts and slots: inclusive scan inside each row of 16 lanes = one tile
        const u32 c = (u32)__popcll(cand);
        const u32 incl = tc_scan16(c);
        if (tid < B * 16) {
            s_cand[tid] = cand;
            if (w == 15) s_tq[j] = incl;
        }
        __syncthreads();
        u32 qbase = 0, QT = 0, dense = 0;  // my tile's first slot; the queue's length and the tiles that stream (workgroup-uniform)
#pragma unroll
        for (u32 k = 0; k < B; k++) {
            const u32 q = s_tq[k];
            if (q > gather_max) dense |= 1u << k;
            else {
                if (k < j) qbase += q;
                QT += q;
            }
        }
        if (tid < nb * 16 && !((dense >> j) & 1)) {
            u32 slot = qbase + incl - c;
            for (u64 m = cand; m; m &= m - 1) queue[slot++] = (u16)(j * FZB_TILE + w * 64 + (u32)__builtin_ctzll(m));
        }
        // 3a. dense tiles: k1_dfa's streaming body, ballots into the tile's decision words too
        for (u32 d = dense; d; d &= d - 1) {
            const u32 k = (u32)__builtin_ctz(d);
            (void)dfa_stream_tile<ET, true>(bytes, ends, first, count, tb + k, (int)tid, ulen, min_len, acc_lo, dfa, bitmap, s_dec + 32 * k);
        }
        __syncthreads();
        // 3b. the queue, two rows per thread and round
        for (u32 e0 = 0; e0 < QT; e0 += 512) {
            const bool two = e0 + 256 < QT;  // workgroup-uniform
            u32 pos[2] = {0, 0};
            bool has[2];
            uint4 a[2], b[2];
            u32 L[2];
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const u32 e = e0 + (u32)r * 256 + tid;
                has[r] = e < QT && (r == 0 || two);
                a[r] = make_uint4(0, 0, 0, 0);
                b[r] = make_uint4(0, 0, 0, 0);
                L[r] = 0;
                if (has[r]) {
                    pos[r] = queue[e];
                    u64 hs;
                    haystack_span_u(ends, ulen, first + (u64)tb * FZB_TILE + pos[r], hs, L[r]);
                    const uint4* vp = (const uint4*)(bytes + hs);
                    if (L[r] > 0) a[r] = vp[0];
                    if (L[r] > 16) b[r] = vp[1];
                }
            }
#pragma unroll
            for (int r = 0; r < 2; r++) {  // (a zero byte matches no row of an eligible needle: an absent row stays in state 0)
                if (L[r] < 16) a[r] = sig_mask_vec(a[r], L[r]);
                if (L[r] < 32) b[r] = sig_mask_vec(b[r], L[r] > 16 ? L[r] - 16 : 0u);
            }
            u32 st[2] = {0, 0};
            if (two) {
                const u32 w0[8] = {a[0].x, a[0].y, a[0].z, a[0].w, b[0].x, b[0].y, b[0].z, b[0].w}, w1[8] = {a[1].x, a[1].y, a[1].z, a[1].w, b[1].x, b[1].y, b[1].z, b[1].w};
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    st[0] = dfa_step<0>(st[0], w0[k], dfa); st[1] = dfa_step<0>(st[1], w1[k], dfa);
                    st[0] = dfa_step<1>(st[0], w0[k], dfa); st[1] = dfa_step<1>(st[1], w1[k], dfa);
                    st[0] = dfa_step<2>(st[0], w0[k], dfa); st[1] = dfa_step<2>(st[1], w1[k], dfa);
                    st[0] = dfa_step<3>(st[0], w0[k], dfa); st[1] = dfa_step<3>(st[1], w1[k], dfa);
                }
            } else {
                st[0] = dfa_chain16(0u, a[0], dfa);
                st[0] = dfa_chain16(st[0], b[0], dfa);
            }
#pragma unroll
            for (int r = 0; r < 2; r++)
                if (has[r] && L[r] >= min_len && st[r] >= acc_lo) atomicOr(&s_dec[pos[r] >> 5], 1u << (pos[r] & 31));
        }
        __syncthreads();
        // 4. the tiles leave one by one, from LDS
        for (u32 k = 0; k < nb; k++) {
            u32 t = tid;
            asm volatile("" : "+v"(t));  // (nothing of the listing is hoisted out of the loops: see the u32 form)
            seg_n += seg_list_tile(s_dec + 32 * k, t, tb + k, !((dense >> k) & 1), bitmap, tile_counts, seg_out, seg_n);
        }
        __syncthreads();  // the next batch clears the decision words
    }
    if (tid == 0) seg.counts[blockIdx.x] = seg_n;
}

// (8 waves per SIMD like k1_dfa, whose grid - 8 workgroups per CU - it shares: without the bound the kernel takes 68 VGPRs and a CU holds 7)
// PLANES (only with SEG): `sig` points at the corpus' bit-planes (u64 words) and sig_planes_run above is the kernel's body; planes2 / nsig2:
// the corpus' repeat planes and the needle's repeat signature (nsig2 == 0: not read).  The u32 form makes no use of either.
template <typename ET, bool SEG, bool PLANES = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void k1_dfa_sig(const u8* __restrict__ bytes, const ET* __restrict__ ends, const u32* __restrict__ sig, u32 nsig, u64 first, u32 count,
                                                  const u8* __restrict__ dfa_g, int rows, u32 min_len, u32 acc_lo, u64* __restrict__ bitmap, u32* __restrict__ tile_counts,
                                                  u32* __restrict__ reset_counters, u32 ulen, u32 gather_max, SegList seg, const u64* __restrict__ planes2, u32 nsig2) {
    if (blockIdx.x == 0 && threadIdx.x < 16) reset_counters[threadIdx.x] = 0;
    // LDS behind the table (which stays the first object, at address 0): tile count, queue length, the tile's 1024 decision bits, the queue
    extern __shared__ __attribute__((aligned(16))) u8 dfa[];
    if constexpr (PLANES) {
        static_assert(SEG, "the plane form lists its survivors");
        dfa_require_lds_base0(dfa);
        sig_planes_run<ET>(bytes, ends, (const u64*)sig, nsig, planes2, nsig2, first, count, (u32)rows, min_len, acc_lo, bitmap, tile_counts, ulen, gather_max, seg, dfa, dfa_g);
        return;
    }
    u32& s_cnt = *(u32*)(dfa + FZB_DFA_LDS_BYTES(rows));
    u32& s_q = *(u32*)(dfa + FZB_DFA_LDS_BYTES(rows) + 4);
    u32* const s_bits = (u32*)(dfa + FZB_DFA_LDS_BYTES(rows) + 16);
    u16* const queue = (u16*)(dfa + FZB_DFA_LDS_BYTES(rows) + 16 + 128);
    const int tid = threadIdx.x, lane = tid & 63;
    dfa_require_lds_base0(dfa);
    dfa_load_lds(dfa, dfa_g, rows);
    const u32 ntiles = (count + FZB_TILE - 1) / FZB_TILE;
    const bool vec = (first & 3) == 0;  // the thread's four signatures are one aligned 16-byte vector
    // signatures of the rows 4 tid .. 4 tid + 3 of a tile; 0 (fails every test: the needle is not empty) at or beyond `count`
    auto load_sigs = [&](u32 tile) -> uint4 {
        const u32 li = tile * FZB_TILE + 4u * (u32)tid;
        uint4 s = make_uint4(0, 0, 0, 0);
        if (vec && li + 4 <= count) {
            s = *(const uint4*)(sig + first + li);
        } else {
            if (li < count) s.x = sig[first + li];
            if (li + 1 < count) s.y = sig[first + li + 1];
            if (li + 2 < count) s.z = sig[first + li + 2];
            if (li + 3 < count) s.w = sig[first + li + 3];
        }
        return s;
    };
    // SEG: the workgroup's run of tiles and the survivors it has listed so far (workgroup-uniform)
    u32 t_begin = blockIdx.x, t_end = ntiles, seg_n = 0;
    if (SEG) tc_run(ntiles, seg.stride / FZB_TILE, blockIdx.x, &t_begin, &t_end);
    u32* const seg_out = SEG ? seg.list + (size_t)blockIdx.x * seg.stride : nullptr;
    for (u32 tile = t_begin; tile < t_end; tile += SEG ? 1u : gridDim.x) {
        if (tid == 0) s_cnt = 0, s_q = 0;
        if (tid < 32) s_bits[tid] = 0;
        const uint4 s = load_sigs(tile);
        __syncthreads();
        const u32 sv[4] = {s.x, s.y, s.z, s.w};
        u64 pb[4];
        u32 tot = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            pb[j] = __ballot(sig_passes(sv[j], nsig));
            tot += (u32)__popcll(pb[j]);
        }
        if (tot) {  // wave-uniform
            u32 base = 0;
            if (lane == 0) base = atomicAdd(&s_q, tot);
            base = __shfl(base, 0);
            const u64 below = ((u64)1 << lane) - 1;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if ((pb[j] >> lane) & 1) queue[base + (u32)__popcll(pb[j] & below)] = (u16)(4 * tid + j);
                base += (u32)__popcll(pb[j]);
            }
        }
        __syncthreads();
        const u32 Q = s_q;  // the same for the whole workgroup: so is the branch
        if (Q > gather_max) {
            const u32 cnt = dfa_stream_tile<ET, SEG>(bytes, ends, first, count, tile, tid, ulen, min_len, acc_lo, dfa, bitmap, s_bits);
            if (!SEG && lane == 0 && cnt) atomicAdd(&s_cnt, cnt);
        } else {
            for (u32 e = tid; e < Q; e += 256) {
                const u32 pos = queue[e];
                u64 hs;
                u32 L;
                haystack_span_u(ends, ulen, first + (u64)tile * FZB_TILE + pos, hs, L);
                const uint4* vp = (const uint4*)(bytes + hs);
                uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
                if (L > 0) a = vp[0];
                if (L > 16) b = vp[1];
                if (L < 16) a = sig_mask_vec(a, L);
                if (L < 32) b = sig_mask_vec(b, L > 16 ? L - 16 : 0u);
                u32 st = dfa_chain16(0u, a, dfa);
                st = dfa_chain16(st, b, dfa);
                if (L >= min_len && st >= acc_lo) atomicOr(&s_bits[pos >> 5], 1u << (pos & 31));
            }
            if (!SEG) {
                __syncthreads();
                if (tid < FZB_TILE / 64) {
                    const u64 word = (u64)s_bits[2 * tid] | ((u64)s_bits[2 * tid + 1] << 32);
                    bitmap[(size_t)tile * (FZB_TILE / 64) + tid] = word;
                    const u32 c = (u32)__popcll(word);
                    if (c) atomicAdd(&s_cnt, c);
                }
            }
        }
        __syncthreads();
        if (!SEG) {
            if (tid == 0) tile_counts[tile] = s_cnt;
        } else {
            // (The thread index goes through an empty asm and the cross-lane reads are ds_bpermute with addresses made from it: as loop
            // invariants the four word indices, the bit masks and the bitmap word's address are hoisted out of the tile loop - a dozen
            // registers live across the dense tile's body, which the kernel's 64-VGPR bound turns into scratch.)
            u32 t = (u32)tid;
            asm volatile("" : "+v"(t));
            seg_n += seg_list_tile(s_bits, t, tile, Q <= gather_max, bitmap, tile_counts, seg_out, seg_n);
            __syncthreads();  // the next tile clears the decision words
        }
    }
    if (SEG && tid == 0) seg.counts[blockIdx.x] = seg_n;
}

// ---------------------------------------------------------------------------------------------------
// K1-DFA for ragged lists, burst form: a thread requests ALL vectors of its haystack (up to 8 = 128 bytes per round) back to
// back and only then runs the DFA over them from registers.  (SAN = false, a needle without a NUL byte: the zero fill behind a haystack's end matches
// no needle row and the vectors go through the DFA unmasked.)  In the rolling form of rounds 1-2 (one vector ahead) a 128-byte line was touched by ~8 loads
// of a wave that are separated by the DFA work of every resident wave, and the CU's footprint (24 waves x 64 haystacks x up to
// 128 B) is far beyond the vector L1, so most of those touches re-fetch the line from L2; issued back to back they hit.
// C4 shard: 297 -> 242 us.  (Two or four haystacks per thread as interleaved DFA chains on top of it: 276 / 300 us, and again 281 / 405 us after
// the lookups were cut to v_perm + ds_read with one wait per round - with 8 waves per SIMD the lookup chain is already hidden; neither that
// nor removing a quarter of the loop's instructions moved the kernel, so it is bound by its cache transactions: every 16-byte piece of a
// lane is its own request, ~35 lines per wave instruction.)
// ---------------------------------------------------------------------------------------------------
template <typename ET, bool SAN>
__global__ __launch_bounds__(256) void k1_dfa_ragged_burst(const u8* __restrict__ bytes, const ET* __restrict__ ends, u64 first, u32 count,
                                                           const u8* __restrict__ dfa_g, int rows, u32 min_len, u32 dead, u32 acc_lo, u64* __restrict__ bitmap,
                                                           u32* __restrict__ tile_counts, u32* __restrict__ reset_counters) {
    if (blockIdx.x == 0 && threadIdx.x < 16) reset_counters[threadIdx.x] = 0;
    // the table is the ONLY LDS object of the kernel and therefore sits at LDS address 0: a lookup's address is the v_perm result itself
    // (behind a static __shared__ variable every lookup paid a v_add of the table's offset); the tile counter lives behind the table
    extern __shared__ __attribute__((aligned(16))) u8 dfa[];
    u32& s_cnt = *(u32*)(dfa + FZB_DFA_LDS_BYTES(rows));
    const int tid = threadIdx.x;
    dfa_require_lds_base0(dfa);
    dfa_load_lds(dfa, dfa_g, rows);
    const u32 ntiles = (count + FZB_TILE - 1) / FZB_TILE;
    const u32 deadv = dead * 0x01010101u;
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        u32 cnt = 0;
#pragma unroll 1
        for (int sub = 0; sub < 4; sub++) {
            const u32 li = tile * FZB_TILE + sub * 256 + tid;
            u64 hs = 0;
            u32 hl = 0;
            if (li < count) haystack_span(ends, first + li, hs, hl);
            const uint4* vp = (const uint4*)(bytes + hs);
            u32 st = 0;
            for (u32 v0 = 0; 16 * v0 < hl; v0 += 8) {  // rounds of 8 vectors (one round for haystacks up to 128 bytes)
                uint4 q[8];
#pragma unroll
                for (int k = 0; k < 8; k++) q[k] = hl > 16 * (v0 + k) ? vp[v0 + k] : make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    if (hl <= 16 * (v0 + k)) break;
                    u32 w[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
                    if (SAN) {
                        const u32 rem = hl - 16 * (v0 + k);
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const u32 nvb = rem > 4u * j ? rem - 4u * j : 0u;
                            const u32 mask = nvb >= 4 ? 0xFFFFFFFFu : ((1u << (8 * nvb)) - 1);
                            w[j] = (w[j] & mask) | (deadv & ~mask);
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        st = dfa_step<0>(st, w[j], dfa);
                        st = dfa_step<1>(st, w[j], dfa);
                        st = dfa_step<2>(st, w[j], dfa);
                        st = dfa_step<3>(st, w[j], dfa);
                    }
                }
            }
            const bool matched = li < count && hl >= min_len && st >= acc_lo;
            const u64 b = __ballot(matched);
            if (lane_id() == 0) {
                bitmap[(tile * FZB_TILE + sub * 256) / 64 + (tid >> 6)] = b;
                cnt += __popcll(b);
            }
        }
        if (lane_id() == 0 && cnt) atomicAdd(&s_cnt, cnt);
        __syncthreads();
        if (tid == 0) tile_counts[tile] = s_cnt;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// K1-DFA for ragged lists over the CLASS-COMPOSITE automaton (round 3).  Four structural variants (profiles/r03_ragged_filter_variants.txt) left the burst form's time
// where it was, which pointed at the one thing they share: every wave is a serial chain of one dependent LDS lookup PER BYTE (~100 cycles
// each under load), and with all eight wave slots of a SIMD taken the throughput is waves / chain latency.  Here the chain has one link
// per G bytes: the automaton only distinguishes K byte CLASSES (bytes with identical columns: the needle's letters in either case, and
// "anything else" - 6 for `deadbeef`), so the host composes G transitions into one table, next = comp[state][c0 + K c1 + K^2 c2 + K^3 c3]
// (states x K^G bytes; G = 4 when that fits 16 KB, else 2).  Per dword: four class lookups cls[byte] that do NOT depend on the state (issued
// back to back for the whole 16-byte vector, off the chain), three multiply-adds for the offset, and ONE dependent lookup.
// LDS: [0, 256) byte -> class, [256, 256 + states * K^G) the composite table; lookups address LDS directly (the object starts at 0).
// ---------------------------------------------------------------------------------------------------
template <typename ET, bool SAN, int G>
__global__ __launch_bounds__(256) void k1_cdfa_ragged(const u8* __restrict__ bytes, const ET* __restrict__ ends, u64 first, u32 count,
                                                      const u8* __restrict__ cdfa_g, u32 cdfa_bytes, u32 K, u32 KG, u32 min_len, u32 dead, u32 acc_lo,
                                                      u64* __restrict__ bitmap, u32* __restrict__ tile_counts, u32* __restrict__ reset_counters) {
    if (blockIdx.x == 0 && threadIdx.x < 16) reset_counters[threadIdx.x] = 0;
    extern __shared__ __attribute__((aligned(16))) u8 lds[];
    const u32 tab_bytes = (cdfa_bytes + 15u) & ~15u;
    u32& s_cnt = *(u32*)(lds + tab_bytes);
    const int tid = threadIdx.x;
    dfa_require_lds_base0(lds);
    for (u32 i = tid * 4; i < tab_bytes; i += 256 * 4) *(u32*)(lds + i) = i < cdfa_bytes ? *(const u32*)(cdfa_g + i) : 0u;  // (the blob is padded to 16 bytes)
    const u32 ntiles = (count + FZB_TILE - 1) / FZB_TILE;
    const u32 deadv = dead * 0x01010101u;
    auto cls_of = [](u32 b) -> u32 { return *(const __attribute__((address_space(3))) u8*)(uintptr_t)b; };
    auto comp_at = [](u32 a) -> u32 { return *(const __attribute__((address_space(3))) u8*)(uintptr_t)(256u + a); };
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        u32 cnt = 0;
#pragma unroll 1
        for (int sub = 0; sub < 4; sub++) {
            const u32 li = tile * FZB_TILE + sub * 256 + tid;
            u64 hs = 0;
            u32 hl = 0;
            if (li < count) haystack_span(ends, first + li, hs, hl);
            const uint4* vp = (const uint4*)(bytes + hs);
            u32 st = 0;
            for (u32 v0 = 0; 16 * v0 < hl; v0 += 8) {  // rounds of 8 vectors (one round for haystacks up to 128 bytes)
                uint4 q[8];
#pragma unroll
                for (int k = 0; k < 8; k++) q[k] = hl > 16 * (v0 + k) ? vp[v0 + k] : make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    if (hl <= 16 * (v0 + k)) break;
                    u32 w[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
                    if (SAN) {
                        const u32 rem = hl - 16 * (v0 + k);
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const u32 nvb = rem > 4u * j ? rem - 4u * j : 0u;
                            const u32 mask = nvb >= 4 ? 0xFFFFFFFFu : ((1u << (8 * nvb)) - 1);
                            w[j] = (w[j] & mask) | (deadv & ~mask);
                        }
                    }
                    // the vector's sixteen class lookups: independent of the state
                    u32 c[4][4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        c[j][0] = cls_of(w[j] & 0xFF);
                        c[j][1] = cls_of((w[j] >> 8) & 0xFF);
                        c[j][2] = cls_of((w[j] >> 16) & 0xFF);
                        c[j][3] = cls_of(w[j] >> 24);
                    }
                    if (G == 4) {
                        u32 off[4];
#pragma unroll
                        for (int j = 0; j < 4; j++) off[j] = c[j][0] + K * (c[j][1] + K * (c[j][2] + K * c[j][3]));
#pragma unroll
                        for (int j = 0; j < 4; j++) st = comp_at(st * KG + off[j]);  // the chain: one dependent lookup per dword
                    } else {
                        u32 off[8];
#pragma unroll
                        for (int j = 0; j < 4; j++) off[2 * j] = c[j][0] + K * c[j][1], off[2 * j + 1] = c[j][2] + K * c[j][3];
#pragma unroll
                        for (int j = 0; j < 8; j++) st = comp_at(st * KG + off[j]);  // one dependent lookup per byte pair
                    }
                }
            }
            const bool matched = li < count && hl >= min_len && st >= acc_lo;
            const u64 b = __ballot(matched);
            if (lane_id() == 0) {
                bitmap[(tile * FZB_TILE + sub * 256) / 64 + (tid >> 6)] = b;
                cnt += __popcll(b);
            }
        }
        if (lane_id() == 0 && cnt) atomicAdd(&s_cnt, cnt);
        __syncthreads();
        if (tid == 0) tile_counts[tile] = s_cnt;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// The class-composite automaton over the corpus' filter VIEW (CorpusDev::vbytes: tiles sorted by vector count, groups of 64 interleaved by
// vector).  One wave per group: "vector v of my haystack" is ONE coalesced 1 KiB load for the whole wave, every lane of the wave has the
// same number of vectors, and all of a group's loads are issued back to back.  The decision bit goes to the haystack's ORIGINAL position
// in its tile (vperm) through an LDS atomic-or, so the bitmap, the per-tile counts and every later stage see nothing of the view.
// NV = vectors held in registers per haystack (8: lists up to 128 bytes, 16: up to 256).
// ---------------------------------------------------------------------------------------------------
// LEN: the kernel reads the haystacks' lengths (vlen: 2 of the view's ~83 bytes per haystack on the C4 shard).  They are needed to sanitise a
// last vector (SAN), for the stage's header (STAGE), to skip an outlier's lane (0xFFFF) and for `length >= min_len` - but with the zero fill
// harmless (!SAN) an outlier's lane holds zero vectors and cannot leave state 0, and every automaton the view kernel runs accepts only
// haystacks of at least min_len bytes (subsequence / unicode: the needle's bytes all occurred; LCS >= rows - k bytes matched): without SAN
// the launcher passes LEN = false and the array is not touched.
// (Rounds 4-5 also had a STAGE form - the accepting lanes copied their vectors into a per-tile block for the classifier and the scorers; the
// 48 MB copy-out cost the streaming kernel more than the scorers' gathers returned: profiles/HISTORY.md.)
// TPB = 1024 (short lists: the launcher's choice): sixteen waves, ONE group each - a tile is then one load round trip and one walk instead of four
// in a row, which is what a list of fewer tiles than the chip holds workgroups pays (a fixed ~ 13 us of the 256-thread form).
template <bool SAN, int G, int NV, bool LEN = true, int TPB = 256>
__global__ __launch_bounds__(TPB) void k1_cdfa_view(const u8* __restrict__ vbytes, const u32* __restrict__ vgofs, const u8* __restrict__ vgnv, const u16* __restrict__ vlen,
                                                    const u16* __restrict__ vperm, u64 first, u32 count, const u8* __restrict__ cdfa_g, u32 cdfa_bytes, u32 K, u32 KG,
                                                    u32 min_len, u32 dead, u32 acc_lo, u64* __restrict__ bitmap, u32* __restrict__ tile_counts, u32* __restrict__ reset_counters) {
    if (blockIdx.x == 0 && threadIdx.x < 16) reset_counters[threadIdx.x] = 0;
    extern __shared__ __attribute__((aligned(16))) u8 lds[];
    const u32 tab_bytes = (cdfa_bytes + 15u) & ~15u;
    u32& s_cnt = *(u32*)(lds + tab_bytes);
    u32* const s_bits = (u32*)(lds + tab_bytes + 16);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    dfa_require_lds_base0(lds);
    for (u32 i = tid * 4; i < tab_bytes; i += TPB * 4) *(u32*)(lds + i) = i < cdfa_bytes ? *(const u32*)(cdfa_g + i) : 0u;
    const u32 ntiles = (count + FZB_TILE - 1) / FZB_TILE;
    const u32 deadv = dead * 0x01010101u;
    auto cls_of = [](u32 b) -> u32 { return *(const __attribute__((address_space(3))) u8*)(uintptr_t)b; };
    auto comp_at = [](u32 a) -> u32 { return *(const __attribute__((address_space(3))) u8*)(uintptr_t)(256u + a); };
    const u64 g_first = first / 64;  // `first` is a multiple of the tile size
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tid == 0) s_cnt = 0;
        if (tid < 32) s_bits[tid] = 0;
        __syncthreads();
#pragma unroll 1
        for (int gi = 0; gi < 16 / (TPB / 64); gi++) {
            const u32 p = tile * FZB_TILE + (u32)(gi * (TPB / 64) + wave) * 64 + lane;  // sorted position (relative to `first`)
            const u32 gl = tile * (FZB_TILE / 64) + (u32)(gi * (TPB / 64) + wave);       // its group
            if (gl * 64 >= count) continue;
            // vgnv: vectors per member | (bytes stored per member of the LAST row / 4 - 1) << 5 (round 5: the group's last row is as narrow as
            // its longest member's tail allows - 4, 8, 12 or 16 bytes per lane, a contiguous 256..1024 bytes for the wave)
            const u32 code = __builtin_amdgcn_readfirstlane((u32)vgnv[g_first + gl]);
            const u32 nv = code & 31u, tw = ((code >> 5) + 1u) * 4u;
            const u8* gblock = vbytes + (size_t)__builtin_amdgcn_readfirstlane(vgofs[g_first + gl]) * 16;
            const u8* base = gblock + (u32)lane * 16;
            u32 hl = 0, orig = 0;
            if (p < count) { hl = LEN ? (u32)vlen[first + p] : 0u; orig = vperm[first + p]; }
            uint4 q[NV];
            uint4 tail = make_uint4(0, 0, 0, 0);
            if (nv) {  // (wave-uniform width: one load instruction of the width the group was stored with)
                const u8* tp = gblock + (size_t)(nv - 1) * 1024 + (size_t)lane * tw;
                if (tw == 16) tail = load16_stream<true>((const uint4*)tp);
                else tail = load_narrow_stream(tp, tw, true);
            }
            // (non-temporal: a wave's load covers whole lines that nothing reads again - the stream no longer displaces what the later stages
            // re-read: C4 shard 190 -> 183 us).  The FULL rows land in q[0 .. nv-2]; the narrow last row stays in `tail` and is the automaton's
            // last step (selecting it into q[nv-1] cost a chain of scalar branches and a full wait per vector)
#pragma unroll
            for (int k = 0; k < NV; k++) q[k] = (u32)k + 1 < nv ? load16_stream<true>((const uint4*)(base + (size_t)k * 1024)) : make_uint4(0, 0, 0, 0);
            u32 st = 0;
            // one vector of the lane's haystack through the class-composite automaton (vector index kk: only the sanitising form needs it)
            auto step = [&](const uint4& v, u32 kk) {
                u32 w[4] = {v.x, v.y, v.z, v.w};
                if (SAN) {
                    const u32 rem = hl > 16u * kk ? hl - 16u * kk : 0u;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const u32 nvb = rem > 4u * j ? rem - 4u * j : 0u;
                        const u32 mask = nvb >= 4 ? 0xFFFFFFFFu : ((1u << (8 * nvb)) - 1);
                        w[j] = (w[j] & mask) | (deadv & ~mask);
                    }
                }
                u32 c[4][4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    c[j][0] = cls_of(w[j] & 0xFF);
                    c[j][1] = cls_of((w[j] >> 8) & 0xFF);
                    c[j][2] = cls_of((w[j] >> 16) & 0xFF);
                    c[j][3] = cls_of(w[j] >> 24);
                }
                if (G == 4) {
                    u32 off[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) off[j] = c[j][0] + K * (c[j][1] + K * (c[j][2] + K * c[j][3]));
#pragma unroll
                    for (int j = 0; j < 4; j++) st = comp_at(st * KG + off[j]);
                } else {
                    u32 off[8];
#pragma unroll
                    for (int j = 0; j < 4; j++) off[2 * j] = c[j][0] + K * c[j][1], off[2 * j + 1] = c[j][2] + K * c[j][3];
#pragma unroll
                    for (int j = 0; j < 8; j++) st = comp_at(st * KG + off[j]);
                }
            };
#pragma unroll
            for (int k = 0; k < NV; k++) {
                if ((u32)k + 1 >= nv) continue;  // wave-uniform
                step(q[k], (u32)k);
            }
            if (nv) step(tail, nv - 1);
            if (p < count && (!LEN || (hl != 0xFFFFu && hl >= min_len)) && st >= acc_lo) {  // (0xFFFF: an outlier beyond 256 bytes - k1_cdfa_outliers decides it)
                atomicOr(&s_bits[orig >> 5], 1u << (orig & 31));
            }
        }
        __syncthreads();
        if (tid < FZB_TILE / 64) {
            const u64 word = (u64)s_bits[2 * tid] | ((u64)s_bits[2 * tid + 1] << 32);
            bitmap[(size_t)tile * (FZB_TILE / 64) + tid] = word;
            const u32 cnt = (u32)__popcll(word);
            if (cnt) atomicAdd(&s_cnt, cnt);
        }
        __syncthreads();
        if (tid == 0) tile_counts[tile] = s_cnt;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// The view's OUTLIERS (CorpusDev::vlong: the few haystacks beyond 256 bytes, which have no vectors in the view): decided from the canonical
// layout with the same class-composite automaton, the decision OR-ed into the bitmap the view kernel wrote and added to the tile's count.
// Launched behind k1_cdfa_view on the same stream; a list without outliers does not launch it.
// One WAVE per outlier, because a thread walking 600 bytes alone is a chain of 38 loads and 150 dependent lookups (12 us for the 71
// outliers of the Arabic-shaped list, half of what the view kernel takes for the other 285 516 haystacks): lane k takes vector k and
// runs it from EVERY start state (ns x G/4.. independent lookups - the transition function of its 16 bytes, ns bytes in LDS), then the
// wave composes the 64 functions in order: one dependent LDS byte per vector instead of a load and four lookups.
// ---------------------------------------------------------------------------------------------------
template <typename ET, bool SAN, int G>
__global__ __launch_bounds__(256) void k1_cdfa_outliers(const u8* __restrict__ bytes, const ET* __restrict__ ends, u64 first, u32 count, const u32* __restrict__ vlong, u32 n_long,
                                                        const u8* __restrict__ cdfa_g, u32 cdfa_bytes, u32 K, u32 KG, u32 ns, u32 min_len, u32 dead, u32 acc_lo,
                                                        u64* __restrict__ bitmap, u32* __restrict__ tile_counts) {
    extern __shared__ __attribute__((aligned(16))) u8 lds[];
    const u32 tab_bytes = (cdfa_bytes + 15u) & ~15u;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    dfa_require_lds_base0(lds);
    for (u32 i = tid * 4; i < tab_bytes; i += blockDim.x * 4) *(u32*)(lds + i) = i < cdfa_bytes ? *(const u32*)(cdfa_g + i) : 0u;
    __syncthreads();
    u8* fn = lds + tab_bytes + (size_t)wave * ns * 64;  // fn[s * 64 + k]: where vector k of the current round takes state s
    const u32 deadv = dead * 0x01010101u;
    auto cls_of = [](u32 b) -> u32 { return *(const __attribute__((address_space(3))) u8*)(uintptr_t)b; };
    auto comp_at = [](u32 a) -> u32 { return *(const __attribute__((address_space(3))) u8*)(uintptr_t)(256u + a); };
    const u32 wpw = blockDim.x >> 6;  // waves per workgroup: 4, or 1 when four waves' function tables do not fit
    for (u32 j = blockIdx.x * wpw + wave; j < n_long; j += gridDim.x * wpw) {
        const u64 gi = vlong[j];
        if (gi < first || gi >= first + count) continue;  // wave-uniform
        const u32 li = (u32)(gi - first);
        u64 hs;
        u32 hl;
        haystack_span(ends, gi, hs, hl);
        const uint4* vp = (const uint4*)(bytes + hs);
        const u32 nvec = (hl + 15u) >> 4;
        u32 st = 0;
        for (u32 base = 0; base < nvec; base += 64) {
            const u32 v = base + lane;
            if (v < nvec) {
                const uint4 q = vp[v];
                u32 w[4] = {q.x, q.y, q.z, q.w};
                if (SAN) {
                    const u32 rem = hl - 16 * v;
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const u32 nvb = rem > 4u * t ? rem - 4u * t : 0u;
                        const u32 mask = nvb >= 4 ? 0xFFFFFFFFu : ((1u << (8 * nvb)) - 1);
                        w[t] = (w[t] & mask) | (deadv & ~mask);
                    }
                }
                u32 off[G == 4 ? 4 : 8];
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const u32 c0 = cls_of(w[t] & 0xFF), c1 = cls_of((w[t] >> 8) & 0xFF), c2 = cls_of((w[t] >> 16) & 0xFF), c3 = cls_of(w[t] >> 24);
                    if (G == 4) off[t] = c0 + K * (c1 + K * (c2 + K * c3));
                    else off[2 * t] = c0 + K * c1, off[2 * t + 1] = c2 + K * c3;
                }
                for (u32 s0 = 0; s0 < ns; s0++) {
                    u32 t = s0;
#pragma unroll
                    for (int q4 = 0; q4 < (G == 4 ? 4 : 8); q4++) t = comp_at(t * KG + off[q4]);
                    fn[s0 * 64 + lane] = (u8)t;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const u32 steps = min(64u, nvec - base);
            for (u32 k = 0; k < steps; k++) st = fn[st * 64 + k];  // (every lane walks the same chain: broadcast reads)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if (lane == 0 && hl >= min_len && st >= acc_lo) {
            atomicOr((unsigned long long*)&bitmap[li >> 6], 1ull << (li & 63));
            atomicAdd(&tile_counts[li / FZB_TILE], 1u);
        }
    }
}

// (Round 3 measured three more forms of the ragged filter on the canonical layout - software-pipelined burst, cooperative coalesced loads through
// a per-wave LDS window, LDS-staged + length-sorted - at 244-253 / 234-292 / 530-990 us against the burst form's 234; none is kept: the code
// is in the history, the numbers in profiles/r03_ragged_filter_variants.txt, the reading in DESIGN.md "The ragged filter".)

// ---------------------------------------------------------------------------------------------------
// Level-1 compaction in ONE kernel: every workgroup owns a
// contiguous run of tiles, obtains the number of survivors before its run by reducing the (small, L2-resident)
// per-tile count array itself - redundant across workgroups but far cheaper than a dependent scan launch -
// scans its own tiles' counts in LDS, and expands its bitmap words into the index-ordered survivor list.
// The last workgroup also publishes the total.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_compact1(const u64* __restrict__ bitmap, const u32* __restrict__ counts, u32 n_items_host, const u32* __restrict__ n_items_ptr,
                                                  const u32* __restrict__ src, u32* __restrict__ out_idx, u32* __restrict__ total_out,
                                                  u32* __restrict__ total_out2) {
    compact1_body(bitmap, counts, n_items_host, n_items_ptr, src, out_idx, total_out, total_out2, [](u32, u32) {}, [](u32) {});
}

// ---------------------------------------------------------------------------------------------------
// Level-2 compaction (after the lane-exact prefilter re-decided the filter's survivors), same scheme, one kernel:
// here most items are kept, so the work is laid out per ITEM - the gathers of the kept items' haystack index and
// window are coalesced - with the per-word offsets of a batch of tiles prepared once in LDS.
// ---------------------------------------------------------------------------------------------------
#define FZB_C2_BATCH 64  // tiles per batch: 64 x 16 word offsets in LDS
__global__ __launch_bounds__(256) void k_compact2(const u64* __restrict__ bitmap, const u32* __restrict__ counts, const u32* __restrict__ n_items_ptr,
                                                  const u32* __restrict__ in_idx, const u32* __restrict__ in_win, u32* __restrict__ out_idx, u32* __restrict__ out_win,
                                                  u32* __restrict__ total_out) {
    __shared__ u32 red[4];
    __shared__ u32 pre[FZB_C2_BATCH];
    __shared__ u32 woff[FZB_C2_BATCH * (FZB_TILE / 64)];
    const u32 tid = threadIdx.x;
    const u32 n_items = *n_items_ptr;
    const u32 ntiles = (n_items + FZB_TILE - 1) / FZB_TILE;
    u32 t0, t1;
    tc_run(ntiles, tc_tiles_per_run(ntiles, gridDim.x), blockIdx.x, &t0, &t1);
    u32 base = tc_prefix(counts, t0, red);
    const u32 nwords = (n_items + 63) / 64;
    for (u32 tb = t0; tb < t1; tb += FZB_C2_BATCH) {
        const u32 nt = min((u32)FZB_C2_BATCH, t1 - tb);
        const u32 c_tile = tid < nt ? counts[tb + tid] : 0u;
        // offset of every bitmap word inside its tile: 16-lane segmented scan of the popcounts
        const u32 w0 = tb * (FZB_TILE / 64), w1 = (tb + nt) * (FZB_TILE / 64);
        for (u32 wb0 = w0; wb0 < w1; wb0 += 256) {
            const u32 w = wb0 + tid;
            const u32 c = (w < w1 && w < nwords) ? (u32)__popcll(bitmap[w]) : 0u;
            if (w < w1) woff[w - w0] = tc_scan16(c) - c;
        }
        // exclusive scan of the batch's tile counts (its second barrier publishes woff too)
        const u32 batch_total = tc_batch_scan<FZB_C2_BATCH>(c_tile, base, pre, red);
        const u32 j0 = tb * FZB_TILE, j1 = min((tb + nt) * FZB_TILE, n_items);
        for (u32 j = j0 + tid; j < j1; j += 256) {
            const u32 w = j >> 6;
            const u64 bits = bitmap[w];
            if (!((bits >> (j & 63)) & 1)) continue;
            const u32 pos = tc_rank64(pre[j / FZB_TILE - tb] + woff[w - w0], bits, j & 63);
            out_idx[pos] = in_idx ? in_idx[j] : j;
            *(uint2*)(out_win + 2 * (size_t)pos) = *(const uint2*)(in_win + 2 * (size_t)j);
        }
        base += batch_total;
        __syncthreads();  // the next batch overwrites woff
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) *total_out = base;
}

// ---------------------------------------------------------------------------------------------------
// The same accept tests over an ITEM LIST (positions j -> haystack items[j]) whose length lives in device memory:
// the narrowing step of the multi-pattern composition (src/matcher/multi.rs:102-118 re-matches each further pattern
// against only the haystacks that survived the previous ones).  Candidates are a small, sparse subset, so this is
// one plain thread per item; the decisions leave in the usual bitmap + per-1024 counts, indexed by list position.
// ---------------------------------------------------------------------------------------------------
template <typename TW, int MODE, typename ET>
__global__ __launch_bounds__(256) void k1_items(const u8* __restrict__ bytes, const ET* __restrict__ ends, u64 first, const u32* __restrict__ items,
                                                const u32* __restrict__ n_items_ptr, const u64* __restrict__ Tg, int rows, int need, u32 min_len,
                                                u64* __restrict__ bitmap, u32* __restrict__ tile_counts) {
    __shared__ TW T[256];
    T[threadIdx.x] = (TW)Tg[threadIdx.x];  // (published by the flag pass' first barrier)
    const u32 count = *n_items_ptr;
    tc_flag_pass<true>(count, bitmap, tile_counts, [&](u32 tile, u32 slot) {
        const u32 j = tile * FZB_TILE + slot;
        bool matched = false;
        if (j < count) {
            u64 s;
            u32 L;
            haystack_span(ends, first + items[j], s, L);
            if (L >= min_len) {
                const uint4* vp = (const uint4*)(bytes + s);
                TW st = (MODE == 1) ? (TW)1 : (TW)~(TW)0;
                const u32 nvec = (L + 15) >> 4;
                for (u32 v = 0; v < nvec; v++) {
                    const uint4 q = vp[v];
                    const u32 rem = L - 16 * v;
                    filter_word<TW, MODE>(st, q.x, rem, T);
                    if (rem > 4) filter_word<TW, MODE>(st, q.y, rem - 4, T);
                    if (rem > 8) filter_word<TW, MODE>(st, q.z, rem - 8, T);
                    if (rem > 12) filter_word<TW, MODE>(st, q.w, rem - 12, T);
                }
                if (MODE == 1) {
                    matched = (st >> rows) & 1;
                } else {
                    const TW low = rows >= (int)(8 * sizeof(TW)) ? (TW)~(TW)0 : (((TW)1 << rows) - 1);
                    const TW z = ~st & low;
                    const int lcs = sizeof(TW) == 8 ? __popcll((u64)z) : __popc((u32)z);
                    matched = lcs >= need;
                }
            }
        }
        return matched;
    });
}

// ---------------------------------------------------------------------------------------------------
// K1-ITEMS-DFA: the item-list filter for LARGE candidate sets - a narrowing keystroke over a captured match set, a query over the visible
// haystacks of a sparse scope (fzb_subset): 10^5 .. 10^6 items, where k1_items' one-item-at-a-time chain of dependent round trips (item ->
// end offset -> vectors, then the bit-vector automaton out of a 256-entry table) is what the kernel waits for.  Fuzzy matching, an ASCII
// needle, 0 typos only: the automaton is k1_dfa's - `dfa` in LDS at address 0 (dfa_lds.h), same min_len test - and its decisions are k1_dfa's
// on the same rows, bit for bit.  Outputs are k1_items': one bitmap bit per LIST POSITION and the per-1024 tile counts; k_compact1's item
// form follows as before.  The per-item decision is items_filter.h's (fuzzed on the host).
//   SHORT (the list's max_len is known and <= 32): a thread owns positions p * 256 + tid, p = 0..3, of a tile.  Its four items[] loads are
//     issued first, then the four end offsets (none under a uniform-length promise) and - SIG: a list with letter signatures, an eligible
//     needle - the four 4-byte signatures, then all (up to) eight 16-byte row loads, all before the first automaton step; rows that fail the
//     signature or the length test are never requested.  The four chains advance interleaved through dfa_word4, one wait per round.
//   ragged (max_len unknown or beyond 32): a thread per item, a loop over the row's vectors with the next one requested one ahead.
// One ballot word per wave, one LDS atomic per wave, one tile-count store per tile.  No ordering between workgroups.
// ---------------------------------------------------------------------------------------------------
struct ItemsLdsStep {  // the automaton's step for items_filter.h: the table at LDS address 0, row pitch FZB_DFA_STRIDE
    __device__ __forceinline__ u32 operator()(u32 st, u32 b) const { return (u32) * (const __attribute__((address_space(3))) u8*)(uintptr_t)(st * FZB_DFA_STRIDE + b); }
};
template <typename ET, bool SIG, bool SHORT>
__global__ __launch_bounds__(256) void k1_items_dfa(const u8* __restrict__ bytes, const ET* __restrict__ ends, const u32* __restrict__ sig, u32 nsig, u64 first,
                                                    const u32* __restrict__ items, const u32* __restrict__ n_items_ptr, const u8* __restrict__ dfa_g, int rows, u32 min_len,
                                                    u32 acc_lo, u64* __restrict__ bitmap, u32* __restrict__ tile_counts, u32 ulen) {
    extern __shared__ __attribute__((aligned(16))) u8 dfa[];
    u32& s_cnt = *(u32*)(dfa + FZB_DFA_LDS_BYTES(rows));
    const int tid = threadIdx.x;
    dfa_require_lds_base0(dfa);
    dfa_load_lds(dfa, dfa_g, rows);
    const u32 count = *n_items_ptr;
    const u32 ntiles = (count + FZB_TILE - 1) / FZB_TILE;
    const ItemsLdsStep step;
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        u32 cnt = 0;
        if constexpr (SHORT) {
            u32 it[4], sg[4], hl[4];
            u64 hs[4];
            bool want[4];
            uint4 v0[4], v1[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const u32 j = tile * FZB_TILE + p * 256 + tid;
                it[p] = j < count ? items[j] : 0xFFFFFFFFu;
            }
#pragma unroll
            for (int p = 0; p < 4; p++) {
                hs[p] = 0;
                hl[p] = 0;
                sg[p] = 0;
                if (it[p] != 0xFFFFFFFFu) {
                    haystack_span_u(ends, ulen, first + it[p], hs[p], hl[p]);
                    if (SIG) sg[p] = sig[first + it[p]];
                }
            }
#pragma unroll
            for (int p = 0; p < 4; p++) {
                want[p] = it[p] != 0xFFFFFFFFu && items_wants_row(SIG, sg[p], nsig, hl[p], min_len);
                // (a row that is not wanted is never requested: its chain runs over zeros - so a thread whose rows are all full vectors keeps
                // the interleaved form - and its outcome is not looked at)
                v0[p] = make_uint4(0, 0, 0, 0);
                v1[p] = make_uint4(0, 0, 0, 0);
                const uint4* vp = (const uint4*)(bytes + hs[p]);
                if (want[p] && hl[p] > 0) v0[p] = vp[0];
                if (want[p] && hl[p] > 16) v1[p] = vp[1];
            }
            u32 st[4] = {0, 0, 0, 0};
            if (hl[0] >= 16 && hl[1] >= 16 && hl[2] >= 16 && hl[3] >= 16) {
                { const u32 w[4] = {v0[0].x, v0[1].x, v0[2].x, v0[3].x}; dfa_word4<true>(st, w, dfa); }
                { const u32 w[4] = {v0[0].y, v0[1].y, v0[2].y, v0[3].y}; dfa_word4<true>(st, w, dfa); }
                { const u32 w[4] = {v0[0].z, v0[1].z, v0[2].z, v0[3].z}; dfa_word4<true>(st, w, dfa); }
                { const u32 w[4] = {v0[0].w, v0[1].w, v0[2].w, v0[3].w}; dfa_word4<true>(st, w, dfa); }
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const u32 w[4] = {v0[p].x, v0[p].y, v0[p].z, v0[p].w};
                    st[p] = items_chain_vec(st[p], w, items_vec_bytes(hl[p], 0), step);
                }
            }
            if (hl[0] >= 32 && hl[1] >= 32 && hl[2] >= 32 && hl[3] >= 32) {
                { const u32 w[4] = {v1[0].x, v1[1].x, v1[2].x, v1[3].x}; dfa_word4<true>(st, w, dfa); }
                { const u32 w[4] = {v1[0].y, v1[1].y, v1[2].y, v1[3].y}; dfa_word4<true>(st, w, dfa); }
                { const u32 w[4] = {v1[0].z, v1[1].z, v1[2].z, v1[3].z}; dfa_word4<true>(st, w, dfa); }
                { const u32 w[4] = {v1[0].w, v1[1].w, v1[2].w, v1[3].w}; dfa_word4<true>(st, w, dfa); }
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const u32 w[4] = {v1[p].x, v1[p].y, v1[p].z, v1[p].w};
                    st[p] = items_chain_vec(st[p], w, items_vec_bytes(hl[p], 1), step);
                }
            }
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const u64 b = __ballot(want[p] && st[p] >= acc_lo);
                if (lane_id() == 0) {
                    bitmap[(tile * FZB_TILE + p * 256) / 64 + (tid >> 6)] = b;
                    cnt += __popcll(b);
                }
            }
        } else {
#pragma unroll 1
            for (int p = 0; p < FZB_TILE / 256; p++) {
                const u32 j = tile * FZB_TILE + p * 256 + tid;
                bool matched = false;
                if (j < count) {
                    const u32 it = items[j];
                    u64 s;
                    u32 L;
                    haystack_span_u(ends, ulen, first + it, s, L);
                    if (items_wants_row(false, 0u, 0u, L, min_len)) {
                        const uint4* vp = (const uint4*)(bytes + s);
                        const u32 nvec = items_vecs(L);
                        u32 st = 0;
                        uint4 cur = nvec ? vp[0] : make_uint4(0, 0, 0, 0);
                        for (u32 v = 0; v < nvec; v++) {
                            const uint4 nxt = v + 1 < nvec ? vp[v + 1] : make_uint4(0, 0, 0, 0);  // requested ahead of this vector's chain
                            const u32 nb = items_vec_bytes(L, v);
                            if (nb == 16) st = dfa_chain16(st, cur, dfa);
                            else {
                                const u32 w[4] = {cur.x, cur.y, cur.z, cur.w};
                                st = items_chain_vec(st, w, nb, step);
                            }
                            cur = nxt;
                        }
                        matched = st >= acc_lo;
                    }
                }
                const u64 b = __ballot(matched);
                if (lane_id() == 0) {
                    bitmap[(tile * FZB_TILE + p * 256) / 64 + (tid >> 6)] = b;
                    cnt += __popcll(b);
                }
            }
        }
        if (lane_id() == 0 && cnt) atomicAdd(&s_cnt, cnt);
        __syncthreads();
        if (tid == 0) tile_counts[tile] = s_cnt;
        __syncthreads();
    }
}

// Item lists of at least this many items (as far as the host knows: fzb_launch_filter_items' n_hint) take k1_items_dfa where it applies.
// The crossover is measured (profiles/subset.txt, the narrowed match_list_top_device call with only the filter kernel differing, 10 M x
// 32-byte list, us, k1_items -> k1_items_dfa): 1 k candidates 44.1 -> 45.8, 10 k 54.6 -> 57.1, 100 k 61.3 -> 59.9, 1 M 84.9 -> 70.4,
// 5 M 149.8 -> 94.3 with signatures; 100 k 62.0 -> 59.9, 1 M 84.8 -> 80.5, 5 M 150.0 -> 128.4 without: the SHORT form from 100 000 items on.
// The ragged form LOST at every size on the paths-shaped list (1 k 64.6 -> 76.0, 100 k 96.7 -> 109.2, 1 M 129.0 -> 152.4): it is not
// selected; only the tests' hook (fzb_debug_set_items_dfa_min) reaches it.
#define FZB_ITEMS_DFA_MIN_SHORT 100000u
#define FZB_ITEMS_DFA_MIN_RAGGED 0xFFFFFFFFu
static u32 g_items_dfa_min_short = FZB_ITEMS_DFA_MIN_SHORT, g_items_dfa_min_ragged = FZB_ITEMS_DFA_MIN_RAGGED;
extern "C" void fzb_debug_set_items_dfa_min(uint32_t n) {
    g_items_dfa_min_short = n ? n : FZB_ITEMS_DFA_MIN_SHORT;
    g_items_dfa_min_ragged = n ? n : FZB_ITEMS_DFA_MIN_RAGGED;
}
bool fzb_filter_items_dfa_applies(const CorpusDev& c, int mode, int exact, const u8* dfa, int rows, u64 n_hint) {
    const bool shortc = c.max_len != 0 && c.max_len <= 32;
    return mode == 1 && exact && dfa && rows >= 1 && rows <= FZB_MAX_ROWS && !fzb_knobs().no_items_dfa && n_hint != 0 && n_hint >= (u64)(shortc ? g_items_dfa_min_short : g_items_dfa_min_ragged);
}

void fzb_launch_filter_items(const CorpusDev& c, u64 first, const u32* items, const u32* n_items_ptr, const u64* table, int rows, int mode, int need, u32 min_len,
                             u64* bitmap, u32* tile_counts, int grid, hipStream_t st, const u8* dfa, int exact, u32 needle_sig, int sig_ok, u64 n_hint) {
    // dfa / exact / needle_sig / sig_ok / n_hint: a candidate set's item list (host.hip) - fuzzy, ASCII, 0 typos, `dfa` = the subsequence
    // automaton (rows + 1 states, accept in the last), n_hint = what the host knows of the list's length (0: a few thousand at most)
    if (fzb_filter_items_dfa_applies(c, mode, exact, dfa, rows, n_hint)) {
        const size_t lds = (size_t)(rows + 1) * FZB_DFA_STRIDE + 16;  // table + the tile counter
        const bool shortc = c.max_len != 0 && c.max_len <= 32;
        const bool use_sig = shortc && fzb_filter_sig_applies(c, mode, needle_sig, sig_ok);
        const u64 tiles = (n_hint + FZB_TILE - 1) / FZB_TILE;
        const int g = (int)std::max<u64>(1, std::min<u64>((u64)std::max(1, grid) * 2, tiles));  // (`grid` = 4 workgroups per CU: 8 here, every wave slot, as k1_dfa)
#define FZB_K1ID(ET, SIG, SHORT) FZB_LAUNCH((k1_items_dfa<ET, SIG, SHORT>), dim3(g), dim3(256), lds, st, c.bytes, (const ET*)c.ends, c.sig, needle_sig, first, items, n_items_ptr, dfa, rows, min_len, (u32)rows, bitmap, tile_counts, c.uniform_len)
        if (c.ends_u64) { if (use_sig) FZB_K1ID(u64, true, true); else if (shortc) FZB_K1ID(u64, false, true); else FZB_K1ID(u64, false, false); }
        else            { if (use_sig) FZB_K1ID(u32, true, true); else if (shortc) FZB_K1ID(u32, false, true); else FZB_K1ID(u32, false, false); }
#undef FZB_K1ID
        return;
    }
    // MODE 1 with one-hot state needs rows + 1 bits, MODE 2 rows bits
    const bool w64 = (mode == 1) ? rows > 31 : rows > 32;
#define FZB_K1I(TW, MODE, ET) FZB_LAUNCH((k1_items<TW, MODE, ET>), dim3(grid), dim3(256), 0, st, c.bytes, (const ET*)c.ends, first, items, n_items_ptr, table, rows, need, min_len, bitmap, tile_counts)
    if (c.ends_u64) {
        if (mode == 1) { if (w64) FZB_K1I(u64, 1, u64); else FZB_K1I(u32, 1, u64); }
        else           { if (w64) FZB_K1I(u64, 2, u64); else FZB_K1I(u32, 2, u64); }
    } else {
        if (mode == 1) { if (w64) FZB_K1I(u64, 1, u32); else FZB_K1I(u32, 1, u32); }
        else           { if (w64) FZB_K1I(u64, 2, u32); else FZB_K1I(u32, 2, u32); }
    }
#undef FZB_K1I
}

// ---------------------------------------------------------------------------------------------------
// The signatures' BIT-PLANES (sig_filter.h) of the tiles [t0, tiles of n), built from the u32 signatures fzb_sig_sync has just written:
// a workgroup per tile and trip reads the tile's 4 KB coalesced (zero at and beyond n), every wave turns 64 rows into 32 ballots - lane b
// keeps plane b's word -, the tile's 512 words meet in LDS and leave as one coalesced 4 KB store.
// ---------------------------------------------------------------------------------------------------
// (the two halves both builds share: the 32 bits `s` of row p * 256 + tid of a tile into the tile's words in LDS, and the tile's store)
__device__ __forceinline__ void sig_planes_put(u32 s, u32 p, u64* s_pl) {
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u64 mine = 0;
    for (u32 b = 0; b < 32; b++) {
        const u64 bal = __ballot((s >> b) & 1u);
        if (lane == b) mine = bal;
    }
    if (lane < 32) s_pl[lane * FZB_SIG_PLANE_WORDS + p * 4 + wave] = mine;  // (rows p * 256 + wave * 64 ..: word p * 4 + wave)
}
__device__ __forceinline__ void sig_planes_store(const u64* s_pl, u64* __restrict__ planes, u64 tile) {
    const u32 tid = threadIdx.x;
    __syncthreads();
    u64* out = planes + sig_plane_index(tile, 0, 0);
    out[tid] = s_pl[tid];
    out[tid + 256] = s_pl[tid + 256];
    __syncthreads();
}
__global__ __launch_bounds__(256) void k_sig_planes_build(const u32* __restrict__ sig, u64 n, u64 t0, u64* __restrict__ planes) {
    __shared__ u64 s_pl[32 * FZB_SIG_PLANE_WORDS];
    const u64 tiles = sig_plane_tiles(n);
    for (u64 tile = t0 + blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
        for (u32 p = 0; p < FZB_TILE / 256; p++) {
            const u64 i = tile * FZB_TILE + p * 256 + threadIdx.x;
            sig_planes_put(i < n ? sig[i] : 0u, p, s_pl);
        }
        sig_planes_store(s_pl, planes, tile);
    }
}
void fzb_launch_sig_planes(const u32* sig, u64 n, u64 t0, u64* planes, int grid, hipStream_t st) {
    FZB_LAUNCH(k_sig_planes_build, dim3(std::max(1, grid)), dim3(256), 0, st, sig, n, t0, planes);
}
// The REPEAT planes (sig_filter.h) of the tiles [t0, tiles of n), built from the haystack BYTES - the u32 signatures carry no counts, and no
// per-haystack array of repeat signatures stays behind: every thread derives its row's repeat signature as k_sig_build derives the signature
// (both 16-byte vectors, cut to the row's length; uniform and ragged lists, u32 and u64 end offsets), then the ballots and the tile's store
// as above.
template <typename ET>
__global__ __launch_bounds__(256) void k_sig_planes2_build(const u8* __restrict__ bytes, const ET* __restrict__ ends, u32 ulen, u64 n, u64 t0, u64* __restrict__ planes2) {
    __shared__ u64 s_pl[32 * FZB_SIG_PLANE_WORDS];
    const u64 tiles = sig_plane_tiles(n);
    for (u64 tile = t0 + blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll
        for (u32 p = 0; p < FZB_TILE / 256; p++) {
            const u64 i = tile * FZB_TILE + p * 256 + threadIdx.x;
            u32 once = 0, s = 0;
            if (i < n) {
                u64 hs;
                u32 L;
                haystack_span_u(ends, ulen, i, hs, L);
                L = min(L, 32u);  // (the list's bound, as in k_sig_build)
                const uint4* vp = (const uint4*)(bytes + hs);
                uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
                if (L > 0) a = vp[0];
                if (L > 16) b = vp[1];
                u32 w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const u32 nvb = L > 4u * q ? L - 4u * q : 0u;
                    if (nvb < 4) w[q] &= (1u << (8 * nvb)) - 1;
                    sig2_accum_word(w[q], once, s);
                }
            }
            sig_planes_put(s, p, s_pl);
        }
        sig_planes_store(s_pl, planes2, tile);
    }
}
void fzb_launch_sig_planes2(const CorpusDev& c, u64 n, u64 t0, u64* planes2, int grid, hipStream_t st) {
    if (c.ends_u64) FZB_LAUNCH((k_sig_planes2_build<u64>), dim3(std::max(1, grid)), dim3(256), 0, st, c.bytes, (const u64*)c.ends, c.uniform_len, n, t0, planes2);
    else FZB_LAUNCH((k_sig_planes2_build<u32>), dim3(std::max(1, grid)), dim3(256), 0, st, c.bytes, (const u32*)c.ends, c.uniform_len, n, t0, planes2);
}

// ---------------------------------------------------------------------------------------------------
// host-side launch wrappers (called from host.hip)
// ---------------------------------------------------------------------------------------------------
bool fzb_filter_sig_applies(const CorpusDev& c, int mode, u32 needle_sig, int sig_ok) {
    return mode == 1 && c.max_len != 0 && c.max_len <= 32 && sig_ok && needle_sig && c.sig && !fzb_knobs().no_signature;
}

void fzb_launch_filter(const CorpusDev& c, u64 first, u32 count, const u64* table, const u8* dfa, u32 dead, int rows, int mode, int need, u32 min_len,
                       u64* bitmap, u32* tile_counts, u32* reset_counters, int grid, hipStream_t st, u64* bitmap_m, u32* tile_counts_m, u64* reject_bits, u32* tile_rejects, int nul_safe,
                       int acc_lo, const u8* cdfa, u32 cdfa_bytes, int cdfa_K, int cdfa_G, u32 needle_sig, int sig_ok, const SegList* seg, u32 needle_sig2) {
    // mode 1: `dfa` has rows + 1 states, start state 0, and accepts in the states >= acc (the subsequence / unicode / KMP automata: the last
    // state; the LCS automaton of a typo configuration: every state whose LCS reaches the need)
    const u32 acc = acc_lo < 0 ? (u32)rows : (u32)acc_lo;
    const u32 ntiles = (count + FZB_TILE - 1) / FZB_TILE;
    const int cus = std::max(1, grid / 8);  // (`grid` = 8 workgroups per CU = every wave slot)
    if (grid > (int)ntiles) grid = ntiles;
    if (grid < 1) grid = 1;
    if (mode == 1) {
        const size_t lds = (size_t)(rows + 1) * FZB_DFA_STRIDE + 16;  // table + the tile counter
        const bool shortc = c.max_len != 0 && c.max_len <= 32;  // every haystack fits the two pre-requested vectors
        if (fzb_filter_sig_applies(c, mode, needle_sig, sig_ok)) {  // an eligible needle over a list with signatures (host.hip decides eligibility)
            const u32 gmax = std::min<u32>(FZB_SIG_GATHER_MAX, FZB_TILE);
            // u32 form: + the tile's decision bits and the queue of passing rows; plane form: + a batch's tile counts, candidate words, decision bits and queue
            const bool planes = seg && c.sig_planes && first % FZB_TILE == 0 && !fzb_knobs().no_sig_planes;
            const size_t lds_s = planes ? FZB_DFA_LDS_BYTES(rows) + FZB_SIG_BATCH_TILES * (4 + 256 + 2 * (size_t)gmax) : lds + 128 + 2 * FZB_TILE;
#define FZB_K1S(ET, SEG, PL, G, S) FZB_LAUNCH((k1_dfa_sig<ET, SEG, PL>), dim3(G), dim3(256), lds_s, st, c.bytes, (const ET*)c.ends, PL ? (const u32*)c.sig_planes : c.sig, needle_sig, first, count, dfa, rows, min_len, acc, bitmap, tile_counts, reset_counters, c.uniform_len, gmax, S, PL ? c.sig_planes2 : nullptr, PL ? nsig2 : 0u)
            // the needle's repeat signature where the plane form reads a corpus with repeat planes: rows missing a doubled letter are no candidates
            const u32 nsig2 = planes && c.sig_planes2 ? needle_sig2 : 0u;
            if (planes) {  // ... from the corpus' bit-planes, a run's tiles in batches (an aligned range; FZB_NO_SIG_PLANES unset)
                if (g_fzb_record_grids) fzb_record_grid("k1_dfa_sig_planes", seg->nseg);  // (the kernel's name does not say which form ran: a second record for the tests)
                if (g_fzb_record_grids && nsig2) fzb_record_grid("k1_dfa_sig_repeat", seg->nseg);
                if (c.ends_u64) FZB_K1S(u64, true, true, seg->nseg, *seg); else FZB_K1S(u32, true, true, seg->nseg, *seg);
            } else if (seg) {  // the filter lists its survivors: one workgroup per segment
                if (c.ends_u64) FZB_K1S(u64, true, false, seg->nseg, *seg); else FZB_K1S(u32, true, false, seg->nseg, *seg);
            } else {
                if (c.ends_u64) FZB_K1S(u64, false, false, grid, SegList{}); else FZB_K1S(u32, false, false, grid, SegList{});
            }
#undef FZB_K1S
            return;
        }
        if (shortc) {
#define FZB_K1D(ET) FZB_LAUNCH((k1_dfa<ET>), dim3(grid), dim3(256), lds, st, c.bytes, (const ET*)c.ends, first, count, dfa, rows, min_len, dead, acc, bitmap, tile_counts, reset_counters, c.uniform_len)
            if (c.ends_u64) FZB_K1D(u64); else FZB_K1D(u32);
#undef FZB_K1D
            return;
        }
        // Ragged lists: one haystack per thread.  Three forms, best first: the class-composite automaton over the corpus' filter VIEW (6 resident
        // workgroups per CU: C4 shard 8 -> 190 us, 6 -> 187, 4 -> 194), the same automaton over the canonical layout (5 per CU: 8 -> 247 us,
        // 5 -> 232) when the corpus has no view or the range is not tile-aligned, and the byte automaton in its burst form (8 per CU) when the
        // composite table does not fit (host.hip: states x K^G <= 16 KB) or FZB_NO_CDFA=1 asks for it.
        const FzbKnobs& kn = fzb_knobs();
        const bool composite = cdfa && !kn.no_cdfa && (cdfa_G == 4 || cdfa_G == 2);
        u32 kg = 1;
        for (int i = 0; i < cdfa_G; i++) kg *= (u32)cdfa_K;
        if (composite && c.vbytes && !kn.no_filter_view && first % FZB_TILE == 0 && (first + count == c.n || count % FZB_TILE == 0) && c.view_nv != 0 && c.view_nv <= 16) {
            const size_t lds_v = ((cdfa_bytes + 15) & ~(size_t)15) + 16 + 128;
            const int g = std::max(1, std::min<int>(cus * 6, (int)ntiles));
            // (the lengths are not read when nothing needs them: acc >= 1 = the start state does not accept)
            const bool len_free = nul_safe && acc >= 1;
            // short lists (fewer tiles than two per CU, the common form only): 1024-thread workgroups, one group per wave.  Filter / step, us:
            // 100 k paths 14.5 -> 8.3 / 39.8 -> 34.0, 300 k 16.5 -> 13.7 / 42.9 -> 40.6, 0.5 M 8..128-byte items 18.1 -> 12.7 / 55.3 -> 49.1; from
            // 1.4 M items (1 374 tiles) on the 256-thread form's six workgroups per CU win (34.5 against 38.3)
            const bool wide = nul_safe && len_free && ntiles < (u32)cus * 2u;
#define FZB_K1VA const_cast<const u8*>(c.vbytes), c.vgofs, c.vgnv, c.vlen, c.vperm, first, count, cdfa, cdfa_bytes, (u32)cdfa_K, kg, min_len, dead, acc, bitmap, tile_counts, reset_counters
#define FZB_K1V(SAN, G, NV, LEN) FZB_LAUNCH((k1_cdfa_view<SAN, G, NV, LEN>), dim3(g), dim3(256), lds_v, st, FZB_K1VA)
#define FZB_K1W(G, NV) FZB_LAUNCH((k1_cdfa_view<false, G, NV, false, 1024>), dim3(g), dim3(1024), lds_v, st, FZB_K1VA)
#define FZB_K1V_S(SAN, G, NV) do { if (!SAN && wide) FZB_K1W(G, NV); else if (!SAN && len_free) FZB_K1V(SAN, G, NV, false); else FZB_K1V(SAN, G, NV, true); } while (0)
#define FZB_K1V_NV(SAN, G) do { if (c.view_nv <= 8) FZB_K1V_S(SAN, G, 8); else FZB_K1V_S(SAN, G, 16); } while (0)
#define FZB_K1V_G(SAN) do { if (cdfa_G == 4) FZB_K1V_NV(SAN, 4); else FZB_K1V_NV(SAN, 2); } while (0)
            if (nul_safe) FZB_K1V_G(false); else FZB_K1V_G(true);
#undef FZB_K1V_G
#undef FZB_K1V_NV
#undef FZB_K1V_S
#undef FZB_K1W
#undef FZB_K1V
#undef FZB_K1VA
            if (c.n_long) {  // the haystacks beyond 256 bytes: decided from the canonical layout, OR-ed into the view kernel's bitmap
                const u32 ns_o = (cdfa_bytes - 256u) / kg;  // the automaton's states (the table is padded to 16 bytes: at most a phantom state more)
                const u32 wpw = ((cdfa_bytes + 15) & ~(size_t)15) + (size_t)4 * 64 * ns_o + 16 <= 60 * 1024 ? 4u : 1u;
                const size_t lds_o = ((cdfa_bytes + 15) & ~(size_t)15) + (size_t)wpw * 64 * ns_o + 16;
                const int go = (int)std::max<u32>(1u, std::min<u32>((c.n_long + wpw - 1) / wpw, (u32)cus * 16u));  // (4096 on 256 CUs)
#define FZB_K1O(ET, SAN, G) FZB_LAUNCH((k1_cdfa_outliers<ET, SAN, G>), dim3(go), dim3(64 * wpw), lds_o, st, c.bytes, (const ET*)c.ends, first, count, c.vlong, c.n_long, cdfa, cdfa_bytes, (u32)cdfa_K, kg, ns_o, min_len, dead, acc, bitmap, tile_counts)
#define FZB_K1O_G(ET, SAN) do { if (cdfa_G == 4) FZB_K1O(ET, SAN, 4); else FZB_K1O(ET, SAN, 2); } while (0)
                if (c.ends_u64) { if (nul_safe) FZB_K1O_G(u64, false); else FZB_K1O_G(u64, true); }
                else            { if (nul_safe) FZB_K1O_G(u32, false); else FZB_K1O_G(u32, true); }
#undef FZB_K1O_G
#undef FZB_K1O
            }
            return;
        }
        if (composite) {
            const size_t lds_c = ((cdfa_bytes + 15) & ~(size_t)15) + 16;
            const int g = std::max(1, std::min<int>(cus * 5, (int)ntiles));
#define FZB_K1CD(ET, SAN, G) FZB_LAUNCH((k1_cdfa_ragged<ET, SAN, G>), dim3(g), dim3(256), lds_c, st, c.bytes, (const ET*)c.ends, first, count, cdfa, cdfa_bytes, (u32)cdfa_K, kg, min_len, dead, acc, bitmap, tile_counts, reset_counters)
#define FZB_K1CD_G(ET, SAN) do { if (cdfa_G == 4) FZB_K1CD(ET, SAN, 4); else FZB_K1CD(ET, SAN, 2); } while (0)
            if (c.ends_u64) { if (nul_safe) FZB_K1CD_G(u64, false); else FZB_K1CD_G(u64, true); }
            else            { if (nul_safe) FZB_K1CD_G(u32, false); else FZB_K1CD_G(u32, true); }
#undef FZB_K1CD_G
#undef FZB_K1CD
            return;
        }
#define FZB_K1B(ET, SAN) FZB_LAUNCH((k1_dfa_ragged_burst<ET, SAN>), dim3(grid), dim3(256), lds, st, c.bytes, (const ET*)c.ends, first, count, dfa, rows, min_len, dead, acc, bitmap, tile_counts, reset_counters)
        if (c.ends_u64) { if (nul_safe) FZB_K1B(u64, false); else FZB_K1B(u64, true); }
        else            { if (nul_safe) FZB_K1B(u32, false); else FZB_K1B(u32, true); }
#undef FZB_K1B
        return;
    }
    const bool w64 = (mode == 1) ? rows > 31 : rows > 32;
    if (mode == 2 && bitmap_m) {  // LCS filter with the "nothing to spare" bit (typo configurations on the short-haystack path)
        const MargOut mo{bitmap_m, tile_counts_m, reject_bits, tile_rejects};
#define FZB_K1M(TW, ET) FZB_LAUNCH((k1_filter<TW, 2, ET, true>), dim3(grid), dim3(256), 0, st, c.bytes, (const ET*)c.ends, first, count, table, rows, need, min_len, bitmap, tile_counts, reset_counters, mo, c.uniform_len)
        if (c.ends_u64) { if (w64) FZB_K1M(u64, u64); else FZB_K1M(u32, u64); }
        else            { if (w64) FZB_K1M(u64, u32); else FZB_K1M(u32, u32); }
#undef FZB_K1M
        return;
    }
#define FZB_K1(TW, MODE, ET) FZB_LAUNCH((k1_filter<TW, MODE, ET>), dim3(grid), dim3(256), 0, st, c.bytes, (const ET*)c.ends, first, count, table, rows, need, min_len, bitmap, tile_counts, reset_counters, MargOut{}, c.uniform_len)
    if (c.ends_u64) {
        if (mode == 1) { if (w64) FZB_K1(u64, 1, u64); else FZB_K1(u32, 1, u64); }
        else           { if (w64) FZB_K1(u64, 2, u64); else FZB_K1(u32, 2, u64); }
    } else {
        if (mode == 1) { if (w64) FZB_K1(u64, 1, u32); else FZB_K1(u32, 1, u32); }
        else           { if (w64) FZB_K1(u64, 2, u32); else FZB_K1(u32, 2, u32); }
    }
#undef FZB_K1
}

// Exclusive prefix of the per-tile reject counts (decide form of k2a_window) - only when something was rejected at all, which on
// real lists is about one haystack in 1e5 of the marginal ones: one workgroup, and an immediate return otherwise.
__global__ __launch_bounds__(1024) void k_scan_rejects(const u32* __restrict__ tile_rejects, u32 ntiles, const u32* __restrict__ reject_count, u32* __restrict__ rej_prefix) {
    if (*reject_count == 0) return;
    __shared__ u32 wsum[16];
    __shared__ u32 carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (u32 t0 = 0; t0 < ntiles; t0 += 1024) {
        const u32 t = t0 + tid;
        const u32 c = t < ntiles ? tile_rejects[t] : 0u;
        u32 incl = c;
        for (int off = 1; off < 64; off <<= 1) {
            const u32 v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        u32 wb = 0;
        for (int w = 0; w < wave; w++) wb += wsum[w];
        if (t < ntiles) rej_prefix[t] = carry + wb + incl - c;
        __syncthreads();
        if (tid == 1023) carry += wb + incl;
        __syncthreads();
    }
}
void fzb_launch_scan_rejects(const u32* tile_rejects, u32 ntiles, const u32* reject_count, u32* rej_prefix, hipStream_t st) {
    FZB_LAUNCH(k_scan_rejects, dim3(1), dim3(1024), 0, st, tile_rejects, ntiles, reject_count, rej_prefix);
}

void fzb_launch_compact1(const u64* bitmap, const u32* counts, u32 n_items, const u32* n_items_ptr, const u32* src, u32* out_idx, u32* total_out, int grid, hipStream_t st,
                         u32* total_out2) {
    FZB_LAUNCH(k_compact1, dim3(grid), dim3(256), 0, st, bitmap, counts, n_items, n_items_ptr, src, out_idx, total_out, total_out2);
}

__global__ void k_init_counters(u32* __restrict__ counters, u32 n0) {
    if (threadIdx.x < 16) counters[threadIdx.x] = threadIdx.x == 0 ? n0 : 0u;
}
void fzb_launch_init_counters(u32* counters, u32 n0, hipStream_t st) { FZB_LAUNCH(k_init_counters, dim3(1), dim3(64), 0, st, counters, n0); }

void fzb_launch_compact2(const u64* bitmap, const u32* counts, const u32* n_items_ptr, const u32* in_idx, const u32* in_win, u32* out_idx, u32* out_win, u32* total_out,
                         int grid, hipStream_t st) {
    FZB_LAUNCH(k_compact2, dim3(grid), dim3(256), 0, st, bitmap, counts, n_items_ptr, in_idx, in_win, out_idx, out_win, total_out);
}
