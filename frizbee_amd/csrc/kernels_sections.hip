// gfx950 kernels of the sectioned top-`limit` (sections.h): the selection stage of kernels_topk.hip done for up to SECTIONS_MAX tag
// sections at once, and the ordering of each section's head in LDS.  The stage takes the index-ordered records where
// fzb_launch_topk_select takes them - behind the scorers (or the composition), the corpus' own scope drop and the bias - so the filter and
// the scorers run ONCE for all sections.  The decisions are sections.h's and topk_select.h's; the kernels add the tag gather, ballots, LDS
// histograms and barriers:
//   k_sec_hist         per-workgroup S x 256 bins in LDS (8 KB at S = 8), one atomic per non-empty bin and workgroup to HBM; level 0 over all
//                      of a section's records, level 1 over the records of the section's own picked high bin
//   k_sec_cut          a workgroup per section: mode 0 = n_s and the high bin, 1 = the cut by score, 2 = the cut by index (n_s from the scan)
//   k_sec_tile_counts  per 2048-record tile and section: members above T_s / equal T_s (2S rows)
//   k_sec_scan         exclusive scans of the 2S rows, a wave per row, and the rows' totals
//   k_sec_scatter      one stable pass: topk_dest per record and section it belongs to, into the slab out[s * limit + d]; the 2S result words
//   k_sec_order        a workgroup per section: the slab's <= 1024 kept records ranked in LDS (sections_rank) and written back in order
//   k_sec_items        (the form with matched positions) the slabs' kept records -> one dense head + the item list of the traced pass
// The record count lives in device memory; no count is read back between the kernels.  Every loop over records, tiles, rows or sections is
// grid-stride with trip counts that are uniform around ballots, shuffles and barriers.
#include "kernels_common.h"
#include "sections.h"

static_assert(sizeof(sections_rec) == sizeof(fzb_match_rec) && alignof(sections_rec) <= alignof(uint64_t), "the ordering moves fzb_match_rec as a whole");
static_assert(sizeof(sections_state) == 16 * sizeof(u32), "16 state words per section");

// scratch layout (u32 words; a buffer of the matcher's own, fzb_sections_scratch_words):
//   [0, 2048) first-level bins, 256 per section   [2048, 4096) second-level bins   [4096, 4224) sections_state x 8
//   [4224 + (k * 8 + s) * ntiles_cap ...) k = 0: tile counts above T_s, 1: tile counts equal T_s, 2 / 3: their exclusive scans
#define SEC_BINS_A 0
#define SEC_BINS_B (SECTIONS_MAX * 256)
#define SEC_STATE (2 * SECTIONS_MAX * 256)
#define SEC_TILES (SEC_STATE + SECTIONS_MAX * 16)

size_t fzb_sections_scratch_words(size_t n_records) { return SEC_TILES + (size_t)4 * SECTIONS_MAX * (n_records / SECTIONS_TILE + 2); }

__device__ __forceinline__ u32 sec_count(const u32* __restrict__ in_count, u32 in_cap) { return min(in_count[0], in_cap); }
__device__ __forceinline__ const sections_state* sec_state(const u32* scratch) { return (const sections_state*)(scratch + SEC_STATE); }
__device__ __forceinline__ u32* sec_row(u32* scratch, u32 ntiles_cap, int k, u32 s) { return scratch + SEC_TILES + (size_t)(k * SECTIONS_MAX + s) * ntiles_cap; }
__device__ __forceinline__ const u32* sec_row(const u32* scratch, u32 ntiles_cap, int k, u32 s) { return scratch + SEC_TILES + (size_t)(k * SECTIONS_MAX + s) * ntiles_cap; }

__global__ __launch_bounds__(256) void k_sec_hist(const fzb_match_rec* __restrict__ in, const u32* __restrict__ in_count, u32 in_cap, const uint16_t* __restrict__ tags, u64 n_tags,
                                                  sections_set ss, u32 limit, int level, int one_pass, u32* __restrict__ scratch) {
    __shared__ u32 h[SECTIONS_MAX * 256];
    __shared__ sections_state st[SECTIONS_MAX];
    const u32 n = sec_count(in_count, in_cap);
    const u32 S = min(ss.n, (u32)SECTIONS_MAX);
    for (u32 b = threadIdx.x; b < S * 256u; b += 256u) h[b] = 0;
    if (level == 1 && threadIdx.x < S) st[threadIdx.x] = sec_state(scratch)[threadIdx.x];
    __syncthreads();
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const fzb_match_rec r = in[i];
        const u32 score = r.score;
        u32 m = sections_mask(ss, scope_tag_of(tags, n_tags, 0, 0, r.index));
        while (m) {
            const u32 s = (u32)__ffs(m) - 1u;
            m &= m - 1u;
            if (level == 0) atomicAdd(&h[s * 256u + sections_bin_first(score, one_pass)], 1u);
            else if (sections_in_lo(st[s], limit, score)) atomicAdd(&h[s * 256u + (score & 255u)], 1u);
        }
    }
    __syncthreads();
    u32* const bins = scratch + (level == 0 ? SEC_BINS_A : SEC_BINS_B);
    for (u32 b = threadIdx.x; b < S * 256u; b += 256u) {
        const u32 c = h[b];
        if (c) atomicAdd(&bins[b], c);
    }
}

// mode 0: two levels - n_s and the high bin from the first-level bins; mode 1: the cut by score (one_pass: from the first-level bins, which
// also give n_s); mode 2: the cut by index, n_s = the total of the section's tie row.  The bins are staged in LDS and one thread walks them
// with the functions the host tests fuzz.
__global__ __launch_bounds__(256) void k_sec_cut(u32 n_sections, u32 limit, int mode, int one_pass, int desc, u32* __restrict__ scratch) {
    __shared__ u32 bins[256];
    sections_state* const all = (sections_state*)(scratch + SEC_STATE);
    for (u32 s = blockIdx.x; s < n_sections; s += gridDim.x) {
        if (mode != 2) bins[threadIdx.x] = scratch[((mode == 0 || one_pass) ? SEC_BINS_A : SEC_BINS_B) + s * 256u + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) {
            sections_state st = all[s];
            if (mode == 0) {
                sections_pick_hi(bins, limit, &st);
            } else {
                if (mode == 2) {
                    st.n = st.tot_eq;
                    st.cut = topk_cut_by_index(st.n, limit, desc);
                } else {
                    if (one_pass) {
                        st.n = sections_sum(bins);
                        st.hi_bin = 0;
                        st.above_hi = 0;
                    }
                    st.cut = sections_cut_score(st.n, st.hi_bin, st.above_hi, bins, limit, desc);
                }
                st.kept = sections_kept(st.cut, st.n, limit);
            }
            all[s] = st;
        }
        __syncthreads();
    }
}

// the class (sections_class) of the record in every section, two bits per section; 0 for a lane without a record
__device__ __forceinline__ u32 sec_classes(const sections_set& ss, const TopkCut* cuts, int by_score, bool valid, u32 tag, u32 score) {
    u32 cls = 0;
    if (valid) {
        u32 m = sections_mask(ss, tag);
        while (m) {
            const u32 s = (u32)__ffs(m) - 1u;
            m &= m - 1u;
            cls |= sections_class(cuts[s], by_score, score) << (2u * s);
        }
    }
    return cls;
}

// per tile and section: members above T_s, members equal T_s (by index / nothing to remove: every member counts as a tie)
__global__ __launch_bounds__(256) void k_sec_tile_counts(const fzb_match_rec* __restrict__ in, const u32* __restrict__ in_count, u32 in_cap, const uint16_t* __restrict__ tags,
                                                         u64 n_tags, sections_set ss, int by_score, u32* __restrict__ scratch, u32 ntiles_cap) {
    __shared__ u32 acc[2 * SECTIONS_MAX];
    __shared__ TopkCut cuts[SECTIONS_MAX];
    const u32 S = min(ss.n, (u32)SECTIONS_MAX);
    if (threadIdx.x < S) cuts[threadIdx.x] = sec_state(scratch)[threadIdx.x].cut;  // (by index: not read - sections_class decides before it looks)
    const u32 n = sec_count(in_count, in_cap);
    const u32 ntiles = min((n + SECTIONS_TILE - 1) / SECTIONS_TILE, ntiles_cap);
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (threadIdx.x < 2 * SECTIONS_MAX) acc[threadIdx.x] = 0;
        __syncthreads();
        const u32 lo = tile * SECTIONS_TILE, hi = min(lo + SECTIONS_TILE, n);
        u32 g[SECTIONS_MAX], e[SECTIONS_MAX];  // wave-uniform
#pragma unroll
        for (int s = 0; s < SECTIONS_MAX; s++) g[s] = e[s] = 0;
        for (u32 base = lo; base < hi; base += 256) {
            const u32 i = base + threadIdx.x;
            const bool valid = i < hi;
            u32 tag = 0, score = 0;
            if (valid) {
                const fzb_match_rec r = in[i];
                score = r.score;
                tag = scope_tag_of(tags, n_tags, 0, 0, r.index);
            }
            const u32 cls = sec_classes(ss, cuts, by_score, valid, tag, score);
#pragma unroll
            for (int s = 0; s < SECTIONS_MAX; s++) {
                if ((u32)s < S) {
                    g[s] += __popcll(__ballot(((cls >> (2 * s)) & 3u) == 1u));
                    e[s] += __popcll(__ballot(((cls >> (2 * s)) & 3u) == 2u));
                }
            }
        }
        if (lane_id() == 0) {
#pragma unroll
            for (int s = 0; s < SECTIONS_MAX; s++) {
                if (g[s]) atomicAdd(&acc[s], g[s]);
                if (e[s]) atomicAdd(&acc[SECTIONS_MAX + s], e[s]);
            }
        }
        __syncthreads();
        if (threadIdx.x < 2 * SECTIONS_MAX && (threadIdx.x & (SECTIONS_MAX - 1)) < S)
            sec_row(scratch, ntiles_cap, threadIdx.x / SECTIONS_MAX, threadIdx.x & (SECTIONS_MAX - 1))[tile] = acc[threadIdx.x];
        __syncthreads();
    }
}

// exclusive scans of the 2S tile-count rows, a wave per row (row = k * S + s), and each row's total
__global__ __launch_bounds__(64) void k_sec_scan(const u32* __restrict__ in_count, u32 in_cap, u32 n_sections, u32* __restrict__ scratch, u32 ntiles_cap) {
    const u32 n = sec_count(in_count, in_cap);
    const u32 ntiles = min((n + SECTIONS_TILE - 1) / SECTIONS_TILE, ntiles_cap);
    const int lane = lane_id();
    sections_state* const all = (sections_state*)(scratch + SEC_STATE);
    for (u32 row = blockIdx.x; row < 2 * n_sections; row += gridDim.x) {
        const int k = row / n_sections;
        const u32 s = row % n_sections;
        const u32* const cnt = sec_row(scratch, ntiles_cap, k, s);
        u32* const off = sec_row(scratch, ntiles_cap, 2 + k, s);
        u32 carry = 0;
        for (u32 t0 = 0; t0 < ntiles; t0 += 64) {  // uniform trip count: every lane takes part in the shuffles
            const u32 t = t0 + lane;
            const u32 v = t < ntiles ? cnt[t] : 0u;
            u32 incl = v;
            for (int o = 1; o < 64; o <<= 1) {
                const u32 x = __shfl_up(incl, o);
                if (lane >= o) incl += x;
            }
            if (t < ntiles) off[t] = carry + incl - v;
            carry += __shfl(incl, 63);
        }
        if (lane == 0) {
            if (k == 0) all[s].tot_gt = carry;
            else all[s].tot_eq = carry;
        }
    }
}

// the stable scatter of every section in one pass over the records; writes counts[2s] = kept_s, counts[2s + 1] = n_s
__global__ __launch_bounds__(256) void k_sec_scatter(const fzb_match_rec* __restrict__ in, const u32* __restrict__ in_count, u32 in_cap, const uint16_t* __restrict__ tags, u64 n_tags,
                                                     sections_set ss, u32 limit, int by_score, fzb_match_rec* __restrict__ out, u32* __restrict__ counts,
                                                     const u32* __restrict__ scratch, u32 ntiles_cap) {
    __shared__ u32 wave_gt[SECTIONS_MAX][4], wave_eq[SECTIONS_MAX][4];
    __shared__ TopkCut cuts[SECTIONS_MAX];
    __shared__ u32 kept[SECTIONS_MAX];
    const u32 S = min(ss.n, (u32)SECTIONS_MAX);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((u32)tid < S) {
        const sections_state st = sec_state(scratch)[tid];
        cuts[tid] = st.cut;
        kept[tid] = min(st.kept, limit);
        if (blockIdx.x == 0) {
            counts[2 * tid] = min(st.kept, limit);
            counts[2 * tid + 1] = st.n;
        }
    }
    __syncthreads();
    const u32 n = sec_count(in_count, in_cap);
    const u32 ntiles = min((n + SECTIONS_TILE - 1) / SECTIONS_TILE, ntiles_cap);
    const u64 below = ((u64)1 << lane) - 1;
    for (u32 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        u32 run_gt[SECTIONS_MAX], run_eq[SECTIONS_MAX];  // the section's records in front of the slab: uniform over the workgroup
#pragma unroll
        for (int s = 0; s < SECTIONS_MAX; s++) {
            run_gt[s] = (u32)s < S ? sec_row(scratch, ntiles_cap, 2, s)[tile] : 0u;
            run_eq[s] = (u32)s < S ? sec_row(scratch, ntiles_cap, 3, s)[tile] : 0u;
        }
        const u32 lo = tile * SECTIONS_TILE, hi = min(lo + SECTIONS_TILE, n);
        for (u32 base = lo; base < hi; base += 256) {
            const u32 i = base + tid;
            const bool valid = i < hi;
            fzb_match_rec r;
            r.index = 0; r.score = 0; r.exact = 0; r.valid = 0;
            if (valid) r = in[i];
            const u32 cls = sec_classes(ss, cuts, by_score, valid, valid ? scope_tag_of(tags, n_tags, 0, 0, r.index) : 0u, r.score);
            u32 my_gt[SECTIONS_MAX], my_eq[SECTIONS_MAX];
#pragma unroll
            for (int s = 0; s < SECTIONS_MAX; s++) {
                my_gt[s] = my_eq[s] = 0;
                if ((u32)s < S) {
                    const u64 bg = __ballot(((cls >> (2 * s)) & 3u) == 1u);
                    const u64 be = __ballot(((cls >> (2 * s)) & 3u) == 2u);
                    if (lane == 0) {
                        wave_gt[s][wave] = __popcll(bg);
                        wave_eq[s][wave] = __popcll(be);
                    }
                    my_gt[s] = __popcll(bg & below);
                    my_eq[s] = __popcll(be & below);
                }
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < SECTIONS_MAX; s++) {
                if ((u32)s < S) {
                    u32 gt_before = run_gt[s] + my_gt[s], eq_before = run_eq[s] + my_eq[s];
                    u32 all_gt = 0, all_eq = 0;
#pragma unroll
                    for (int w = 0; w < 4; w++) {
                        if (w < wave) {
                            gt_before += wave_gt[s][w];
                            eq_before += wave_eq[s][w];
                        }
                        all_gt += wave_gt[s][w];
                        all_eq += wave_eq[s][w];
                    }
                    if ((cls >> (2 * s)) & 3u) {
                        const u32 d = topk_dest(cuts[s], by_score, r.score, gt_before, eq_before);
                        if (d != TOPK_NOT_KEPT && d < kept[s]) out[(size_t)s * limit + d] = r;  // (kept_s <= limit: inside the section's slab)
                    }
                    run_gt[s] += all_gt;
                    run_eq[s] += all_eq;
                }
            }
            __syncthreads();  // (the wave counts are written again in the next round)
        }
    }
}

// the order of each section's head: the slab's kept records (record order) -> LDS -> their ranks (sections_rank) -> the slab
__global__ __launch_bounds__(256) void k_sec_order(fzb_match_rec* __restrict__ out, u32 n_sections, u32 limit, int by_score, int desc, const u32* __restrict__ scratch) {
    __shared__ sections_rec slab[SECTIONS_LIMIT_MAX];
    for (u32 s = blockIdx.x; s < n_sections; s += gridDim.x) {
        const u32 kept = min(min(sec_state(scratch)[s].kept, limit), (u32)SECTIONS_LIMIT_MAX);
        sections_rec* const dst = (sections_rec*)out + (size_t)s * limit;
        for (u32 i = threadIdx.x; i < kept; i += 256) slab[i] = dst[i];
        __syncthreads();
        for (u32 i = threadIdx.x; i < kept; i += 256) dst[sections_rank(slab, kept, i, by_score, desc)] = slab[i];
        __syncthreads();
    }
}

// Sectioned top-`limit` with matched positions: the stage's slabs -> ONE dense head and the item list of the traced pass, where k_top_items
// (kernels_indices.hip) takes a head that is dense already.  Every workgroup re-derives the exclusive prefix of the S <= 8 kept counts
// (sections_head_base) from the stage's count words: no extra launch, no workgroup waits for another one.  Slot k of the slabs goes to
// head[base_s + j] and items[base_s + j]; workgroup 0 writes the item count, the head's pair (records in all, twice: the pack copies the
// second word into the word the contract leaves unspecified), the caller's 2S count words, and clears the two words the pack only raises.
__global__ __launch_bounds__(256) void k_sec_items(const fzb_match_rec* __restrict__ slabs, const u32* __restrict__ counts, u32 n_sections, u32 limit, u32 cap,
                                                   fzb_match_rec* __restrict__ head, u32* __restrict__ head_count, u32* __restrict__ items, u32* __restrict__ n_items,
                                                   u32* __restrict__ dev_counts) {
    __shared__ u32 s_counts[2 * SECTIONS_MAX], s_base[SECTIONS_MAX + 1];
    const u32 S = min(n_sections, (u32)SECTIONS_MAX);
    if (threadIdx.x < 2 * S) s_counts[threadIdx.x] = counts[threadIdx.x];
    __syncthreads();
    if (threadIdx.x <= S) s_base[threadIdx.x] = sections_head_base(s_counts, threadIdx.x, limit);
    __syncthreads();
    const u32 slots = S * limit;
    for (u32 k = blockIdx.x * 256u + threadIdx.x; k < slots; k += gridDim.x * 256u) {
        const u32 d = sections_head_dest(s_counts, s_base, limit, k);
        if (d != SECTIONS_NO_SLOT && d < cap) {  // (the sum of the kept counts is at most S * min(limit, haystacks) = cap)
            const fzb_match_rec r = slabs[k];
            head[d] = r;
            items[d] = r.index;
        }
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < 2 * S) dev_counts[threadIdx.x] = (threadIdx.x & 1u) ? s_counts[threadIdx.x] : sections_slab_kept(s_counts, threadIdx.x >> 1, limit);
        if (threadIdx.x == 0) {
            const u32 total = min(s_base[S], cap);
            n_items[0] = total;
            head_count[0] = total;
            head_count[1] = total;
            dev_counts[2 * S + 2] = 0;
            dev_counts[2 * S + 3] = 0;
        }
    }
}

// slabs / counts: what fzb_launch_sections_select wrote (n_sections slabs of `limit` records, 2 n_sections words).  head / items: room for cap >=
// n_sections * min(limit, haystacks) entries; head_count: two words; n_items: one; dev_counts: 2 n_sections + 4 words, of which [2S] and
// [2S + 1] are left to the pack (fzb_launch_indices_pack with dev_count = dev_counts + 2S).
void fzb_launch_sections_items(const fzb_match_rec* slabs, const u32* counts, u32 n_sections, u32 limit, u32 cap, fzb_match_rec* head, u32* head_count, u32* items, u32* n_items,
                               u32* dev_counts, int grid, hipStream_t st) {
    const int g = (int)std::max<u32>(1, std::min<u32>((u32)grid, (n_sections * limit + 255) / 256));
    FZB_LAUNCH(k_sec_items, dim3(g), dim3(256), 0, st, slabs, counts, n_sections, limit, cap, head, head_count, items, n_items, dev_counts);
}

// in: *in_count records (at most in_cap) in record order, numbered from 0 over the corpus whose tag column is `tags` (n_tags entries; null /
// 0: every tag 0).  out: n_sections slabs of `limit` records (limit <= SECTIONS_LIMIT_MAX), slab s = the ordered head of section s;
// counts[2s] = its records, counts[2s + 1] = the section's matches.  scratch: fzb_sections_scratch_words(in_cap) words; ntiles_cap =
// in_cap / SECTIONS_TILE + 2.  in and out must not overlap.  Returns the first error of the fill or the launches.
hipError_t fzb_launch_sections_select(const fzb_match_rec* in, const u32* in_count, u32 in_cap, const uint16_t* tags, u64 n_tags, const sections_set& ss, u32 limit, int by_score,
                                      int desc, int one_pass, fzb_match_rec* out, u32* counts, u32* scratch, u32 ntiles_cap, int grid, hipStream_t st) {
    const u32 S = ss.n;
    if (S == 0) return hipSuccess;
    if (!tags) n_tags = 0;
    const hipError_t e = hipMemsetAsync(scratch, 0, SEC_TILES * sizeof(u32), st);
    if (e != hipSuccess) return e;  // (nothing launched: the bins would hold the previous query's counts)
    const int small = tc_grid(S, grid), rows = tc_grid(2 * S, grid);
    if (by_score) {
        FZB_LAUNCH(k_sec_hist, dim3(grid), dim3(256), 0, st, in, in_count, in_cap, tags, n_tags, ss, limit, 0, one_pass, scratch);
        if (!one_pass) {
            FZB_LAUNCH(k_sec_cut, dim3(small), dim3(256), 0, st, S, limit, 0, one_pass, desc, scratch);
            FZB_LAUNCH(k_sec_hist, dim3(grid), dim3(256), 0, st, in, in_count, in_cap, tags, n_tags, ss, limit, 1, one_pass, scratch);
        }
        FZB_LAUNCH(k_sec_cut, dim3(small), dim3(256), 0, st, S, limit, 1, one_pass, desc, scratch);
    }
    FZB_LAUNCH(k_sec_tile_counts, dim3(grid), dim3(256), 0, st, in, in_count, in_cap, tags, n_tags, ss, by_score, scratch, ntiles_cap);
    FZB_LAUNCH(k_sec_scan, dim3(rows), dim3(64), 0, st, in_count, in_cap, S, scratch, ntiles_cap);
    if (!by_score) FZB_LAUNCH(k_sec_cut, dim3(small), dim3(256), 0, st, S, limit, 2, one_pass, desc, scratch);
    FZB_LAUNCH(k_sec_scatter, dim3(grid), dim3(256), 0, st, in, in_count, in_cap, tags, n_tags, ss, limit, by_score, out, counts, scratch, ntiles_cap);
    if (limit != 0 && (by_score || desc)) FZB_LAUNCH(k_sec_order, dim3(small), dim3(256), 0, st, out, S, limit, by_score, desc, scratch);
    return hipGetLastError();
}
