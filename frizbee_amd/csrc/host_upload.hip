// fzb_corpus_upload: what `match_list(&haystacks)` borrows (src/matcher/mod.rs:212), brought into HBM at link speed.
//
// The caller's two arrays (all haystack bytes back to back + exclusive end offsets) travel AS THEY ARE, one hipMemcpy each: the runtime
// pins the pageable source on the fly and the DMA engines run at 52-53 GB/s (measured on the MI355X box, tools/bench_upload.py:
// 10 M x 32 B = 400 MB of bytes + offsets in 7.6 ms, a 12.5 M-item ragged shard = 950 MB in 18 ms).  Round 2 repacked the list on the
// host first (82 ms for the same 10 M list - the repack, not the copy, was the cost).  Two alternatives are kept behind
// FZB_UPLOAD_MODE for comparison: "register" (hipHostRegister + copy: the same 7.6 ms) and "staged" (worker threads copying through
// their own page-locked staging buffers into asynchronous copies: 20 ms, bound by the host memcpy).  The library's device layout
// ("padded-16": every haystack on a 16-byte boundary, zero
// gaps, end offsets inside that layout) is then built ON the device:
//   k_up_tiles    per 1024 haystacks: sum of the padded lengths, min / max length, "offsets decrease" flag
//   k_up_scan     exclusive scan of the tile sums (one workgroup)
//   k_up_build    per tile: the haystacks' padded starts (scan in LDS), the end offsets in the padded layout, and the bytes - one
//                 thread per 16-byte OUTPUT vector (binary search of its haystack in the tile's starts), so writes are whole aligned
//                 vectors and reads run along each haystack
// A list whose lengths are all multiples of 16 (the 32-byte bench lists) already IS the padded layout: the uploaded buffer is kept and
// only the offsets are rewritten.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "host_internal.h"
#include "kernels_common.h"
#include "sig_filter.h"
#include "score_bias.h"

namespace {

constexpr int UP_TILE = 1024;
constexpr int UP_THREADS = 256;

// stats block (device): [0] total padded bytes (u64) [1] min len [2] max len (u64 each) [3] bad flag [4] haystacks beyond 256 bytes
// [5] the longest haystack within 256 bytes ([4], [5]: what decides whether the list calls for a filter view)
struct UpStats {
    u64 total_padded, min_len, max_len, bad, n_long, max_short;
};

__global__ __launch_bounds__(UP_THREADS) void k_up_tiles(const u64* __restrict__ ends, u64 n, u64 ends_base, u64* __restrict__ tile_sums, UpStats* __restrict__ stats) {
    __shared__ u64 s_sum[UP_THREADS / 64];
    __shared__ u64 s_min[UP_THREADS / 64];
    __shared__ u64 s_max[UP_THREADS / 64];
    __shared__ u64 s_short[UP_THREADS / 64];
    __shared__ u32 s_nlong[UP_THREADS / 64];
    const u64 tile = blockIdx.x;
    u64 sum = 0, mn = ~(u64)0, mx = 0, ms = 0;
    u32 nl = 0;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < UP_TILE / UP_THREADS; k++) {
        const u64 i = tile * UP_TILE + (u64)k * UP_THREADS + threadIdx.x;
        if (i < n) {
            const u64 e = ends[i], p = i ? ends[i - 1] : ends_base;
            if (e < p) bad = true;
            const u64 len = e >= p ? e - p : 0;
            sum += (len + 15) & ~(u64)15;
            mn = min(mn, len);
            mx = max(mx, len);
            if (len > 256) nl++;
            else ms = max(ms, len);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off);
        mn = min(mn, (u64)__shfl_xor(mn, off));
        mx = max(mx, (u64)__shfl_xor(mx, off));
        ms = max(ms, (u64)__shfl_xor(ms, off));
        nl += __shfl_xor(nl, off);
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr((unsigned long long*)&stats->bad, 1ull);
    if ((threadIdx.x & 63) == 0) {
        s_sum[threadIdx.x >> 6] = sum;
        s_min[threadIdx.x >> 6] = mn;
        s_max[threadIdx.x >> 6] = mx;
        s_short[threadIdx.x >> 6] = ms;
        s_nlong[threadIdx.x >> 6] = nl;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = 0, a = ~(u64)0, b = 0, sh = 0, l = 0;
        for (int w = 0; w < UP_THREADS / 64; w++) {
            t += s_sum[w];
            a = min(a, s_min[w]);
            b = max(b, s_max[w]);
            sh = max(sh, s_short[w]);
            l += s_nlong[w];
        }
        tile_sums[tile] = t;
        atomicMin((unsigned long long*)&stats->min_len, (unsigned long long)a);
        atomicMax((unsigned long long*)&stats->max_len, (unsigned long long)b);
        atomicMax((unsigned long long*)&stats->max_short, (unsigned long long)sh);
        if (l) atomicAdd((unsigned long long*)&stats->n_long, (unsigned long long)l);
    }
}

// The same four figures (min / max length, haystacks beyond 256 bytes, longest within 256) of the first n haystacks of a RESIDENT list,
// read from its padded-layout offsets: what fzb_corpus_truncate re-measures for the kept prefix, and what a borrowed corpus' view goes by.
template <typename ET>
__global__ __launch_bounds__(UP_THREADS) void k_up_measure(const ET* __restrict__ ends, u64 n, UpStats* __restrict__ stats) {
    u64 mn = ~(u64)0, mx = 0, ms = 0;
    u32 nl = 0;
    const u64 stride = (u64)gridDim.x * UP_THREADS;
    for (u64 i = (u64)blockIdx.x * UP_THREADS + threadIdx.x; i < n; i += stride) {
        const u64 st = i ? ((u64)ends[i - 1] + 15) & ~(u64)15 : 0;
        const u64 e = (u64)ends[i], len = e >= st ? e - st : 0;
        mn = min(mn, len);
        mx = max(mx, len);
        if (len > 256) nl++;
        else ms = max(ms, len);
    }
    for (int off = 32; off > 0; off >>= 1) {
        mn = min(mn, (u64)__shfl_xor(mn, off));
        mx = max(mx, (u64)__shfl_xor(mx, off));
        ms = max(ms, (u64)__shfl_xor(ms, off));
        nl += __shfl_xor(nl, off);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin((unsigned long long*)&stats->min_len, (unsigned long long)mn);
        atomicMax((unsigned long long*)&stats->max_len, (unsigned long long)mx);
        atomicMax((unsigned long long*)&stats->max_short, (unsigned long long)ms);
        if (nl) atomicAdd((unsigned long long*)&stats->n_long, (unsigned long long)nl);
    }
}

// exclusive scan of the tile sums in place (one workgroup of 1024 threads, chunks of 1024 tiles with a running carry)
__global__ __launch_bounds__(1024) void k_up_scan(u64* __restrict__ tile_sums, u64 ntiles, UpStats* __restrict__ stats) {
    __shared__ u64 s_wave[16];
    __shared__ u64 s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (u64 base = 0; base < ntiles; base += 1024) {
        const u64 i = base + threadIdx.x;
        const u64 v = i < ntiles ? tile_sums[i] : 0;
        u64 incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const u64 t = __shfl_up(incl, off);
            if ((int)(threadIdx.x & 63) >= off) incl += t;
        }
        if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
        __syncthreads();
        u64 wave_base = 0;
        for (u32 w = 0; w < (threadIdx.x >> 6); w++) wave_base += s_wave[w];
        const u64 carry = s_carry;
        if (i < ntiles) tile_sums[i] = carry + wave_base + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = carry + wave_base + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) stats->total_padded = s_carry;
}

// ET = u32 / u64 end offsets of the padded layout.  COPY = false: the raw buffer already is the padded layout (only offsets are written).
// The batch is laid out BEHIND what is resident: its first haystack starts at byte `out_base` (a multiple of 16) of `padded` and is
// haystack `index_base` of `ends_out` (0, 0 for a whole list).
template <typename ET, bool COPY>
__global__ __launch_bounds__(UP_THREADS) void k_up_build(const u8* __restrict__ raw, const u64* __restrict__ ends, u64 n, u64 ends_base, const u64* __restrict__ tile_base,
                                                         u8* __restrict__ padded, ET* __restrict__ ends_out, u64 out_base, u64 index_base) {
    __shared__ u64 s_pstart[UP_TILE + 1];  // padded start of each haystack of the tile, relative to the tile's base
    __shared__ u64 s_wave[UP_THREADS / 64];
    const u64 tile = blockIdx.x;
    const u64 i0 = tile * UP_TILE;
    const u64 base = tile_base[tile] + out_base;
    // every thread owns 4 CONSECUTIVE haystacks: serial prefix of their padded lengths, then a scan over the threads
    const u64 first = i0 + (u64)threadIdx.x * 4;
    const u64 e_prev = first == 0 ? ends_base : (first <= n ? ends[first - 1] : 0);
    u64 plen[4], e[4], mine = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u64 i = first + k;
        const u64 p = k ? e[k - 1] : e_prev;
        e[k] = i < n ? ends[i] : p;
        plen[k] = ((e[k] - p) + 15) & ~(u64)15;
        mine += plen[k];
    }
    u64 incl = mine;
    for (int off = 1; off < 64; off <<= 1) {
        const u64 t = __shfl_up(incl, off);
        if ((int)(threadIdx.x & 63) >= off) incl += t;
    }
    if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    u64 run = incl - mine;
    for (u32 w = 0; w < (threadIdx.x >> 6); w++) run += s_wave[w];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u64 i = first + k;
        s_pstart[threadIdx.x * 4 + k] = run;
        if (i < n) ends_out[index_base + i] = (ET)(base + run + (e[k] - (k ? e[k - 1] : e_prev)));
        run += plen[k];
    }
    if (threadIdx.x == UP_THREADS - 1) s_pstart[UP_TILE] = run;
    __syncthreads();
    if (!COPY) return;
    const u64 tile_bytes = s_pstart[UP_TILE];
    const u32 cnt = (u32)min((u64)UP_TILE, n - i0);
    for (u64 v = (u64)threadIdx.x * 16u; v < tile_bytes; v += UP_THREADS * 16u) {
        // the haystack this output vector belongs to: last j with pstart[j] <= v (empty haystacks share a start with their successor:
        // the search lands on the last of them, the one that owns the bytes)
        u32 lo = 0, hi = cnt;
        while (hi - lo > 1) {
            const u32 mid = (lo + hi) >> 1;
            if (s_pstart[mid] <= v) lo = mid;
            else hi = mid;
        }
        const u64 i = i0 + lo;
        const u64 src_lo = i ? ends[i - 1] : ends_base, src_hi = ends[i];
        const u64 off = v - s_pstart[lo];
        const u64 len = src_hi - src_lo;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (off < len) {
            const u64 p = src_lo - ends_base + off;  // byte position in `raw`
            const u32 rem = (u32)min((u64)16, len - off);
            const u32* a = (const u32*)(raw + (p & ~(u64)3));
            const u32 sh = (u32)(p & 3);
            // 16 bytes from an arbitrary byte position: five aligned dwords, funnel-shifted (the raw buffer has >= 96 readable bytes of slack)
            const u32 w0 = a[0], w1 = a[1], w2 = a[2], w3 = a[3], w4 = sh ? a[4] : 0u;
            u32 x[4] = {__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh), __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh)};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const u32 lo_b = 4u * k;
                if (rem <= lo_b) x[k] = 0;
                else if (rem - lo_b < 4) x[k] &= (1u << (8 * (rem - lo_b))) - 1;
            }
            q = make_uint4(x[0], x[1], x[2], x[3]);
        }
        *(uint4*)(padded + base + v) = q;
    }
}

// The streaming filter's VIEW of a ragged list (CorpusDev::vbytes; layout described there): two passes over the canonical layout, one
// workgroup per 1024-haystack tile.
//   k_up_view_sort   ranks the tile's haystacks by descending vector count (counting sort, LDS atomics - upload time), writes vperm / vlen,
//                    the vectors-per-member of each of its 16 groups, and the tile's size in the view (in 16-byte units)
//   (k_up_scan: exclusive scan of the tile sizes - the same kernel the canonical layout uses)
//   k_up_view_fill   writes the groups' block offsets and copies every vector to its interleaved position (the buffer was cleared: the
//                    zero vectors behind a group's shorter members are already there)
// Both take the FIRST TILE they work on (workgroup b = tile first_tile + b): an append re-sorts and re-fills only the tiles from the last,
// partial one on (view_sync below); the fill then places tile first_tile at `unit_base`, the offset that tile already had.
//   k_up_vlong_prune drops the outliers of the tiles about to be re-sorted from the list (they re-enter it from the sort), in place
#define FV_CLASSES 258  // sort key = the haystack's LENGTH, 0..256 bytes (round 5; rounds 3-4: its vector count, 18 classes), and a guard class
// Round 5: a group's LAST vector row is stored as narrow as its longest member's tail allows - 4, 8, 12 or 16 bytes per member instead of 16
// (vgnv[group] = vectors per member | (tail bytes / 4 - 1) << 5) - and the tile is sorted by exact length, so that the 64 members of a group end
// within a few bytes of each other: the view of the C4 shard shrinks from 1.19 to 1.12 x the haystack bytes (padded-16 alone costs 1.106).
template <typename ET>
__global__ __launch_bounds__(UP_THREADS) void k_up_view_sort(const ET* __restrict__ ends, u64 n, u16* __restrict__ vperm, u16* __restrict__ vlen, u8* __restrict__ vgnv,
                                                             u64* __restrict__ tile_units, UpStats* __restrict__ stats, u32* __restrict__ vlong, u32 long_cap, u32 first_tile) {
    __shared__ u32 s_len[UP_TILE];
    __shared__ u16 s_inv[UP_TILE];
    __shared__ u32 s_hist[FV_CLASSES], s_base[FV_CLASSES];
    __shared__ u32 s_gunits[UP_TILE / 64];
    const u64 i0 = ((u64)blockIdx.x + first_tile) * UP_TILE;
    const u32 nt = (u32)min((u64)UP_TILE, n - i0);
    const int tid = threadIdx.x;
    for (int c = tid; c < FV_CLASSES; c += UP_THREADS) s_hist[c] = 0;
    __syncthreads();
    u32 cls[4], rk[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u32 j = tid + UP_THREADS * k;
        cls[k] = rk[k] = 0;
        if (j < nt) {
            const ET st = (i0 + j) ? (ends[i0 + j - 1] + (ET)15) & ~(ET)15 : (ET)0;
            u32 len = (u32)min((u64)(ends[i0 + j] - st), (u64)0xFFFFu);
            if (len > 256u) {  // an OUTLIER: not in the view (no vectors, sorted last, vlen = 0xFFFF) - listed for the filter's follow-up launch
                const u32 slot = (u32)atomicAdd((unsigned long long*)&stats->bad, 1ull);  // (bad = the outlier count here)
                if (slot < long_cap) vlong[slot] = (u32)(i0 + j);
                len = 0xFFFFu;
            }
            s_len[j] = len;
            cls[k] = len == 0xFFFFu ? 0u : min(len, (u32)FV_CLASSES - 1);
            rk[k] = atomicAdd(&s_hist[cls[k]], 1u);
        }
    }
    __syncthreads();
    if (tid == 0) {  // descending: the longest haystacks first
        u32 run = 0, top = 0, low = FV_CLASSES;
        for (int c = FV_CLASSES - 1; c >= 0; c--) {
            s_base[c] = run;
            run += s_hist[c];
            if (s_hist[c]) { top = max(top, (u32)c); low = min(low, (u32)c); }
        }
        atomicMax((unsigned long long*)&stats->max_len, (unsigned long long)((top + 15u) >> 4));  // in VECTORS: the view's widest / narrowest member
        atomicMin((unsigned long long*)&stats->min_len, (unsigned long long)((low + 15u) >> 4));
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u32 j = tid + UP_THREADS * k;
        if (j < nt) s_inv[s_base[cls[k]] + rk[k]] = (u16)j;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u32 p = tid + UP_THREADS * k;  // sorted position
        if (p < nt) {
            const u32 j = s_inv[p];
            vperm[i0 + p] = (u16)j;
            vlen[i0 + p] = (u16)s_len[j];
        }
    }
    if (tid < UP_TILE / 64) {  // the tile's 16 groups: vectors per member and tail width = the group's first (longest) member's
        const u32 p0 = tid * 64;
        const u32 l0 = p0 < nt ? s_len[s_inv[p0]] : 0u;
        const u32 len0 = l0 == 0xFFFFu ? 0u : l0;
        const u32 nv = (len0 + 15u) >> 4;
        const u32 tw = nv ? ((len0 - 16u * (nv - 1) + 3u) & ~3u) : 0u;  // 4, 8, 12 or 16 bytes of the last vector are stored per member
        vgnv[i0 / 64 + tid] = (u8)(nv ? (nv | ((tw / 4 - 1) << 5)) : 0u);
        s_gunits[tid] = nv ? (nv - 1) * 64 + tw * 4 : 0u;  // 16-byte units of the group's block: nv - 1 rows of 1 KiB + 64 tails of tw bytes
    }
    __syncthreads();
    if (tid == 0) {
        u64 t = 0;
        for (int g = 0; g < UP_TILE / 64; g++) t += s_gunits[g];
        tile_units[blockIdx.x] = t;
    }
}

template <typename ET>
__global__ __launch_bounds__(UP_THREADS) void k_up_view_fill(const u8* __restrict__ bytes, const ET* __restrict__ ends, u64 n, const u16* __restrict__ vperm,
                                                             const u8* __restrict__ vgnv, const u64* __restrict__ tile_base_units, u8* __restrict__ vbytes, u32* __restrict__ vgofs,
                                                             u32 first_tile, u64 unit_base) {
    __shared__ u32 s_gofs[UP_TILE / 64], s_gnv[UP_TILE / 64], s_gtw[UP_TILE / 64];
    const u64 i0 = ((u64)blockIdx.x + first_tile) * UP_TILE;
    const u32 nt = (u32)min((u64)UP_TILE, n - i0);
    const int tid = threadIdx.x;
    if (tid == 0) {
        u64 run = tile_base_units[blockIdx.x] + unit_base;
        for (int g = 0; g < UP_TILE / 64; g++) {
            const u32 code = vgnv[i0 / 64 + g], nv = code & 31u, tw = nv ? ((code >> 5) + 1u) * 4u : 0u;
            s_gofs[g] = (u32)run;
            s_gnv[g] = nv;
            s_gtw[g] = tw;
            vgofs[i0 / 64 + g] = (u32)run;
            run += nv ? (u64)(nv - 1) * 64 + (u64)tw * 4 : 0;
        }
    }
    __syncthreads();
    // four threads per sorted haystack, each copying every fourth vector; the group's last row holds `tw` bytes per member
    for (u32 p = tid >> 2; p < nt; p += UP_THREADS / 4) {
        const u64 j = i0 + vperm[i0 + p];
        const ET st = j ? (ends[j - 1] + (ET)15) & ~(ET)15 : (ET)0;
        if (ends[j] - st > (ET)256) continue;  // an outlier has no vectors in the view
        const u32 nv = (u32)((ends[j] - st + (ET)15) >> 4);
        const u32 gnv = s_gnv[p >> 6], gtw = s_gtw[p >> 6];
        const uint4* src = (const uint4*)(bytes + st);
        u8* gblock = vbytes + (size_t)s_gofs[p >> 6] * 16;
        for (u32 v = tid & 3; v < nv; v += 4) {
            const uint4 q = src[v];
            if (v + 1 < gnv) {
                *(uint4*)(gblock + (size_t)v * 1024 + (size_t)(p & 63) * 16) = q;
            } else {  // (a member as long in vectors as its group's longest: its last vector goes to the narrow row; bytes beyond `gtw` are zero)
                u32* dst = (u32*)(gblock + (size_t)(gnv - 1) * 1024 + (size_t)(p & 63) * gtw);
                dst[0] = q.x;
                if (gtw > 4) dst[1] = q.y;
                if (gtw > 8) dst[2] = q.z;
                if (gtw > 12) dst[3] = q.w;
            }
        }
    }
}

// keeps the outliers below haystack `limit`, in their order, and leaves their number in stats->bad (where k_up_view_sort goes on counting):
// one workgroup, chunks of 1024 entries with a running carry - an entry is written at or before the place it was read from
__global__ __launch_bounds__(1024) void k_up_vlong_prune(u32* __restrict__ vlong, u32 n_long, u32 limit, UpStats* __restrict__ stats) {
    __shared__ u32 s_wave[16];
    __shared__ u32 s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (u32 base = 0; base < n_long; base += 1024) {
        const u32 i = base + threadIdx.x;
        const u32 v = i < n_long ? vlong[i] : 0u;
        const bool keep = i < n_long && v < limit;
        const u64 m = __ballot(keep);
        const u32 rank = (u32)__popcll(m & (((u64)1 << (threadIdx.x & 63)) - 1));
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = (u32)__popcll(m);
        __syncthreads();  // (every entry of the chunk has been read)
        u32 wave_base = 0, total = 0;
        for (u32 w = 0; w < 16; w++) {
            if (w < (threadIdx.x >> 6)) wave_base += s_wave[w];
            total += s_wave[w];
        }
        const u32 carry = s_carry;
        if (keep) vlong[carry + wave_base + rank] = v;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = carry + total;
        __syncthreads();
    }
    if (threadIdx.x == 0) stats->bad = s_carry;
}

// ---- host -> device at link speed ---------------------------------------------------------------------------------------------
// One hipMemcpy per array straight from the caller's pageable memory: 52-53 GB/s measured (profiles/r03_upload_modes.txt; hipHostRegister
// first and a pool of threads with pinned staging buffers were both slower there and left with round 6's prune).
struct H2DJob {
    void* dst;
    const void* src;
    size_t bytes;
};

// copies every job; returns hipSuccess or the first error
hipError_t h2d_all(const std::vector<H2DJob>& jobs, int device) {
    (void)device;
    for (const H2DJob& j : jobs)
        if (j.bytes) {
            hipError_t e = hipMemcpy(j.dst, j.src, j.bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

const UpStats UP_STATS_INIT{0, ~(u64)0, 0, 0, 0, 0};
inline u64 up_tiles(u64 n) { return (n + UP_TILE - 1) / UP_TILE; }
// outliers (haystacks beyond 256 bytes) the view of n haystacks tolerates: one in 256, at least 64 - more, and the list is not a short-haystack list
inline u64 long_cap_of(u64 n) { return std::min<u64>(n / 256 + 64, 0x7FFFFFFFu); }

// ---- "lay out a batch behind position p": the two halves of the layout pass, for a whole list (upload) and for an appended batch ----
// The batch is resident as it arrived: d_ends64[i] = exclusive end of its haystack i counted from `ends_base`.
// First half: per-tile sums of the padded lengths, their exclusive scan (d_tiles), and the batch's stats - padded size, min / max length,
// "offsets decrease" flag, outlier figures - read back: the one synchronisation, before anything of the corpus is written.
hipError_t batch_measure(const u64* d_ends64, u64 n, u64 ends_base, u64* d_tiles, UpStats* d_stats, UpStats* st) {
    hipError_t e = hipMemcpy(d_stats, &UP_STATS_INIT, sizeof(UpStats), hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    FZB_LAUNCH(k_up_tiles, dim3((unsigned)up_tiles(n)), dim3(UP_THREADS), 0, nullptr, d_ends64, n, ends_base, d_tiles, d_stats);
    FZB_LAUNCH(k_up_scan, dim3(1), dim3(1024), 0, nullptr, d_tiles, up_tiles(n), d_stats);
    return hipMemcpy(st, d_stats, sizeof(UpStats), hipMemcpyDeviceToHost);
}
// Second half: the batch's bytes from byte `out_base` of `out_bytes` on (copy = false: they are there already, `raw` is the padded layout)
// and its end offsets from entry `index_base` of `out_ends` on, in the padded layout's terms.
void batch_lay_out(const u8* d_raw, const u64* d_ends64, u64 n, u64 ends_base, const u64* d_tiles, u8* out_bytes, u64 out_base, void* out_ends, u64 index_base, bool ends_u64,
                   bool copy) {
#define FZB_UP_BUILD(ET, COPY) \
    FZB_LAUNCH((k_up_build<ET, COPY>), dim3((unsigned)up_tiles(n)), dim3(UP_THREADS), 0, nullptr, d_raw, d_ends64, n, ends_base, d_tiles, out_bytes, (ET*)out_ends, out_base, index_base)
    if (ends_u64) { if (copy) FZB_UP_BUILD(u64, true); else FZB_UP_BUILD(u64, false); }
    else { if (copy) FZB_UP_BUILD(u32, true); else FZB_UP_BUILD(u32, false); }
#undef FZB_UP_BUILD
}

// the host's figures of a list -> what the kernels go by (as a fresh upload sets them)
void set_measured(fzb_corpus* c) {
    const u64 n = c->dev.n;
    if (!n) { c->min_len = ~(u64)0; c->max_len = 0; c->n_over256 = 0; c->max_short = 0; }
    c->dev.max_len = (u32)std::min<u64>(c->max_len, 0xFFFFFFFFu);
    c->dev.uniform_len = (n && c->min_len == c->max_len && c->max_len && c->max_len < 0xFFFFFFFFu) ? (u32)c->max_len : 0u;  // kernels then skip the end offsets
}

// the tile sums / tile units scratch and the stats block of the layout and view passes, kept with the corpus
hipError_t ensure_tiles_scratch(fzb_corpus* c, u64 tiles) {
    if (!c->stage_stats) {
        hipError_t e = fzb_dev_alloc(&c->stage_stats, sizeof(UpStats));
        if (e != hipSuccess) return e;
    }
    if (c->stage_tiles && c->stage_tiles_cap >= tiles) return hipSuccess;
    void* p = nullptr;
    hipError_t e = fzb_dev_alloc(&p, std::max<u64>(tiles, 1) * 8);
    if (e != hipSuccess) return e;
    if (c->stage_tiles) (void)hipFree(c->stage_tiles);
    c->stage_tiles = p;
    c->stage_tiles_cap = std::max<u64>(tiles, 1);
    return hipSuccess;
}

// ---- the filter's view, kept in step with the list -------------------------------------------------------------------------------
// A view of n haystacks never takes more than their padded bytes + 16 KiB per tile: a group's block is 64 x its longest member (rounded
// to 4 bytes), which every member of the group before it - the tile is sorted - is at least as long as; the tile's first group has
// nobody before it: 64 x 256 bytes.
inline u64 view_units_bound(u64 items, u64 padded_bytes) { return padded_bytes / 16 + up_tiles(items) * 1024; }

void view_free(fzb_corpus* c) {
    for (int q = 0; q < 6; q++) {
        if (c->own_view[q]) (void)hipFree(c->own_view[q]);
        c->own_view[q] = nullptr;
    }
    c->view_cap_items = c->view_cap_units = 0;
    (void)hipGetLastError();
}
// the corpus goes on without a view; its buffers stay for the list that calls for one again (their used part cleared)
hipError_t view_deactivate(fzb_corpus* c) {
    hipError_t e = hipSuccess;
    if (c->dev.vbytes && c->own_view[0] && c->view_units) e = hipMemsetAsync(c->own_view[0], 0, c->view_units * 16, nullptr);
    c->dev.vbytes = nullptr; c->dev.vgofs = nullptr; c->dev.vgnv = nullptr; c->dev.vlen = nullptr; c->dev.vperm = nullptr; c->dev.vlong = nullptr;
    c->dev.view_nv = 0;
    c->dev.n_long = 0;
    c->view_units = c->view_items = 0;
    return e;
}
// Room for the per-haystack arrays of `items` haystacks (own_view[1..5]) and for `units` 16-byte units of view bytes (own_view[0], its
// 1 KiB of slack behind them; 0 = leave them as they are); what is in use of a live view (`keep_items` haystacks, `keep_units` units) moves device to device.
// hipErrorOutOfMemory: nothing has changed.
hipError_t view_ensure_room(fzb_corpus* c, u64 items, u64 units, u64 keep_items, u64 keep_units) {
    const bool live = c->dev.vbytes != nullptr;
    if (c->view_cap_items < items || !c->own_view[1]) {
        const u64 groups = up_tiles(items) * (UP_TILE / 64), keep_groups = up_tiles(keep_items) * (UP_TILE / 64);
        const size_t sizes[6] = {0, (size_t)groups * 4, (size_t)groups, (size_t)items * 2, (size_t)items * 2, (size_t)long_cap_of(items) * 4};
        const size_t keep[6] = {0, (size_t)keep_groups * 4, (size_t)keep_groups, (size_t)keep_items * 2, (size_t)keep_items * 2, (size_t)c->dev.n_long * 4};
        void* fresh[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        hipError_t e = hipSuccess;
        for (int q = 1; q < 6 && e == hipSuccess; q++) {
            e = fzb_dev_alloc(&fresh[q], sizes[q]);
            if (e == hipSuccess && live && keep[q]) e = hipMemcpy(fresh[q], c->own_view[q], keep[q], hipMemcpyDeviceToDevice);
        }
        if (e != hipSuccess) {
            for (void* p : fresh)
                if (p) (void)hipFree(p);
            return e;
        }
        for (int q = 1; q < 6; q++) {
            if (c->own_view[q]) (void)hipFree(c->own_view[q]);
            c->own_view[q] = fresh[q];
        }
        c->view_cap_items = items;
        if (live) {
            c->dev.vgofs = (const u32*)c->own_view[1]; c->dev.vgnv = (const u8*)c->own_view[2]; c->dev.vlen = (const u16*)c->own_view[3];
            c->dev.vperm = (const u16*)c->own_view[4]; c->dev.vlong = (const u32*)c->own_view[5];
        }
    }
    if (units && (c->view_cap_units < units || !c->own_view[0])) {
        void* p = nullptr;
        hipError_t e = fzb_dev_alloc(&p, (size_t)units * 16 + 1024);
        if (e == hipSuccess) e = hipMemset(p, 0, (size_t)units * 16 + 1024);
        if (e == hipSuccess && live && keep_units) e = hipMemcpy(p, c->own_view[0], (size_t)keep_units * 16, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {
            if (p) (void)hipFree(p);
            return e;
        }
        if (c->own_view[0]) (void)hipFree(c->own_view[0]);
        c->own_view[0] = p;
        c->view_cap_units = units;
        if (live) c->dev.vbytes = (const u8*)p;
    }
    return hipSuccess;
}

// Brings the view in step with the list, whose figures (n, uniform_len, n_over256, max_short) are current.  The view's data for the first
// `n_valid` haystacks is good (0 for a first build; the old length after an append; the new one after a truncate): only the tiles from
// the one that holds haystack n_valid on are sorted and filled - the last, partial tile of before and what came behind it.
// No view, and FZB_OK, when the list does not call for one or the device has no room (see fzb_build_filter_view).
int view_sync(fzb_corpus* c, u64 n_valid) {
    const u64 n = c->dev.n;
    const bool want = !fzb_knobs().no_filter_view && n && !c->dev.uniform_len && c->max_short > 32 && c->n_over256 <= long_cap_of(n);
    auto bail = [&](hipError_t e) {
        (void)view_deactivate(c);
        view_free(c);
        return fzb_fail(FZB_ERR_HIP, std::string("filter view: ") + hipGetErrorString(e));
    };
    auto no_room = [&]() {  // the view is an accelerator, not part of the corpus: the filter then streams the canonical layout
        (void)view_deactivate(c);
        view_free(c);
        return FZB_OK;
    };
    hipError_t e;
    if (!want) {
        e = view_deactivate(c);
        return e == hipSuccess ? FZB_OK : bail(e);
    }
    const bool live = c->dev.vbytes != nullptr;
    if (!live) n_valid = 0;
    n_valid = std::min(n_valid, n);
    const u64 t0 = n_valid / UP_TILE, ntiles = up_tiles(n), tiles_r = ntiles - t0;
    const u64 old_units = live ? c->view_units : 0, old_tiles = live ? up_tiles(c->view_items) : 0;
    e = ensure_tiles_scratch(c, tiles_r);
    if (e == hipSuccess) e = view_ensure_room(c, std::max<u64>(n, c->cap_items), 0, std::min(c->view_items, t0 * UP_TILE + UP_TILE), old_units);
    if (e == hipErrorOutOfMemory) return no_room();
    if (e != hipSuccess) return bail(e);
    // where tile t0 starts in the view: where it started before, or - a tile of its own - behind everything
    u64 base_units = old_units;
    if (live && t0 < old_tiles) {
        u32 g = 0;
        e = hipMemcpy(&g, (const u32*)c->own_view[1] + t0 * (UP_TILE / 64), 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return bail(e);
        base_units = g;
    }
    UpStats* d_stats = (UpStats*)c->stage_stats;
    u64* d_vt = (u64*)c->stage_tiles;
    UpStats init = UP_STATS_INIT;
    init.bad = live ? c->dev.n_long : 0;  // the outlier list is appended to
    e = hipMemcpy(d_stats, &init, sizeof(init), hipMemcpyHostToDevice);
    if (e != hipSuccess) return bail(e);
    if (live && c->dev.n_long && c->view_items > t0 * UP_TILE)
        FZB_LAUNCH(k_up_vlong_prune, dim3(1), dim3(1024), 0, nullptr, (u32*)c->own_view[5], c->dev.n_long, (u32)(t0 * UP_TILE), d_stats);
    const u32 long_room = (u32)long_cap_of(c->view_cap_items);
    if (tiles_r) {
        if (c->dev.ends_u64)
            FZB_LAUNCH((k_up_view_sort<u64>), dim3((unsigned)tiles_r), dim3(UP_THREADS), 0, nullptr, (const u64*)c->dev.ends, n, (u16*)c->own_view[4], (u16*)c->own_view[3], (u8*)c->own_view[2], d_vt, d_stats, (u32*)c->own_view[5], long_room, (u32)t0);
        else
            FZB_LAUNCH((k_up_view_sort<u32>), dim3((unsigned)tiles_r), dim3(UP_THREADS), 0, nullptr, (const u32*)c->dev.ends, n, (u16*)c->own_view[4], (u16*)c->own_view[3], (u8*)c->own_view[2], d_vt, d_stats, (u32*)c->own_view[5], long_room, (u32)t0);
        FZB_LAUNCH(k_up_scan, dim3(1), dim3(1024), 0, nullptr, d_vt, tiles_r, d_stats);  // total_padded = the rebuilt tiles' size in 16-byte units
    }
    UpStats vst = UP_STATS_INIT;
    e = hipMemcpy(&vst, d_stats, sizeof(vst), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return bail(e);
    const u64 units = base_units + vst.total_padded;
    // no view: group offsets beyond 32 bits of 16-byte units (64 GB); (more outliers than the list holds: decided above, from the host's count)
    if (units > 0xFFFFFFF0ull || vst.bad > long_cap_of(n)) {
        e = view_deactivate(c);
        return e == hipSuccess ? FZB_OK : bail(e);
    }
    if (units > c->view_cap_units || !c->own_view[0]) {  // grows like the canonical arrays: twice the old room, or what a full list of the reserved size can take
        const u64 geo = std::max<u64>({units, 2 * c->view_cap_units, c->cap_items > n ? view_units_bound(c->cap_items, c->cap_bytes) : 0});
        e = view_ensure_room(c, c->view_cap_items, geo, 0, base_units);
        if (e == hipErrorOutOfMemory && geo > units) { (void)hipGetLastError(); e = view_ensure_room(c, c->view_cap_items, units, 0, base_units); }
        if (e == hipErrorOutOfMemory) return no_room();
        if (e != hipSuccess) return bail(e);
    }
    // the rebuilt tiles' old blocks: cleared (zero vectors behind a group's shorter members); everything behind the used part is zero already
    if (old_units > base_units) {
        e = hipMemsetAsync((u8*)c->own_view[0] + base_units * 16, 0, (old_units - base_units) * 16, nullptr);
        if (e != hipSuccess) return bail(e);
    }
    if (tiles_r) {
        if (c->dev.ends_u64)
            FZB_LAUNCH((k_up_view_fill<u64>), dim3((unsigned)tiles_r), dim3(UP_THREADS), 0, nullptr, c->dev.bytes, (const u64*)c->dev.ends, n, (const u16*)c->own_view[4], (const u8*)c->own_view[2], (const u64*)d_vt, (u8*)c->own_view[0], (u32*)c->own_view[1], (u32)t0, base_units);
        else
            FZB_LAUNCH((k_up_view_fill<u32>), dim3((unsigned)tiles_r), dim3(UP_THREADS), 0, nullptr, c->dev.bytes, (const u32*)c->dev.ends, n, (const u16*)c->own_view[4], (const u8*)c->own_view[2], (const u64*)d_vt, (u8*)c->own_view[0], (u32*)c->own_view[1], (u32)t0, base_units);
    }
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return bail(e);
    c->dev.vbytes = (const u8*)c->own_view[0];
    c->dev.vgofs = (const u32*)c->own_view[1];
    c->dev.vgnv = (const u8*)c->own_view[2];
    c->dev.vlen = (const u16*)c->own_view[3];
    c->dev.vperm = (const u16*)c->own_view[4];
    c->dev.vlong = (const u32*)c->own_view[5];
    c->dev.view_nv = (u32)((c->max_short + 15) >> 4);  // the view's widest member in vectors (outliers are not in it)
    c->dev.n_long = (u32)vst.bad;
    c->view_units = units;
    c->view_items = n;
    return FZB_OK;
}

// min / max length and the outlier figures of the first n haystacks of the resident list, into the corpus' host figures
hipError_t measure_resident(fzb_corpus* c, u64 n) {
    hipError_t e = ensure_tiles_scratch(c, 1);
    if (e != hipSuccess) return e;
    UpStats st = UP_STATS_INIT;
    if (n) {
        e = hipMemcpy(c->stage_stats, &UP_STATS_INIT, sizeof(UpStats), hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
        const unsigned grid = fzb_grid_cap((n + UP_THREADS - 1) / UP_THREADS, 8);  // (2048 on 256 CUs)
        if (c->dev.ends_u64) FZB_LAUNCH((k_up_measure<u64>), dim3(grid), dim3(UP_THREADS), 0, nullptr, (const u64*)c->dev.ends, n, (UpStats*)c->stage_stats);
        else FZB_LAUNCH((k_up_measure<u32>), dim3(grid), dim3(UP_THREADS), 0, nullptr, (const u32*)c->dev.ends, n, (UpStats*)c->stage_stats);
        e = hipMemcpy(&st, c->stage_stats, sizeof(st), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
    }
    c->min_len = st.min_len; c->max_len = st.max_len; c->n_over256 = st.n_long; c->max_short = st.max_short;
    return hipSuccess;
}

// ---- the letter signatures (sig_filter.h), kept in step with the list -----------------------------------------------------------------
// One thread per haystack of [first, first + count): both 16-byte vectors, cut to the haystack's length, OR-ed into CorpusDev::sig.
template <typename ET>
__global__ __launch_bounds__(UP_THREADS) void k_sig_build(const u8* __restrict__ bytes, const ET* __restrict__ ends, u32 ulen, u64 first, u64 count, u32* __restrict__ sig) {
    const u64 stride = (u64)gridDim.x * UP_THREADS;
    for (u64 k = (u64)blockIdx.x * UP_THREADS + threadIdx.x; k < count; k += stride) {
        u64 hs;
        u32 L;
        haystack_span_u(ends, ulen, first + k, hs, L);
        L = min(L, 32u);  // (the list's bound: fzb_sig_sync builds signatures for lists within it only)
        const uint4* vp = (const uint4*)(bytes + hs);
        uint4 a = make_uint4(0, 0, 0, 0), b = make_uint4(0, 0, 0, 0);
        if (L > 0) a = vp[0];
        if (L > 16) b = vp[1];
        u32 w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        u32 s = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const u32 nvb = L > 4u * j ? L - 4u * j : 0u;
            if (nvb < 4) w[j] &= (1u << (8 * nvb)) - 1;
            s |= sig_of_word(w[j]);
        }
        sig[first + k] = s;
    }
}

// Room for one array of bit-planes (sig_filter.h) of `items` haystacks, the first keep_tiles tiles taken over in one copy: own / cap_tiles /
// live = the corpus' allocation, its room and the pointer the kernels read (own_planes .. dev.sig_planes, or the repeat planes' three).
// An accelerator of an accelerator: without room the corpus goes on without that array (false) - without planes the filter reads the u32
// signatures, without repeat planes it tests the planes alone.
bool planes_ensure_room(void*& own, u64& cap_tiles, const u64*& live, u64 items, u64 keep_tiles) {
    const u64 tiles = sig_plane_tiles(items);
    if (own && cap_tiles >= tiles) return true;
    const size_t tile_bytes = 32 * FZB_SIG_PLANE_WORDS * sizeof(u64);
    void* p = nullptr;
    hipError_t e = fzb_dev_alloc(&p, (size_t)tiles * tile_bytes);
    if (e == hipSuccess && keep_tiles && own) e = hipMemcpy(p, own, (size_t)std::min(keep_tiles, cap_tiles) * tile_bytes, hipMemcpyDeviceToDevice);
    if (own) (void)hipFree(own);
    own = nullptr;
    cap_tiles = 0;
    if (e != hipSuccess) {
        if (p) (void)hipFree(p);
        (void)hipGetLastError();
        live = nullptr;
        return false;
    }
    own = p;
    cap_tiles = tiles;
    if (live) live = (const u64*)p;
    return true;
}

}  // namespace

int fzb_sig_sync(fzb_corpus* c, u64 n_valid) {
    const u64 n = c->dev.n;
    const bool want = !fzb_knobs().no_signature && n && c->dev.max_len != 0 && c->dev.max_len <= 32;
    if (!want) {  // (the arrays stay for the list that calls for signatures again)
        c->dev.sig = nullptr;
        c->dev.sig_planes = c->dev.sig_planes2 = nullptr;
        return FZB_OK;
    }
    if (!c->dev.sig) n_valid = 0, c->dev.sig_planes = c->dev.sig_planes2 = nullptr;
    n_valid = std::min(n_valid, n);
    const u64 planes_t0 = c->dev.sig_planes ? n_valid / FZB_SIG_PLANE_TILE : 0;  // the first tile whose planes are rebuilt
    const u64 planes2_t0 = c->dev.sig_planes2 ? n_valid / FZB_SIG_PLANE_TILE : 0;
    if (!c->own_sig || c->sig_cap_items < n) {
        const u64 items = std::max<u64>(n, c->cap_items);
        void* p = nullptr;
        hipError_t e = fzb_dev_alloc(&p, (size_t)items * 4);
        if (e == hipSuccess && n_valid) e = hipMemcpy(p, c->own_sig, (size_t)n_valid * 4, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {  // an accelerator, like the view: without room the corpus goes on without it
            if (p) (void)hipFree(p);
            (void)hipGetLastError();
            c->dev.sig = nullptr;
            c->dev.sig_planes = c->dev.sig_planes2 = nullptr;
            if (e == hipErrorOutOfMemory) return FZB_OK;
            return fzb_fail(FZB_ERR_HIP, std::string("letter signatures: ") + hipGetErrorString(e));
        }
        if (c->own_sig) (void)hipFree(c->own_sig);
        c->own_sig = p;
        c->sig_cap_items = items;
    }
    if (n > n_valid) {
        const u64 cnt = n - n_valid;
        const unsigned grid = fzb_grid_cap((cnt + UP_THREADS - 1) / UP_THREADS, 32);  // (8192 on 256 CUs)
        if (c->dev.ends_u64) FZB_LAUNCH((k_sig_build<u64>), dim3(grid), dim3(UP_THREADS), 0, nullptr, c->dev.bytes, (const u64*)c->dev.ends, c->dev.uniform_len, n_valid, cnt, (u32*)c->own_sig);
        else FZB_LAUNCH((k_sig_build<u32>), dim3(grid), dim3(UP_THREADS), 0, nullptr, c->dev.bytes, (const u32*)c->dev.ends, c->dev.uniform_len, n_valid, cnt, (u32*)c->own_sig);
    }
    c->dev.sig = (const u32*)c->own_sig;
    // the bit-planes of every tile from n_valid's on, out of the signatures just written (k_sig_planes_build, kernels_filter.hip)
    const u64 tiles = sig_plane_tiles(n);
    if (planes_ensure_room(c->own_planes, c->planes_cap_tiles, c->dev.sig_planes, std::max<u64>(n, c->cap_items), planes_t0)) {
        if (planes_t0 < tiles) fzb_launch_sig_planes(c->dev.sig, n, planes_t0, (u64*)c->own_planes, (int)fzb_grid_cap(tiles - planes_t0, 8), nullptr);
        c->dev.sig_planes = (const u64*)c->own_planes;
    }
    // ... and the REPEAT planes of the same tiles, out of the haystacks' bytes (k_sig_planes2_build); only beside the planes, whose form of the filter reads them
    if (!c->dev.sig_planes) c->dev.sig_planes2 = nullptr;
    else if (planes_ensure_room(c->own_planes2, c->planes2_cap_tiles, c->dev.sig_planes2, std::max<u64>(n, c->cap_items), planes2_t0)) {
        if (planes2_t0 < tiles) fzb_launch_sig_planes2(c->dev, n, planes2_t0, (u64*)c->own_planes2, (int)fzb_grid_cap(tiles - planes2_t0, 8), nullptr);
        c->dev.sig_planes2 = (const u64*)c->own_planes2;
    }
    return FZB_OK;
}

// A borrowed corpus (fzb_corpus_set_uniform_len / _set_max_len, behind their verifying pass): on the device its bytes live on
int fzb_sig_sync_borrowed(fzb_corpus* c) {
    int prev_dev = 0, own_dev = 0;
    HIPCHK(hipGetDevice(&prev_dev));
    own_dev = prev_dev;
    hipPointerAttribute_t attr;
    if (c->dev.bytes && hipPointerGetAttributes(&attr, c->dev.bytes) == hipSuccess && attr.type == hipMemoryTypeDevice) own_dev = attr.device;
    else (void)hipGetLastError();
    struct DeviceGuard {
        int prev, cur;
        ~DeviceGuard() { if (cur != prev) (void)hipSetDevice(prev); }
    } guard{prev_dev, own_dev};
    if (own_dev != prev_dev) HIPCHK(hipSetDevice(own_dev));
    if (c->own_sig && c->sig_device != own_dev) {  // (the array follows the bytes)
        (void)hipFree(c->own_sig);
        c->own_sig = nullptr; c->sig_cap_items = 0;
        if (c->own_planes) (void)hipFree(c->own_planes);
        c->own_planes = nullptr; c->planes_cap_tiles = 0;
        if (c->own_planes2) (void)hipFree(c->own_planes2);
        c->own_planes2 = nullptr; c->planes2_cap_tiles = 0;
    }
    c->dev.sig = nullptr;  // the promise changed: nothing of an earlier build is taken over
    c->dev.sig_planes = c->dev.sig_planes2 = nullptr;
    // FZB_VERIFY_PROMISES=0: nobody has checked the end offsets, and this set-up pass must not read wherever they point
    if (!fzb_knobs().verify_promises) return FZB_OK;
    HIPCHK(hipDeviceSynchronize());  // the caller may have filled the buffers on any stream of that device
    const int rc = fzb_sig_sync(c, 0);
    if (rc) return rc;
    if (c->dev.sig) {
        c->sig_device = own_dev;
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipGetLastError());
    }
    return FZB_OK;
}

// The streaming filter's view of a corpus whose canonical layout is resident (uploaded or borrowed), on the CURRENT device.  Sets
// c->dev.v* and view_nv on success; leaves the corpus without a view (and returns FZB_OK) when the list does not call for one - more
// than one haystack in 256 (+64) beyond 256 bytes (the few that are become OUTLIERS: listed in vlong, decided by k1_cdfa_outliers from
// the canonical layout), nothing beyond 32, a uniform-length list - or when the device has no room: the view is an accelerator,
// not part of the corpus (the filter then streams the canonical layout).  Any other error is reported.
int fzb_build_filter_view(fzb_corpus* c) {
    if (!c->dev.n || c->dev.uniform_len || c->dev.vbytes) return FZB_OK;
    if (!c->own_bytes) {  // borrowed: the lengths are read from the end offsets (an uploaded corpus knows its figures)
        const hipError_t e = measure_resident(c, c->dev.n);
        if (e != hipSuccess) return fzb_fail(FZB_ERR_HIP, std::string("filter view: ") + hipGetErrorString(e));
    }
    return view_sync(c, 0);
}

// For a BORROWED corpus (fzb_corpus_upload builds the view itself): the lengths are read from the end offsets,
// so no hint is needed and a wrong fzb_corpus_set_max_len cannot mislead it.  *out_built (optional) = 1 when the corpus has a view now.
extern "C" int fzb_corpus_build_view(fzb_corpus* c, int* out_built) {
    if (!c) return fzb_fail(FZB_ERR_INVALID, "null argument");
    const int rc = fzb_build_filter_view(c);
    if (out_built) *out_built = c->dev.vbytes != nullptr;
    return rc;
}

// The upload proper, on the CURRENT device: `bytes` points at the first byte of haystack 0 of this list, `end_offsets[i]` are exclusive
// ends counted from `ends_base` (0 for a whole list; a shard passes the end of the haystack before its first one).
int fzb_corpus_upload_impl(const uint8_t* bytes, const uint64_t* end_offsets, size_t n, uint64_t ends_base, fzb_corpus** out) {
    if (!out || (n && (!bytes || !end_offsets))) return fzb_fail(FZB_ERR_INVALID, "null argument");
    if (n > 0xFFFFFFFFull)
        return fzb_fail(FZB_ERR_PANIC, "too many items in haystack, will overflow the u32 index: " + std::to_string(n) + " > 4294967295 (index offset: 0)");
    if (n && end_offsets[n - 1] < ends_base) return fzb_fail(FZB_ERR_INVALID, "end_offsets must be non-decreasing");
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    const u64 raw_bytes = n ? end_offsets[n - 1] - ends_base : 0;
    const u64 ntiles = up_tiles(n);
    auto c = new fzb_corpus();
    c->device = device;
    u8* d_raw = nullptr;
    u64* d_ends64 = nullptr;
    auto cleanup = [&]() {
        for (void* p : {(void*)d_raw, (void*)d_ends64})
            if (p) (void)hipFree(p);
    };
    auto bail = [&](hipError_t e, const char* what) {
        cleanup();
        fzb_corpus_free(c);
        return fzb_fail(FZB_ERR_HIP, std::string("corpus upload (") + what + "): " + hipGetErrorString(e));
    };
    hipError_t e = fzb_dev_alloc((void**)&d_raw, raw_bytes + 96);
    if (e == hipSuccess) e = fzb_dev_alloc((void**)&d_ends64, std::max<size_t>(n, 1) * 8);
    if (e == hipSuccess) e = ensure_tiles_scratch(c, ntiles);  // (tile sums + stats stay with the corpus: the view's passes and later appends use them)
    if (e != hipSuccess) return bail(e, "device buffers");
    e = hipMemset(d_raw + raw_bytes, 0, 96);
    if (e == hipSuccess) e = h2d_all({H2DJob{d_ends64, end_offsets, n * 8}, H2DJob{d_raw, bytes, (size_t)raw_bytes}}, device);
    if (e != hipSuccess) return bail(e, "host to device");
    c->h2d_bytes = raw_bytes + (u64)n * 8;
    UpStats st = UP_STATS_INIT;
    if (n) {
        e = batch_measure(d_ends64, n, ends_base, (u64*)c->stage_tiles, (UpStats*)c->stage_stats, &st);  // the one synchronisation of the upload: sizes the padded buffer
        if (e != hipSuccess) return bail(e, "layout pass");
        if (st.bad) {
            cleanup();
            fzb_corpus_free(c);
            return fzb_fail(FZB_ERR_INVALID, "end_offsets must be non-decreasing");
        }
    }
    const u64 total = st.total_padded + 96;
    const bool ends_u64 = total > 0xFFFFFFF0ull;
    const bool adopt = st.total_padded == raw_bytes;  // every length a multiple of 16: the upload format is the device layout
    c->dev.n = n;
    c->dev.total_bytes = total;
    c->dev.ends_u64 = ends_u64;
    c->min_len = st.min_len; c->max_len = st.max_len; c->n_over256 = st.n_long; c->max_short = st.max_short;
    set_measured(c);
    e = fzb_dev_alloc(&c->own_ends, std::max<size_t>(n, 1) * (ends_u64 ? 8 : 4));
    if (e == hipSuccess && !adopt) e = fzb_dev_alloc(&c->own_bytes, total);
    if (e != hipSuccess) return bail(e, "padded layout");
    if (adopt) {
        c->own_bytes = d_raw;
        d_raw = nullptr;
    } else {
        e = hipMemsetAsync((u8*)c->own_bytes + st.total_padded, 0, 96, nullptr);
        if (e != hipSuccess) return bail(e, "padded layout");
    }
    c->cap_items = std::max<size_t>(n, 1);
    c->cap_bytes = total;
    if (n) batch_lay_out(adopt ? (const u8*)c->own_bytes : d_raw, d_ends64, n, ends_base, (const u64*)c->stage_tiles, (u8*)c->own_bytes, 0, c->own_ends, 0, ends_u64, !adopt);
    c->dev.bytes = (const u8*)c->own_bytes;
    c->dev.ends = c->own_ends;
    // the streaming filter's view (CorpusDev::vbytes): ragged lists whose haystacks are 33..256 bytes.  A second copy of the bytes (+ ~5 %
    // for the zero vectors behind shorter group members, + 4.2 bytes per haystack); FZB_FILTER_VIEW=0 turns it off.
    int rc = view_sync(c, 0);  // (a list with more than a few haystacks beyond 256 bytes gets none)
    if (!rc) rc = fzb_sig_sync(c, 0);  // the letter signatures of a list of short haystacks (4 bytes per haystack)
    if (rc) {
        const std::string msg = fzb_last_error();
        cleanup();
        fzb_corpus_free(c);
        return fzb_fail(rc, msg);
    }
    e = hipDeviceSynchronize();  // the temporaries are released below; the corpus is complete when the call returns
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return bail(e, "layout kernels");
    cleanup();
    *out = c;
    return FZB_OK;
}

extern "C" int fzb_corpus_upload(const uint8_t* bytes, const uint64_t* end_offsets, size_t n, fzb_corpus** out) {
    return fzb_corpus_upload_impl(bytes, end_offsets, n, 0, out);
}

// ---- a corpus that grows ---------------------------------------------------------------------------------------------------------
namespace {

// set-up calls on a corpus the library owns, on its device, with nothing of the device's earlier work outstanding
int grow_begin(fzb_corpus* c, const char* what) {
    if (!c) return fzb_fail(FZB_ERR_INVALID, "null argument");
    if (!c->own_bytes)
        return fzb_fail(FZB_ERR_INVALID, std::string(what) + ": the corpus borrows its device memory (fzb_corpus_from_device); only a corpus made by fzb_corpus_upload can change");
    int device = 0;
    HIPCHK(hipGetDevice(&device));
    if (device != c->device) return fzb_fail(FZB_ERR_INVALID, std::string(what) + ": the corpus lives on device " + std::to_string(c->device) + ", the current device is " + std::to_string(device));
    HIPCHK(hipDeviceSynchronize());
    return FZB_OK;
}

// a fresh device buffer of `bytes` (first try) or `exact` bytes; *got = the size obtained
hipError_t alloc_geometric(void** p, u64 bytes, u64 exact, u64* got) {
    hipError_t e = fzb_dev_alloc(p, bytes);
    *got = bytes;
    if (e == hipErrorOutOfMemory && exact < bytes) {
        (void)hipGetLastError();
        e = fzb_dev_alloc(p, exact);
        *got = exact;
    }
    return e;
}

// Room for `items` haystacks and `bytes` bytes of padded layout + tail in the canonical arrays; what is resident moves device to device.
// geometric: an array that lacks room gets at least twice what it had (the exact size when the device refuses that).  On an error
// nothing has changed.
hipError_t canon_ensure_room(fzb_corpus* c, u64 items, u64 bytes, bool geometric) {
    const u64 esz = c->dev.ends_u64 ? 8 : 4;
    void *nb = nullptr, *ne = nullptr;
    u64 got_b = 0, got_e = 0;
    hipError_t e = hipSuccess;
    u64 want_bytes = bytes > c->cap_bytes ? (geometric ? std::max(bytes, 2 * c->cap_bytes) : bytes) : c->cap_bytes;
    if (items > c->cap_items) {
        const u64 want_items = geometric ? std::max(items, 2 * c->cap_items) : items;
        // the bytes follow the items: room for the new item capacity at the list's average length so far (+ 1/16), so that the two arrays
        // regrow in the same call and the regrows of a list ingested in equal batches stay logarithmic in their number
        if (geometric && bytes > 96) want_bytes = std::max(want_bytes, std::min<u64>((u64)((double)(bytes - 96) / (double)items * (double)want_items * 1.0625) + 96,
                                                                                       c->dev.ends_u64 ? ~(u64)0 : 0xFFFFFFF0ull));
        e = alloc_geometric(&ne, want_items * esz, items * esz, &got_e);
        if (e == hipSuccess && c->dev.n) e = hipMemcpy(ne, c->own_ends, c->dev.n * esz, hipMemcpyDeviceToDevice);
    }
    if (e == hipSuccess && want_bytes > c->cap_bytes) {
        if (bytes > c->cap_bytes) e = alloc_geometric(&nb, want_bytes, bytes, &got_b);
        else if (fzb_dev_alloc(&nb, want_bytes) == hipSuccess) got_b = want_bytes;  // (following the items only: refused by the device, the bytes stay as they are)
        else { nb = nullptr; (void)hipGetLastError(); }
        const u64 used = c->dev.total_bytes - 96;
        if (e == hipSuccess && nb && used) e = hipMemcpy(nb, c->own_bytes, used, hipMemcpyDeviceToDevice);
        if (e == hipSuccess && nb) e = hipMemset((u8*)nb + used, 0, got_b - used);  // zero behind the list, wherever it will end
    }
    if (e != hipSuccess) {
        if (nb) (void)hipFree(nb);
        if (ne) (void)hipFree(ne);
        return e;
    }
    if (ne) {
        (void)hipFree(c->own_ends);
        c->own_ends = ne;
        c->dev.ends = ne;
        c->cap_items = got_e / esz;
    }
    if (nb) {
        (void)hipFree(c->own_bytes);
        c->own_bytes = nb;
        c->dev.bytes = (const u8*)nb;
        c->cap_bytes = got_b;
    }
    if (nb || ne) c->regrows++;
    return hipSuccess;
}

// the landing place of a batch as it arrives: `items` u64 offsets, `raw` bytes (+ the slack k_up_build's dword reads may touch)
hipError_t stage_ensure_room(fzb_corpus* c, u64 items, u64 raw) {
    hipError_t e = ensure_tiles_scratch(c, up_tiles(items) + 1);
    if (e == hipSuccess && (!c->stage_ends || c->stage_items_cap < items)) {
        void* p = nullptr;
        e = fzb_dev_alloc(&p, std::max<u64>(items, 1) * 8);
        if (e == hipSuccess) {
            if (c->stage_ends) (void)hipFree(c->stage_ends);
            c->stage_ends = p;
            c->stage_items_cap = std::max<u64>(items, 1);
        }
    }
    if (e == hipSuccess && (!c->stage_raw || c->stage_raw_cap < raw)) {
        void* p = nullptr;
        e = fzb_dev_alloc(&p, raw + 96);
        if (e == hipSuccess) {
            if (c->stage_raw) (void)hipFree(c->stage_raw);
            c->stage_raw = p;
            c->stage_raw_cap = raw;
        }
    }
    return e;
}

// ---- the per-haystack columns in step with the list: the score bias (score_bias.h; query side: host.hip's apply_bias) and the tags --------
// (scope.h; host.hip's apply_terms).  One set of rules (ItemColumn, host_internal.h), written once for both.  Invariant, as for the bytes:
// every entry at or behind the list's length is ZERO (the array is cleared when allocated, by truncate, by a removal's freed tail and by
// clear), so appended haystacks start at 0 and a column that is not live keeps an all-zero array, if any.
static_assert(SBIAS_TILE == UP_TILE, "k_col_compact walks the edit pass' tiles");
constexpr u64 PAIR_STAGE_MIN_PAIRS = 4096;  // pairs an update stages without another allocation once a column exists

// room for `items` entries; the first n of a live column move device to device.  On an error nothing has changed.
template <typename V>
hipError_t col_ensure_room(ItemColumn<V>& col, u64 n, u64 items) {
    if (col.data && col.cap_items >= items) return hipSuccess;
    void* p = nullptr;
    const u64 cap = std::max<u64>(items, 8);
    hipError_t e = fzb_dev_alloc(&p, cap * sizeof(V));
    if (e == hipSuccess) e = hipMemset(p, 0, cap * sizeof(V));
    if (e == hipSuccess && col.live && n) e = hipMemcpy(p, col.data, n * sizeof(V), hipMemcpyDeviceToDevice);
    if (e != hipSuccess) {
        if (p) (void)hipFree(p);
        return e;
    }
    if (col.data) (void)hipFree(col.data);
    col.data = (V*)p;
    col.cap_items = cap;
    return hipSuccess;
}
// a column that exists follows the item capacity (reserve, append): appends within the room allocate nothing
template <typename V>
hipError_t col_follow(fzb_corpus* c, ItemColumn<V>& col, u64 items) {
    return col.data ? col_ensure_room(col, c->dev.n, items) : hipSuccess;
}
hipError_t pair_stage_ensure(fzb_corpus* c, u64 pairs) {
    if (c->pair_stage && c->pair_stage_cap >= pairs) return hipSuccess;
    void* p = nullptr;
    const u64 cap = std::max(pairs, PAIR_STAGE_MIN_PAIRS);
    const hipError_t e = fzb_dev_alloc(&p, cap * 6);
    if (e != hipSuccess) return e;
    if (c->pair_stage) (void)hipFree(c->pair_stage);
    c->pair_stage = p;
    c->pair_stage_cap = cap;
    return hipSuccess;
}
// the array (all zero on first use, sized for max(len, reserved items)) and the landing place of an update's pairs
template <typename V>
hipError_t col_create(fzb_corpus* c, ItemColumn<V>& col, u64 stage_pairs) {
    hipError_t e = col_ensure_room(col, c->dev.n, std::max(c->dev.n, c->cap_items));
    if (e == hipSuccess) e = pair_stage_ensure(c, stage_pairs);
    return e;
}

// sparse "set": col[idx[k]] = val[k]; the indices are unique (checked on the host), so no two threads write one entry
// (V: the column's 2-byte value type - int16_t for the bias, uint16_t for the tags)
template <typename V>
__global__ __launch_bounds__(UP_THREADS) void k_col_scatter(const u32* __restrict__ idx, const V* __restrict__ val, u64 n_pairs, V* __restrict__ col, u64 len) {
    const u64 stride = (u64)gridDim.x * UP_THREADS;
    for (u64 k = (u64)blockIdx.x * UP_THREADS + threadIdx.x; k < n_pairs; k += stride) {
        const u32 i = idx[k];
        if (i < len) col[i] = val[k];
    }
}

// The remove compaction of a column: one workgroup per 1024-haystack SOURCE tile of the suffix from i0 on (the edit pass' tiles), a
// wave per 64 haystacks.  A haystack whose bit of the pass' bitmap is clear is kept: its rank inside the wave from the wave's ballot, the
// waves' totals through LDS, the tile's base = the pass' scanned per-tile kept count.  Written to scratch (a removal moves entries towards
// lower indices, into tiles another workgroup may not have read yet); the copy into place is a separate, stream-ordered step.
template <typename V>
__global__ __launch_bounds__(SBIAS_TILE) void k_col_compact(const V* __restrict__ col, const u32* __restrict__ bitmap, const u64* __restrict__ tile_cnt, u64 n, u64 i0,
                                                            V* __restrict__ out, u64 out_cap) {
    __shared__ u32 s_total[SBIAS_WAVES];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 t0 = i0 + (u64)blockIdx.x * SBIAS_TILE;
    const bool kept = sbias_tile_keeps(bitmap, n, t0, wave, lane);
    const u64 mask = __ballot(kept);
    if (lane == 0) s_total[wave] = (u32)__popcll(mask);
    __syncthreads();
    if (kept) sbias_tile_place(col, t0, wave, lane, mask, s_total, tile_cnt[blockIdx.x], out, out_cap);
}

// ---- the set-up calls of a column, behind the entry point's argument checks and grow_begin; `what` = the public call, for the messages ----
// one value per haystack, from the host; complete on return
template <typename V>
int col_set(fzb_corpus* c, ItemColumn<V>& col, const char* what, const V* values, size_t n) {
    if ((u64)n != c->dev.n)
        return fzb_fail(FZB_ERR_INVALID, std::string(what) + ": " + std::to_string(n) + " values for the corpus' " + std::to_string(c->dev.n) + " haystacks (one per haystack)");
    hipError_t e = col_create(c, col, 0);
    if (e == hipSuccess && n) e = hipMemcpy(col.data, values, n * sizeof(V), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fzb_fail(FZB_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    HIPCHK(hipDeviceSynchronize());
    return FZB_OK;
}
// col[indices[k]] = values[k] for n > 0 unique indices in range (a column that does not exist yet: an all-zero one first); complete on return
template <typename V>
int col_update(fzb_corpus* c, ItemColumn<V>& col, const std::string& what, const uint32_t* indices, const V* values, size_t n) {
    for (size_t k = 0; k < n; k++)
        if (indices[k] >= c->dev.n)
            return fzb_fail(FZB_ERR_INVALID, what + ": index " + std::to_string(indices[k]) + " at position " + std::to_string(k) + " is beyond the corpus' " + std::to_string(c->dev.n) +
                                                 " haystacks");
    std::vector<u32> order(n);
    for (size_t k = 0; k < n; k++) order[k] = (u32)k;
    std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return indices[a] != indices[b] ? indices[a] < indices[b] : a < b; });
    for (size_t k = 1; k < n; k++)
        if (indices[order[k]] == indices[order[k - 1]])
            return fzb_fail(FZB_ERR_INVALID, what + ": haystack " + std::to_string(indices[order[k]]) + " is named twice (positions " + std::to_string(order[k - 1]) + " and " +
                                                 std::to_string(order[k]) + ")");
    // the pairs travel in one copy: n indices, then n values
    std::vector<u8> pairs(n * 6);
    memcpy(pairs.data(), indices, n * 4);
    memcpy(pairs.data() + n * 4, values, n * 2);
    hipError_t e = col_create(c, col, n);
    if (e == hipSuccess) e = hipMemcpy(c->pair_stage, pairs.data(), pairs.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fzb_fail(FZB_ERR_HIP, what + ": " + hipGetErrorString(e));
    const unsigned grid = fzb_grid_cap((n + UP_THREADS - 1) / UP_THREADS, 4);  // (1024 on 256 CUs)
    FZB_LAUNCH(k_col_scatter<V>, dim3(grid), dim3(UP_THREADS), 0, nullptr, (const u32*)c->pair_stage, (const V*)((const u8*)c->pair_stage + n * 4), (u64)n, col.data, c->dev.n);
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return fzb_fail(FZB_ERR_HIP, what + " (scatter): " + hipGetErrorString(e));
    return FZB_OK;
}
// a live column back to all zero, the allocation kept; complete on return, and the caller's flags change only then
template <typename V>
int col_clear(ItemColumn<V>& col) {
    if (!col.live) return FZB_OK;
    HIPCHK(hipMemset(col.data, 0, col.cap_items * sizeof(V)));
    HIPCHK(hipDeviceSynchronize());
    return FZB_OK;
}
// truncate: the entries of the cut haystacks [n, n_old)
template <typename V>
hipError_t col_truncate(ItemColumn<V>& col, u64 n_old, u64 n) {
    return col.live ? hipMemsetAsync(col.data + n, 0, (n_old - n) * sizeof(V), nullptr) : hipSuccess;
}

}  // namespace

extern "C" {

int fzb_corpus_set_bias(fzb_corpus* c, const int16_t* values, size_t n) {
    if (!c || (n && !values)) return fzb_fail(FZB_ERR_INVALID, "null argument");
    int rc = grow_begin(c, "fzb_corpus_set_bias");
    if (!rc) rc = col_set(c, c->bias, "fzb_corpus_set_bias", values, n);
    if (rc) return rc;
    int32_t hi = 0;
    for (size_t k = 0; k < n; k++) hi = std::max<int32_t>(hi, values[k]);
    c->bias_hi = (u32)hi;
    c->bias.live = true;
    return FZB_OK;
}

int fzb_corpus_update_bias(fzb_corpus* c, const uint32_t* indices, const int16_t* values, size_t n) {
    if (!c || (n && (!indices || !values))) return fzb_fail(FZB_ERR_INVALID, "null argument");
    int rc = grow_begin(c, "fzb_corpus_update_bias");
    if (rc || !n) return rc;
    if ((rc = col_update(c, c->bias, "fzb_corpus_update_bias", indices, values, n))) return rc;
    int32_t hi = c->bias.live ? (int32_t)c->bias_hi : 0;
    for (size_t k = 0; k < n; k++) hi = std::max<int32_t>(hi, values[k]);
    c->bias_hi = (u32)hi;
    c->bias.live = true;
    return FZB_OK;
}

int fzb_corpus_clear_bias(fzb_corpus* c) {
    int rc = grow_begin(c, "fzb_corpus_clear_bias");
    if (!rc) rc = col_clear(c->bias);
    if (rc) return rc;
    c->bias.live = false;  // (the array stays, all zero: the invariant of a column that is not live)
    c->bias_hi = 0;
    return FZB_OK;
}

int fzb_corpus_bias_info(const fzb_corpus* c, uint64_t out[4]) {
    if (!c || !out) return fzb_fail(FZB_ERR_INVALID, "null argument");
    out[0] = c->bias.live ? 1 : 0;
    out[1] = c->bias.cap_items;
    out[2] = fzb_corpus_bias_hi(c);
    out[3] = c->bias.cap_items * sizeof(int16_t) + c->pair_stage_cap * 6;
    return FZB_OK;
}

// the tags are live from the moment their array exists, whatever became of the call that allocated it
static int tags_made(fzb_corpus* c, int rc) {
    c->tags.live = c->tags.data != nullptr;
    return rc;
}

int fzb_corpus_set_tags(fzb_corpus* c, const uint16_t* values, size_t n) {
    if (!c || (n && !values)) return fzb_fail(FZB_ERR_INVALID, "null argument");
    int rc = grow_begin(c, "fzb_corpus_set_tags");
    if (rc) return rc;
    return tags_made(c, col_set(c, c->tags, "fzb_corpus_set_tags", values, n));
}

int fzb_corpus_update_tags(fzb_corpus* c, const uint32_t* indices, const uint16_t* values, size_t n) {
    if (!c || (n && (!indices || !values))) return fzb_fail(FZB_ERR_INVALID, "null argument");
    int rc = grow_begin(c, "fzb_corpus_update_tags");
    if (rc || !n) return rc;
    return tags_made(c, col_update(c, c->tags, "fzb_corpus_update_tags", indices, values, n));
}

int fzb_corpus_clear_tags(fzb_corpus* c) {
    int rc = grow_begin(c, "fzb_corpus_clear_tags");
    if (!rc) rc = col_clear(c->tags);
    if (rc) return rc;
    c->scope_require = c->scope_exclude = 0;  // (the scope changes only once the tags are zero)
    return FZB_OK;
}

int fzb_corpus_set_scope(fzb_corpus* c, uint16_t require, uint16_t exclude) {
    if (!c) return fzb_fail(FZB_ERR_INVALID, "null argument");
    if (!c->tags.data) {  // the first scope of a corpus without tags: an all-zero array, under the set-up calls' rules
        int rc = grow_begin(c, "fzb_corpus_set_scope");
        if (rc) return rc;
        const hipError_t e = col_create(c, c->tags, 0);
        tags_made(c, 0);
        if (e != hipSuccess) return fzb_fail(FZB_ERR_HIP, std::string("fzb_corpus_set_scope: ") + hipGetErrorString(e));
        HIPCHK(hipDeviceSynchronize());
    }
    c->scope_require = require;  // host only: the two words travel as kernel arguments of the next query
    c->scope_exclude = exclude;
    return FZB_OK;
}

int fzb_corpus_scope_info(const fzb_corpus* c, uint64_t out[4]) {
    if (!c || !out) return fzb_fail(FZB_ERR_INVALID, "null argument");
    out[0] = fzb_corpus_scoped(c) ? 1 : 0;
    out[1] = c->tags.cap_items;
    out[2] = (u64)c->scope_require | ((u64)c->scope_exclude << 16);
    out[3] = c->tags.cap_items * sizeof(uint16_t);
    return FZB_OK;
}

int fzb_corpus_reserve(fzb_corpus* c, size_t items, uint64_t bytes) {
    int rc = grow_begin(c, "fzb_corpus_reserve");
    if (rc) return rc;
    if (items > 0xFFFFFFFFull)
        return fzb_fail(FZB_ERR_PANIC, "too many items in haystack, will overflow the u32 index: " + std::to_string(items) + " > 4294967295 (index offset: 0)");
    if (!c->dev.ends_u64 && bytes + 96 > 0xFFFFFFF0ull)
        return fzb_fail(FZB_ERR_CAPACITY, "fzb_corpus_reserve: a corpus whose end offsets are 32-bit holds less than 4 GiB of padded bytes");
    const u64 regrows = c->regrows;
    hipError_t e = canon_ensure_room(c, items, bytes + 96, false);
    c->regrows = regrows;  // (room asked for is not a regrow)
    // a batch may be as large as the room: its landing place, and - unless FZB_FILTER_VIEW=0 - the view's arrays, are sized for that
    if (e == hipSuccess) e = stage_ensure_room(c, c->cap_items - c->dev.n, c->cap_bytes - c->dev.total_bytes);
    if (e == hipSuccess) e = ensure_tiles_scratch(c, up_tiles(c->cap_items) + 1);
    if (e == hipSuccess) e = col_follow(c, c->bias, c->cap_items);  // the columns follow the item capacity: appends within the room allocate nothing
    if (e == hipSuccess) e = col_follow(c, c->tags, c->cap_items);
    if (e != hipSuccess) return fzb_fail(FZB_ERR_HIP, std::string("fzb_corpus_reserve: ") + hipGetErrorString(e));
    if (!fzb_knobs().no_filter_view) {
        const u64 live_units = c->dev.vbytes ? c->view_units : 0;
        e = view_ensure_room(c, c->cap_items, std::max(c->view_cap_units, view_units_bound(c->cap_items, c->cap_bytes)), c->view_items, live_units);
        if (e == hipErrorOutOfMemory) (void)hipGetLastError();  // the view is an accelerator: the corpus has its room, the view grows - or goes - when it must
        else if (e != hipSuccess) return fzb_fail(FZB_ERR_HIP, std::string("fzb_corpus_reserve (filter view): ") + hipGetErrorString(e));
    }
    // the letter signatures of a list that has (or, still empty, may get) them: room for the item capacity, so that appends allocate nothing
    if (!fzb_knobs().no_signature && (!c->dev.n || (c->dev.max_len != 0 && c->dev.max_len <= 32)) && c->sig_cap_items < c->cap_items) {
        void* p = nullptr;
        e = fzb_dev_alloc(&p, (size_t)c->cap_items * 4);
        if (e == hipSuccess && c->dev.sig && c->dev.n) e = hipMemcpy(p, c->own_sig, (size_t)c->dev.n * 4, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) {
            if (c->own_sig) (void)hipFree(c->own_sig);
            c->own_sig = p;
            c->sig_cap_items = c->cap_items;
            if (c->dev.sig) c->dev.sig = (const u32*)p;
        } else {
            if (p) (void)hipFree(p);
            (void)hipGetLastError();  // (an accelerator: it grows - or goes - when it must)
        }
    }
    // ... and their bit-planes and the repeat planes, another 4 bytes per haystack each, behind them
    if (!fzb_knobs().no_signature && (!c->dev.n || (c->dev.max_len != 0 && c->dev.max_len <= 32)) && c->own_sig && c->sig_cap_items >= c->cap_items) {
        if (planes_ensure_room(c->own_planes, c->planes_cap_tiles, c->dev.sig_planes, c->cap_items, c->dev.sig_planes ? sig_plane_tiles(c->dev.n) : 0))
            (void)planes_ensure_room(c->own_planes2, c->planes2_cap_tiles, c->dev.sig_planes2, c->cap_items, c->dev.sig_planes2 ? sig_plane_tiles(c->dev.n) : 0);
        if (!c->dev.sig_planes) c->dev.sig_planes2 = nullptr;
    }
    HIPCHK(hipDeviceSynchronize());
    return FZB_OK;
}

int fzb_corpus_append(fzb_corpus* c, const uint8_t* bytes, const uint64_t* end_offsets, size_t n_new) {
    if (!c || (n_new && !end_offsets)) return fzb_fail(FZB_ERR_INVALID, "null argument");
    const u64 raw = n_new ? end_offsets[n_new - 1] : 0;
    if (raw && !bytes) return fzb_fail(FZB_ERR_INVALID, "null argument");
    int rc = grow_begin(c, "fzb_corpus_append");
    if (rc) return rc;
    if (!n_new) return FZB_OK;
    const u64 n_old = c->dev.n;
    if (n_old + (u64)n_new > 0xFFFFFFFFull)
        return fzb_fail(FZB_ERR_PANIC, "too many items in haystack, will overflow the u32 index: " + std::to_string(n_old + (u64)n_new) + " > 4294967295 (index offset: 0)");
    // the batch travels as it is, one copy per array, and is validated where it lands: nothing of the corpus is written before
    hipError_t e = stage_ensure_room(c, n_new, raw);
    if (e == hipSuccess) e = h2d_all({H2DJob{c->stage_ends, end_offsets, n_new * 8}, H2DJob{c->stage_raw, bytes, (size_t)raw}}, c->device);
    UpStats st = UP_STATS_INIT;
    if (e == hipSuccess) e = batch_measure((const u64*)c->stage_ends, n_new, 0, (u64*)c->stage_tiles, (UpStats*)c->stage_stats, &st);
    if (e != hipSuccess) return fzb_fail(FZB_ERR_HIP, std::string("fzb_corpus_append (host to device): ") + hipGetErrorString(e));
    if (st.bad) return fzb_fail(FZB_ERR_INVALID, "end_offsets must be non-decreasing");
    const u64 used = c->dev.total_bytes - 96;  // a multiple of 16: where the batch's first haystack starts
    const u64 total = used + st.total_padded + 96;
    if (!c->dev.ends_u64 && total > 0xFFFFFFF0ull)
        return fzb_fail(FZB_ERR_CAPACITY, "fzb_corpus_append: the batch takes the padded list to 4 GiB, beyond this corpus' 32-bit end offsets; upload such a list in one piece");
    e = canon_ensure_room(c, n_old + n_new, total, true);
    // (the columns regrow with the items, device to device; the new haystacks' entries are zero by the invariant)
    if (e == hipSuccess) e = col_follow(c, c->bias, std::max<u64>(n_old + n_new, c->cap_items));
    if (e == hipSuccess) e = col_follow(c, c->tags, std::max<u64>(n_old + n_new, c->cap_items));
    if (e != hipSuccess) return fzb_fail(FZB_ERR_HIP, std::string("fzb_corpus_append (room for the batch): ") + hipGetErrorString(e));
    batch_lay_out((const u8*)c->stage_raw, (const u64*)c->stage_ends, n_new, 0, (const u64*)c->stage_tiles, (u8*)c->own_bytes, used, c->own_ends, n_old, c->dev.ends_u64 != 0, true);
    c->h2d_bytes += raw + (u64)n_new * 8;
    c->dev.n = n_old + n_new;
    c->dev.total_bytes = total;
    c->generation++;
    c->min_len = std::min(c->min_len, st.min_len);
    c->max_len = std::max(c->max_len, st.max_len);
    c->max_short = std::max(c->max_short, st.max_short);
    c->n_over256 += st.n_long;
    set_measured(c);
    rc = view_sync(c, n_old);
    if (!rc) rc = fzb_sig_sync(c, n_old);
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipGetLastError();
    if (rc) return rc;
    if (e != hipSuccess) return fzb_fail(FZB_ERR_HIP, std::string("fzb_corpus_append (layout kernels): ") + hipGetErrorString(e));
    return FZB_OK;
}

int fzb_corpus_truncate(fzb_corpus* c, size_t n) {
    int rc = grow_begin(c, "fzb_corpus_truncate");
    if (rc) return rc;
    if (n > c->dev.n) return fzb_fail(FZB_ERR_INVALID, "fzb_corpus_truncate: " + std::to_string(n) + " is beyond the corpus' " + std::to_string(c->dev.n) + " haystacks");
    if (n == c->dev.n) return FZB_OK;
    u64 used = 0;
    if (n) {  // the kept list ends where its last haystack does, rounded up to the layout's 16 bytes
        u64 last = 0;
        const size_t esz = c->dev.ends_u64 ? 8 : 4;
        HIPCHK(hipMemcpy(&last, (const u8*)c->own_ends + (n - 1) * esz, esz, hipMemcpyDeviceToHost));
        used = (last + 15) & ~(u64)15;
    }
    const u64 old_used = c->dev.total_bytes - 96;
    if (old_used > used) HIPCHK(hipMemsetAsync((u8*)c->own_bytes + used, 0, old_used - used, nullptr));  // gaps and tail are zero
    hipError_t e = measure_resident(c, n);
    if (e == hipSuccess) e = col_truncate(c->bias, c->dev.n, n);  // the cut haystacks' biases and tags
    if (e == hipSuccess) e = col_truncate(c->tags, c->dev.n, n);
    if (e != hipSuccess) return fzb_fail(FZB_ERR_HIP, std::string("fzb_corpus_truncate: ") + hipGetErrorString(e));
    c->dev.n = n;
    c->dev.total_bytes = used + 96;
    c->generation++;
    set_measured(c);
    rc = view_sync(c, n);
    if (!rc) rc = fzb_sig_sync(c, n);
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipGetLastError();
    if (rc) return rc;
    if (e != hipSuccess) return fzb_fail(FZB_ERR_HIP, std::string("fzb_corpus_truncate: ") + hipGetErrorString(e));
    return FZB_OK;
}

int fzb_corpus_info(const fzb_corpus* c, uint64_t out[12]) {
    if (!c || !out) return fzb_fail(FZB_ERR_INVALID, "null argument");
    const bool own = c->own_bytes != nullptr;
    out[0] = c->dev.n;
    out[1] = own ? std::max<u64>(c->cap_items, c->dev.n) : c->dev.n;
    out[2] = c->dev.total_bytes >= 96 && own ? c->dev.total_bytes - 96 : c->dev.total_bytes;
    out[3] = own ? c->cap_bytes - 96 : c->dev.total_bytes;
    out[4] = c->dev.max_len;
    out[5] = c->dev.uniform_len;
    out[6] = c->dev.vbytes != nullptr;
    out[7] = c->dev.vbytes ? c->dev.view_nv : 0;
    out[8] = c->dev.vbytes ? c->dev.n_long : 0;
    out[9] = c->dev.ends_u64 != 0;
    out[10] = c->regrows;
    out[11] = c->h2d_bytes;
    return FZB_OK;
}

int fzb_corpus_signature_info(const fzb_corpus* c, int* out_built, uint64_t* out_bytes) {
    if (!c) return fzb_fail(FZB_ERR_INVALID, "null argument");
    if (out_built) *out_built = c->dev.sig != nullptr;
    if (out_bytes) *out_bytes = c->dev.sig ? (uint64_t)c->dev.n * 4 : 0;
    return FZB_OK;
}

int fzb_corpus_signature_planes_info(const fzb_corpus* c, int* out_built, uint64_t* out_bytes) {
    if (!c) return fzb_fail(FZB_ERR_INVALID, "null argument");
    if (out_built) *out_built = c->dev.sig_planes != nullptr;
    if (out_bytes) *out_bytes = c->dev.sig_planes ? sig_plane_words(c->dev.n) * 8 : 0;
    return FZB_OK;
}

int fzb_corpus_signature_repeat_planes_info(const fzb_corpus* c, int* out_built, uint64_t* out_bytes) {
    if (!c) return fzb_fail(FZB_ERR_INVALID, "null argument");
    if (out_built) *out_built = c->dev.sig_planes2 != nullptr;
    if (out_bytes) *out_bytes = c->dev.sig_planes2 ? sig_plane_words(c->dev.n) * 8 : 0;
    return FZB_OK;
}

int fzb_debug_corpus_read(const fzb_corpus* c, int what, void* host_out, size_t cap_bytes, size_t* out_bytes) {
    if (!c || !out_bytes) return fzb_fail(FZB_ERR_INVALID, "null argument");
    const u64 n = c->dev.n, groups = up_tiles(n) * (UP_TILE / 64);
    const bool view = c->dev.vbytes != nullptr;
    const void* src = nullptr;
    size_t bytes = 0;
    switch (what) {
        case 0: src = c->dev.bytes; bytes = c->own_bytes ? (size_t)c->dev.total_bytes : 0; break;  // (a borrowed buffer's tail is its owner's)
        case 1: src = c->dev.ends; bytes = (size_t)n * (c->dev.ends_u64 ? 8 : 4); break;
        case 2: src = c->dev.vbytes; bytes = view ? (size_t)c->view_units * 16 : 0; break;
        case 3: src = c->dev.vgofs; bytes = view ? (size_t)groups * 4 : 0; break;
        case 4: src = c->dev.vgnv; bytes = view ? (size_t)groups : 0; break;
        case 5: src = c->dev.vlen; bytes = view ? (size_t)n * 2 : 0; break;
        case 6: src = c->dev.vperm; bytes = view ? (size_t)n * 2 : 0; break;
        case 7: src = c->dev.vlong; bytes = view ? (size_t)c->dev.n_long * 4 : 0; break;
        case 8: src = c->dev.sig; bytes = c->dev.sig ? (size_t)n * 4 : 0; break;
        case 9: src = c->bias.data; bytes = c->bias.live ? (size_t)n * sizeof(int16_t) : 0; break;
        case 10: src = c->tags.data; bytes = c->tags.live ? (size_t)n * sizeof(uint16_t) : 0; break;
        case 11: src = c->dev.sig_planes; bytes = c->dev.sig_planes ? (size_t)sig_plane_words(n) * 8 : 0; break;
        case 12: src = c->dev.sig_planes2; bytes = c->dev.sig_planes2 ? (size_t)sig_plane_words(n) * 8 : 0; break;
        default: return fzb_fail(FZB_ERR_INVALID, "fzb_debug_corpus_read: unknown array " + std::to_string(what));
    }
    *out_bytes = bytes;
    if (!bytes) return FZB_OK;
    if (!host_out || cap_bytes < bytes) return fzb_fail(FZB_ERR_CAPACITY, "fzb_debug_corpus_read: the array has " + std::to_string(bytes) + " bytes");
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(host_out, src, bytes, hipMemcpyDeviceToHost));
    return FZB_OK;
}

}  // extern "C"

// ---- a corpus that is EDITED: haystacks removed or replaced anywhere in the list ----------------------------------------------------
// One pass serves both ("Layout under edit").  i0 = the first touched haystack; nothing in front of it is read or
// written.  The suffix from i0 on is cut into tiles of 1024 SOURCE haystacks:
//   k_ed_mark     checks the index list where it lies (HBM) and sets one bit per touched haystack (vector atomics on u32 words); the
//                 lowest touched index and the first bad position come back in the pass' first readback
//   k_ed_tiles    per tile: sum of the NEW padded lengths (0 for a dropped haystack, the batch item's for a replaced one) and the
//                 number of haystacks kept
//   k_ed_scan     exclusive scan of both (one workgroup); the totals - the suffix' new size - come back in the second readback, which
//                 decides capacity, room and scratch: every check and allocation lies before the first write to a resident array
//   k_ed_gather   per tile: new starts and end offsets (scan in LDS), and the bytes - one thread per 16-byte OUTPUT vector, as in
//                 k_up_build; a kept haystack is read as whole aligned vectors from the resident layout (its zero padding comes along),
//                 a replacement through the funnel shift from the staged batch
//   k_ed_place    copies what the gather produced to its place in the canonical arrays
// The gather writes to SCRATCH, never to the resident arrays: a removal moves data towards lower addresses, so a tile's destination
// overlaps sources of tiles that another workgroup may not have read yet.  Nothing rests on the order in which the workgroups of one
// launch run: gather and place are separate, stream-ordered launches.  The suffix goes through the scratch in CHUNKS of
// FZB_EDIT_CHUNK_ITEMS source haystacks (knobs.h; 1 Mi by default), gather then place per chunk, front to back: placing chunk c is safe when
// its destination ends at or before the place where chunk c + 1's first source haystack starts - always so for a removal, and for a
// replace unless growing items push data towards higher addresses; k_ed_scan checks every chunk boundary, and a pass that fails the
// check takes the whole suffix through the scratch as one chunk.  A memset clears what the list no longer covers.
namespace {

struct EdStats {
    u64 bad_pos, first, count, new_bytes, new_items, start0;
    u64 max_chunk_bytes, forward_ok;  // the largest chunk's new bytes; 1 = chunks can be placed front to back
};
const EdStats ED_STATS_INIT{~(u64)0, ~(u64)0, 0, 0, 0, 0, 0, 0};

// what a touched haystack becomes: dropped (replace = 0), or item rk[k] of the staged batch, k = the position of its index in the sorted ridx
struct EdSrc {
    const u32* bitmap;
    const u32* ridx;
    const u32* rk;
    const u64* bends;  // the batch's exclusive end offsets, from its first byte
    u32 n_repl;
    u32 replace;
};

__device__ __forceinline__ bool ed_touched(const EdSrc& s, u64 i) { return (s.bitmap[i >> 5] >> (i & 31)) & 1u; }
// the batch item that replaces haystack i (i is in ridx): its first byte in the batch and its length
__device__ __forceinline__ void ed_batch_item(const EdSrc& s, u64 i, u64* from, u64* len) {
    u32 lo = 0, hi = s.n_repl;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (s.ridx[mid] <= (u32)i) lo = mid;
        else hi = mid;
    }
    const u32 k = s.rk[lo];
    const u64 b = k ? s.bends[k - 1] : 0;
    *from = b;
    *len = s.bends[k] - b;
}

// entry k of the list = the u32 at word k * stride_words; count = min(*dev_count, max_count) (dev_count == nullptr: max_count)
__global__ __launch_bounds__(UP_THREADS) void k_ed_mark(const u32* __restrict__ idx, u64 stride_words, const u32* __restrict__ dev_count, u64 max_count, u64 n,
                                                        u32* __restrict__ bitmap, EdStats* __restrict__ st) {
    const u64 cnt = dev_count ? min((u64)*dev_count, max_count) : max_count;
    u64 first = ~(u64)0, bad = ~(u64)0;
    const u64 stride = (u64)gridDim.x * UP_THREADS;
    for (u64 k = (u64)blockIdx.x * UP_THREADS + threadIdx.x; k < cnt; k += stride) {
        const u32 v = idx[k * stride_words];
        if (v >= n) bad = min(bad, k);
        else {
            atomicOr(&bitmap[v >> 5], 1u << (v & 31));
            first = min(first, (u64)v);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        first = min(first, (u64)__shfl_xor(first, off));
        bad = min(bad, (u64)__shfl_xor(bad, off));
    }
    if ((threadIdx.x & 63) == 0) {
        if (first != ~(u64)0) atomicMin((unsigned long long*)&st->first, (unsigned long long)first);
        if (bad != ~(u64)0) atomicMin((unsigned long long*)&st->bad_pos, (unsigned long long)bad);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) st->count = cnt;
}

template <typename ET>
__global__ __launch_bounds__(UP_THREADS) void k_ed_tiles(const ET* __restrict__ ends, u64 n, u64 i0, EdSrc src, u64* __restrict__ tile_bytes, u64* __restrict__ tile_cnt,
                                                         u64* __restrict__ tile_start, EdStats* __restrict__ st) {
    __shared__ u64 s_sum[UP_THREADS / 64];
    __shared__ u32 s_cnt[UP_THREADS / 64];
    u64 sum = 0;
    u32 kept = 0;
#pragma unroll
    for (int k = 0; k < UP_TILE / UP_THREADS; k++) {
        const u64 i = i0 + (u64)blockIdx.x * UP_TILE + (u64)k * UP_THREADS + threadIdx.x;
        if (i < n) {
            const u64 start = i ? ((u64)ends[i - 1] + 15) & ~(u64)15 : 0;
            u64 len = (u64)ends[i] - start, from;
            bool keep = true;
            if (ed_touched(src, i)) {
                if (src.replace) ed_batch_item(src, i, &from, &len);
                else keep = false;
            }
            if (keep) {
                sum += (len + 15) & ~(u64)15;
                kept++;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off);
        kept += __shfl_xor(kept, off);
    }
    if ((threadIdx.x & 63) == 0) {
        s_sum[threadIdx.x >> 6] = sum;
        s_cnt[threadIdx.x >> 6] = kept;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = 0, k = 0;
        for (int w = 0; w < UP_THREADS / 64; w++) {
            t += s_sum[w];
            k += s_cnt[w];
        }
        tile_bytes[blockIdx.x] = t;
        tile_cnt[blockIdx.x] = k;
        // where the tile's first haystack starts NOW: a later chunk's gather cannot read it from the end offsets, which an earlier chunk's
        // place may have rewritten up to the entry before it
        const u64 t0 = i0 + (u64)blockIdx.x * UP_TILE;
        tile_start[blockIdx.x] = t0 ? ((u64)ends[t0 - 1] + 15) & ~(u64)15 : 0;
        if (blockIdx.x == 0) st->start0 = tile_start[0];  // where haystack i0 starts: where the new suffix will
    }
}

// exclusive scan of the tiles' new bytes and kept counts in place (k_up_scan's form, two values at a time); entry [ntiles] = the totals.
// Then, over the chunks of `chunk_tiles` tiles: the largest chunk's new bytes, and whether every chunk's destination ends at or before
// the start of the first source haystack behind it.
__global__ __launch_bounds__(1024) void k_ed_scan(u64* __restrict__ tile_bytes, u64* __restrict__ tile_cnt, const u64* __restrict__ tile_start, u64 ntiles, EdStats* __restrict__ st,
                                                  u64 chunk_tiles) {
    __shared__ u64 s_wb[16], s_wc[16];
    __shared__ u64 s_cb, s_cc;
    if (threadIdx.x == 0) s_cb = s_cc = 0;
    __syncthreads();
    for (u64 base = 0; base < ntiles; base += 1024) {
        const u64 i = base + threadIdx.x;
        const u64 vb = i < ntiles ? tile_bytes[i] : 0, vc = i < ntiles ? tile_cnt[i] : 0;
        u64 ib = vb, ic = vc;
        for (int off = 1; off < 64; off <<= 1) {
            const u64 tb = __shfl_up(ib, off), tc = __shfl_up(ic, off);
            if ((int)(threadIdx.x & 63) >= off) {
                ib += tb;
                ic += tc;
            }
        }
        if ((threadIdx.x & 63) == 63) {
            s_wb[threadIdx.x >> 6] = ib;
            s_wc[threadIdx.x >> 6] = ic;
        }
        __syncthreads();
        u64 wb = 0, wc = 0;
        for (u32 w = 0; w < (threadIdx.x >> 6); w++) {
            wb += s_wb[w];
            wc += s_wc[w];
        }
        const u64 cb = s_cb, cc = s_cc;
        if (i < ntiles) {
            tile_bytes[i] = cb + wb + ib - vb;
            tile_cnt[i] = cc + wc + ic - vc;
        }
        __syncthreads();
        if (threadIdx.x == 1023) {
            s_cb = cb + wb + ib;
            s_cc = cc + wc + ic;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        st->new_bytes = s_cb;
        st->new_items = s_cc;
        tile_bytes[ntiles] = s_cb;
        tile_cnt[ntiles] = s_cc;
    }
    __syncthreads();
    const u64 start0 = tile_start[0];
    u64 mx = 0;
    bool ok = true;
    for (u64 t = (u64)threadIdx.x * chunk_tiles; t < ntiles; t += 1024 * chunk_tiles) {
        const u64 te = min(ntiles, t + chunk_tiles);
        mx = max(mx, tile_bytes[te] - tile_bytes[t]);
        if (te < ntiles && start0 + tile_bytes[te] > tile_start[te]) ok = false;  // (tile te's first haystack: the first source behind the chunk)
    }
    if (mx) atomicMax((unsigned long long*)&st->max_chunk_bytes, (unsigned long long)mx);
    if (threadIdx.x == 0) st->forward_ok = 1;
    __syncthreads();
    if (!ok) st->forward_ok = 0;
}

// One chunk of the new suffix (the tiles from `tile_first` on, one per workgroup), out of place: its bytes from byte 0 of `out` on, its
// end offsets - in the canonical layout's terms, where the suffix starts at byte start0 - from entry 0 of `out_ends` on.
template <typename ET>
__global__ __launch_bounds__(UP_THREADS) void k_ed_gather(const u8* __restrict__ bytes, const ET* __restrict__ ends, u64 n, u64 i0, EdSrc src, const u8* __restrict__ braw,
                                                          const u64* __restrict__ tile_bytes, const u64* __restrict__ tile_cnt, const u64* __restrict__ tile_start, u8* __restrict__ out,
                                                          ET* __restrict__ out_ends, u64 start0, u64 tile_first) {
    __shared__ u64 s_pstart[UP_TILE + 1];  // new padded start of each source haystack of the tile, relative to the tile's base (a dropped one takes no room)
    __shared__ u64 s_from[UP_TILE];        // where its bytes are read: byte position in the resident layout, or in the batch | FROM_BATCH
    __shared__ u64 s_len[UP_TILE];
    __shared__ u64 s_wave[UP_THREADS / 64];
    __shared__ u32 s_wcnt[UP_THREADS / 64];
    constexpr u64 FROM_BATCH = (u64)1 << 63;
    const u64 tile = tile_first + blockIdx.x;
    const u64 t0 = i0 + tile * UP_TILE;
    const u64 base = tile_bytes[tile], chunk_base = tile_bytes[tile_first];
    const u64 first = t0 + (u64)threadIdx.x * 4;
    u64 prev_end = threadIdx.x == 0 ? tile_start[tile] : (first < n ? (u64)ends[first - 1] : 0);  // (a start is its own round-up)
    u64 plen[4], len[4], mine = 0;
    u32 keep[4], mykept = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u64 i = first + k;
        u64 from = 0;
        len[k] = 0;
        keep[k] = 0;
        if (i < n) {
            const u64 start = (prev_end + 15) & ~(u64)15;
            prev_end = (u64)ends[i];
            len[k] = prev_end - start;
            from = start;
            keep[k] = 1;
            if (ed_touched(src, i)) {
                if (src.replace) {
                    ed_batch_item(src, i, &from, &len[k]);
                    from |= FROM_BATCH;
                } else {
                    keep[k] = 0;
                    len[k] = 0;
                }
            }
        }
        s_from[threadIdx.x * 4 + k] = from;
        s_len[threadIdx.x * 4 + k] = len[k];
        plen[k] = (len[k] + 15) & ~(u64)15;
        mine += plen[k];
        mykept += keep[k];
    }
    u64 incl = mine;
    u32 cincl = mykept;
    for (int off = 1; off < 64; off <<= 1) {
        const u64 t = __shfl_up(incl, off);
        const u32 c = __shfl_up(cincl, off);
        if ((int)(threadIdx.x & 63) >= off) {
            incl += t;
            cincl += c;
        }
    }
    if ((threadIdx.x & 63) == 63) {
        s_wave[threadIdx.x >> 6] = incl;
        s_wcnt[threadIdx.x >> 6] = cincl;
    }
    __syncthreads();
    u64 run = incl - mine;
    u64 rank = tile_cnt[tile] - tile_cnt[tile_first] + cincl - mykept;
    for (u32 w = 0; w < (threadIdx.x >> 6); w++) {
        run += s_wave[w];
        rank += s_wcnt[w];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        s_pstart[threadIdx.x * 4 + k] = run;
        if (keep[k]) out_ends[rank++] = (ET)(start0 + base + run + len[k]);
        run += plen[k];
    }
    if (threadIdx.x == UP_THREADS - 1) s_pstart[UP_TILE] = run;
    __syncthreads();
    const u64 tile_total = s_pstart[UP_TILE];
    const u32 cnt = (u32)min((u64)UP_TILE, n - t0);
    for (u64 v = (u64)threadIdx.x * 16u; v < tile_total; v += UP_THREADS * 16u) {
        // the haystack this output vector belongs to: last j with pstart[j] <= v (dropped and empty haystacks share a start with their
        // successor: the search lands on the last of them, the one that owns the bytes)
        u32 lo = 0, hi = cnt;
        while (hi - lo > 1) {
            const u32 mid = (lo + hi) >> 1;
            if (s_pstart[mid] <= v) lo = mid;
            else hi = mid;
        }
        const u64 off = v - s_pstart[lo], from = s_from[lo];
        const u64 hlen = s_len[lo];
        uint4 q = make_uint4(0, 0, 0, 0);
        if (off < hlen) {
            if (!(from & FROM_BATCH)) {
                q = *(const uint4*)(bytes + from + off);  // resident: aligned, and zero behind the haystack's last byte
            } else {
                const u64 p = (from & ~FROM_BATCH) + off;  // byte position in the batch
                const u32 rem = (u32)min((u64)16, hlen - off);
                const u32* a = (const u32*)(braw + (p & ~(u64)3));
                const u32 sh = (u32)(p & 3);
                // 16 bytes from an arbitrary byte position: five aligned dwords, funnel-shifted (the landing buffer has 96 readable bytes of slack)
                const u32 w0 = a[0], w1 = a[1], w2 = a[2], w3 = a[3], w4 = sh ? a[4] : 0u;
                u32 x[4] = {__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh), __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh)};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const u32 lo_b = 4u * k;
                    if (rem <= lo_b) x[k] = 0;
                    else if (rem - lo_b < 4) x[k] &= (1u << (8 * (rem - lo_b))) - 1;
                }
                q = make_uint4(x[0], x[1], x[2], x[3]);
            }
        }
        *(uint4*)(out + (base - chunk_base) + v) = q;
    }
}

// the chunk of tiles [tile_first, tile_end), gathered into `src_b` / `src_e`, to its place: bytes to start0 + its base, offsets to i0 + its rank
template <typename ET>
__global__ __launch_bounds__(UP_THREADS) void k_ed_place(const u8* __restrict__ src_b, const ET* __restrict__ src_e, const u64* __restrict__ tile_bytes,
                                                         const u64* __restrict__ tile_cnt, u64 tile_first, u64 tile_end, u8* __restrict__ bytes, ET* __restrict__ ends, u64 start0, u64 i0) {
    const u64 vecs = (tile_bytes[tile_end] - tile_bytes[tile_first]) / 16, items = tile_cnt[tile_end] - tile_cnt[tile_first];
    const uint4* s = (const uint4*)src_b;
    uint4* d = (uint4*)(bytes + start0 + tile_bytes[tile_first]);
    ET* de = ends + i0 + tile_cnt[tile_first];
    const u64 stride = (u64)gridDim.x * UP_THREADS;
    for (u64 v = (u64)blockIdx.x * UP_THREADS + threadIdx.x; v < vecs; v += stride) d[v] = s[v];
    for (u64 k = (u64)blockIdx.x * UP_THREADS + threadIdx.x; k < items; k += stride) de[k] = src_e[k];
}

inline u64 round_up(u64 v, u64 a) { return (v + a - 1) / a * a; }

struct EditRequest {
    const char* what;
    // the touched indices: in host memory (copied into the pass' scratch), or where the caller keeps them in HBM
    const u32* host_idx = nullptr;
    const void* dev_idx = nullptr;
    u64 stride_words = 1;
    const u32* dev_count = nullptr;
    u64 max_count = 0;
    // replace: host_idx is sorted, host_rk[k] = the item of the staged batch (c->stage_raw / c->stage_ends) that haystack host_idx[k] becomes
    const u32* host_rk = nullptr;
    u64 batch_h2d = 0;
};

// A removal's scratch of one column: the kept entries of the suffix from i0 on pass through it, 2 bytes per suffix haystack.  A replace keeps
// every entry where it is (the index map is the identity) and a column that is not live is all zero: neither needs any.
template <typename V>
struct ColScratch {
    V* work = nullptr;
    u64 bytes = 0;
};
template <typename V>
u64 col_scratch_bytes(const ItemColumn<V>& col, bool replace, u64 suffix) {
    return (!replace && col.live) ? round_up(suffix * sizeof(V), 16) : 0;
}
template <typename V>
hipError_t col_scratch_alloc(ColScratch<V>& s, u64 bytes) {
    if (!bytes) return hipSuccess;
    const hipError_t e = fzb_dev_alloc((void**)&s.work, bytes);
    if (e == hipSuccess) s.bytes = bytes;
    else s.work = nullptr;
    return e;
}
// the kept entries from i0 on, compacted through the scratch, copied into place, the freed tail [n_new, n) cleared
template <typename V>
hipError_t col_compact(ItemColumn<V>& col, const ColScratch<V>& s, const u32* bitmap, const u64* tile_cnt, u64 tiles, u64 n, u64 i0, u64 n_new) {
    if (!s.work) return hipSuccess;
    FZB_LAUNCH(k_col_compact<V>, dim3((unsigned)tiles), dim3(SBIAS_TILE), 0, nullptr, (const V*)col.data, bitmap, tile_cnt, n, i0, s.work, n - i0);
    hipError_t e = hipSuccess;
    if (n_new > i0) e = hipMemcpyAsync(col.data + i0, s.work, (n_new - i0) * sizeof(V), hipMemcpyDeviceToDevice, nullptr);
    if (e == hipSuccess && n > n_new) e = hipMemsetAsync(col.data + n_new, 0, (n - n_new) * sizeof(V), nullptr);
    return e;
}

// grow_begin has passed.  Everything up to canon_ensure_room only reads the corpus: an error before it leaves nothing to undo.
int edit_run(fzb_corpus* c, const EditRequest& rq) {
    const std::string what = rq.what;
    const bool replace = rq.host_rk != nullptr;
    const u64 n = c->dev.n, esz = c->dev.ends_u64 ? 8 : 4;
    const u64 tiles_cap = up_tiles(n) + 1;
    // scratch of the pass itself, one allocation: stats | bitmap | three tile arrays | the index list (host form) | the batch's item numbers
    const u64 off_bitmap = 64, off_tb = off_bitmap + round_up((n + 31) / 32 * 4, 8), off_tc = off_tb + tiles_cap * 8, off_ts = off_tc + tiles_cap * 8, off_idx = off_ts + tiles_cap * 8;
    const u64 off_rk = off_idx + (rq.host_idx ? round_up(rq.max_count * 4, 8) : 0), aux_bytes = off_rk + (replace ? rq.max_count * 4 : 0);
    u8* aux = nullptr;
    u8* work = nullptr;
    ColScratch<int16_t> bias_tmp;  // a removal on a corpus with live columns
    ColScratch<uint16_t> tags_tmp;
    auto done = [&](int rc) {
        if (aux) (void)hipFree(aux);
        if (work) (void)hipFree(work);
        if (bias_tmp.work) (void)hipFree(bias_tmp.work);
        if (tags_tmp.work) (void)hipFree(tags_tmp.work);
        return rc;
    };
    auto hip_fail = [&](hipError_t e, const char* where) { return done(fzb_fail(FZB_ERR_HIP, what + " (" + where + "): " + hipGetErrorString(e))); };
    hipError_t e = fzb_dev_alloc((void**)&aux, aux_bytes);
    if (e != hipSuccess) { aux = nullptr; return hip_fail(e, "scratch"); }
    EdStats* d_st = (EdStats*)aux;
    u32* d_bitmap = (u32*)(aux + off_bitmap);
    u64 *d_tb = (u64*)(aux + off_tb), *d_tc = (u64*)(aux + off_tc), *d_ts = (u64*)(aux + off_ts);
    e = hipMemsetAsync(aux, 0, off_tb, nullptr);
    if (e == hipSuccess) e = hipMemcpy(d_st, &ED_STATS_INIT, sizeof(EdStats), hipMemcpyHostToDevice);
    if (e == hipSuccess && rq.host_idx) e = hipMemcpy(aux + off_idx, rq.host_idx, rq.max_count * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && replace) e = hipMemcpy(aux + off_rk, rq.host_rk, rq.max_count * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "scratch");
    const u32* d_idx = rq.host_idx ? (const u32*)(aux + off_idx) : (const u32*)rq.dev_idx;
    const unsigned mark_grid = fzb_grid_cap((rq.max_count + UP_THREADS - 1) / UP_THREADS, 8);  // (2048 on 256 CUs)
    FZB_LAUNCH(k_ed_mark, dim3(mark_grid), dim3(UP_THREADS), 0, nullptr, d_idx, rq.stride_words, rq.dev_count, rq.max_count, n, d_bitmap, d_st);
    EdStats st = ED_STATS_INIT;
    e = hipMemcpy(&st, d_st, sizeof(st), hipMemcpyDeviceToHost);  // first readback: is the list valid, and where does the edit begin
    if (e != hipSuccess) return hip_fail(e, "index list");
    if (st.bad_pos != ~(u64)0)
        return done(fzb_fail(FZB_ERR_INVALID, what + ": the index at position " + std::to_string(st.bad_pos) + " of the list is beyond the corpus' " + std::to_string(n) + " haystacks"));
    if (!st.count) return done(FZB_OK);
    const u64 i0 = st.first, tiles = up_tiles(n - i0);
    EdSrc src{d_bitmap, replace ? d_idx : nullptr, replace ? (const u32*)(aux + off_rk) : nullptr, (const u64*)c->stage_ends, (u32)(replace ? rq.max_count : 0), replace ? 1u : 0u};
    if (c->dev.ends_u64) FZB_LAUNCH((k_ed_tiles<u64>), dim3((unsigned)tiles), dim3(UP_THREADS), 0, nullptr, (const u64*)c->dev.ends, n, i0, src, d_tb, d_tc, d_ts, d_st);
    else FZB_LAUNCH((k_ed_tiles<u32>), dim3((unsigned)tiles), dim3(UP_THREADS), 0, nullptr, (const u32*)c->dev.ends, n, i0, src, d_tb, d_tc, d_ts, d_st);
    const u64 chunk_knob = (u64)fzb_knobs().edit_chunk_items / UP_TILE;
    FZB_LAUNCH(k_ed_scan, dim3(1), dim3(1024), 0, nullptr, d_tb, d_tc, (const u64*)d_ts, tiles, d_st, chunk_knob);
    e = hipMemcpy(&st, d_st, sizeof(st), hipMemcpyDeviceToHost);  // second readback: the new suffix' size
    if (e != hipSuccess) return hip_fail(e, "sizing pass");
    const u64 old_used = c->dev.total_bytes - 96, new_used = st.start0 + st.new_bytes, total = new_used + 96, n_new = i0 + st.new_items;
    if (!c->dev.ends_u64 && total > 0xFFFFFFF0ull)
        return done(fzb_fail(FZB_ERR_CAPACITY, what + ": the new content takes the padded list to 4 GiB, beyond this corpus' 32-bit end offsets; upload such a list in one piece"));
    // where the new suffix is gathered: the corpus' landing buffers when they are free (a replace's batch lies in them) and large enough
    const u64 chunk_tiles = st.forward_ok ? chunk_knob : tiles;  // (front to back, or everything through the scratch at once)
    const u64 need_b = st.forward_ok ? st.max_chunk_bytes : st.new_bytes, need_e = std::min(st.new_items, chunk_tiles * UP_TILE) * esz;
    u8* out_b = (!replace && c->stage_raw && c->stage_raw_cap + 96 >= need_b) ? (u8*)c->stage_raw : nullptr;
    u8* out_e = (!replace && c->stage_ends && c->stage_items_cap * 8 >= need_e) ? (u8*)c->stage_ends : nullptr;
    const u64 work_b = out_b ? 0 : round_up(need_b, 16), work_bytes = work_b + (out_e ? 0 : need_e);
    if (work_bytes) {
        e = fzb_dev_alloc((void**)&work, work_bytes);
        if (e != hipSuccess) { work = nullptr; return hip_fail(e, "scratch for the new suffix"); }
        if (!out_b) out_b = work;
        if (!out_e) out_e = work + work_b;
    }
    if ((e = col_scratch_alloc(bias_tmp, col_scratch_bytes(c->bias, replace, n - i0))) != hipSuccess) return hip_fail(e, "scratch for the score bias");
    if ((e = col_scratch_alloc(tags_tmp, col_scratch_bytes(c->tags, replace, n - i0))) != hipSuccess) return hip_fail(e, "scratch for the tags");
    if (total > c->cap_bytes) {
        e = canon_ensure_room(c, n_new, total, true);
        if (e != hipSuccess) return hip_fail(e, "room for the new content");
    }
    // ---- from here on the corpus changes ----
    for (u64 ta = 0; ta < tiles; ta += chunk_tiles) {
        const u64 te = std::min(tiles, ta + chunk_tiles);
        const unsigned place_grid = fzb_grid_cap((te - ta) * 4, 16);  // (4096 on 256 CUs)
        if (c->dev.ends_u64) {
            FZB_LAUNCH((k_ed_gather<u64>), dim3((unsigned)(te - ta)), dim3(UP_THREADS), 0, nullptr, (const u8*)c->own_bytes, (const u64*)c->own_ends, n, i0, src, (const u8*)c->stage_raw, d_tb, d_tc, d_ts, out_b, (u64*)out_e, st.start0, ta);
            FZB_LAUNCH((k_ed_place<u64>), dim3(place_grid), dim3(UP_THREADS), 0, nullptr, (const u8*)out_b, (const u64*)out_e, d_tb, d_tc, ta, te, (u8*)c->own_bytes, (u64*)c->own_ends, st.start0, i0);
        } else {
            FZB_LAUNCH((k_ed_gather<u32>), dim3((unsigned)(te - ta)), dim3(UP_THREADS), 0, nullptr, (const u8*)c->own_bytes, (const u32*)c->own_ends, n, i0, src, (const u8*)c->stage_raw, d_tb, d_tc, d_ts, out_b, (u32*)out_e, st.start0, ta);
            FZB_LAUNCH((k_ed_place<u32>), dim3(place_grid), dim3(UP_THREADS), 0, nullptr, (const u8*)out_b, (const u32*)out_e, d_tb, d_tc, ta, te, (u8*)c->own_bytes, (u32*)c->own_ends, st.start0, i0);
        }
    }
    e = hipSuccess;
    if (e == hipSuccess && old_used > new_used) e = hipMemsetAsync((u8*)c->own_bytes + new_used, 0, old_used - new_used, nullptr);  // gaps and tail are zero
    const bool had_view = c->dev.vbytes != nullptr;
    if (e == hipSuccess) e = measure_resident(c, n_new);
    if (e == hipSuccess) e = col_compact(c->bias, bias_tmp, d_bitmap, d_tc, tiles, n, i0, n_new);
    if (e == hipSuccess) e = col_compact(c->tags, tags_tmp, d_bitmap, d_tc, tiles, n, i0, n_new);
    if (e != hipSuccess) return hip_fail(e, "layout");
    c->dev.n = n_new;
    c->dev.total_bytes = total;
    c->h2d_bytes += rq.batch_h2d;
    c->generation++;
    set_measured(c);
    int rc = view_sync(c, i0);
    if (!rc) rc = fzb_sig_sync(c, i0);
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipGetLastError();
    if (rc) return done(rc);
    if (e != hipSuccess) return hip_fail(e, "layout kernels");
    c->edit_info[0] = i0;
    c->edit_info[1] = st.new_bytes + (old_used > new_used ? old_used - new_used : 0) + st.new_items * esz;
    c->edit_info[2] = c->dev.vbytes ? up_tiles(n_new) - (had_view ? std::min(i0, n_new) / UP_TILE : 0) : 0;
    c->edit_info[3] = aux_bytes + work_bytes + bias_tmp.bytes + tags_tmp.bytes;
    return done(FZB_OK);
}

}  // namespace

extern "C" {

int fzb_corpus_remove_device(fzb_corpus* c, const void* dev_indices, size_t stride_bytes, const uint32_t* dev_count, size_t max_count) {
    if (!c || !dev_indices || !dev_count) return fzb_fail(FZB_ERR_INVALID, "null argument");
    if (stride_bytes < 4 || (stride_bytes & 3)) return fzb_fail(FZB_ERR_INVALID, "fzb_corpus_remove_device: stride_bytes must be a multiple of 4, at least 4");
    if (((uintptr_t)dev_indices & 3) || ((uintptr_t)dev_count & 3)) return fzb_fail(FZB_ERR_INVALID, "fzb_corpus_remove_device: dev_indices and dev_count must be 4-byte aligned");
    int rc = grow_begin(c, "fzb_corpus_remove_device");
    if (rc) return rc;
    if (!max_count) return FZB_OK;
    EditRequest rq;
    rq.what = "fzb_corpus_remove_device";
    rq.dev_idx = dev_indices;
    rq.stride_words = stride_bytes / 4;
    rq.dev_count = dev_count;
    rq.max_count = max_count;
    return edit_run(c, rq);
}

int fzb_corpus_remove(fzb_corpus* c, const uint32_t* indices, size_t n_indices) {
    if (!c || (n_indices && !indices)) return fzb_fail(FZB_ERR_INVALID, "null argument");
    int rc = grow_begin(c, "fzb_corpus_remove");
    if (rc) return rc;
    if (!n_indices) return FZB_OK;
    for (size_t k = 0; k < n_indices; k++)
        if (indices[k] >= c->dev.n)
            return fzb_fail(FZB_ERR_INVALID, "fzb_corpus_remove: index " + std::to_string(indices[k]) + " at position " + std::to_string(k) + " is beyond the corpus' " + std::to_string(c->dev.n) + " haystacks");
    EditRequest rq;  // the device form over a copy of the list
    rq.what = "fzb_corpus_remove";
    rq.host_idx = indices;
    rq.max_count = n_indices;
    return edit_run(c, rq);
}

int fzb_corpus_replace(fzb_corpus* c, const uint32_t* indices, size_t n, const uint8_t* bytes, const uint64_t* end_offsets) {
    if (!c || (n && (!indices || !end_offsets))) return fzb_fail(FZB_ERR_INVALID, "null argument");
    const u64 raw = n ? end_offsets[n - 1] : 0;
    if (raw && !bytes) return fzb_fail(FZB_ERR_INVALID, "null argument");
    int rc = grow_begin(c, "fzb_corpus_replace");
    if (rc) return rc;
    if (!n) return FZB_OK;
    for (size_t k = 0; k < n; k++) {
        if (indices[k] >= c->dev.n)
            return fzb_fail(FZB_ERR_INVALID, "fzb_corpus_replace: index " + std::to_string(indices[k]) + " at position " + std::to_string(k) + " is beyond the corpus' " + std::to_string(c->dev.n) + " haystacks");
        if (end_offsets[k] < (k ? end_offsets[k - 1] : 0)) return fzb_fail(FZB_ERR_INVALID, "end_offsets must be non-decreasing");
    }
    // sorted by haystack: the pass finds a touched haystack's batch item by binary search
    std::vector<u32> order(n), sorted_idx(n);
    for (size_t k = 0; k < n; k++) order[k] = (u32)k;
    std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return indices[a] < indices[b]; });
    for (size_t k = 0; k < n; k++) {
        sorted_idx[k] = indices[order[k]];
        if (k && sorted_idx[k] == sorted_idx[k - 1])
            return fzb_fail(FZB_ERR_INVALID, "fzb_corpus_replace: haystack " + std::to_string(sorted_idx[k]) + " is named twice (positions " + std::to_string(std::min(order[k - 1], order[k])) + " and " +
                                                 std::to_string(std::max(order[k - 1], order[k])) + ")");
    }
    // the batch travels as an appended one does: as it is, into the corpus' landing buffers
    hipError_t e = stage_ensure_room(c, n, raw);
    if (e == hipSuccess) e = h2d_all({H2DJob{c->stage_ends, end_offsets, n * 8}, H2DJob{c->stage_raw, bytes, (size_t)raw}}, c->device);
    if (e != hipSuccess) return fzb_fail(FZB_ERR_HIP, std::string("fzb_corpus_replace (host to device): ") + hipGetErrorString(e));
    EditRequest rq;
    rq.what = "fzb_corpus_replace";
    rq.host_idx = sorted_idx.data();
    rq.max_count = n;
    rq.host_rk = order.data();
    rq.batch_h2d = raw + (u64)n * 8;
    return edit_run(c, rq);
}

int fzb_corpus_edit_info(const fzb_corpus* c, uint64_t out[4]) {
    if (!c || !out) return fzb_fail(FZB_ERR_INVALID, "null argument");
    for (int k = 0; k < 4; k++) out[k] = c->edit_info[k];
    return FZB_OK;
}

}  // extern "C"
