// The matched-indices walk: AlignmentPathIter (src/smith_waterman/alignment_iter.rs:108-181) over the score / match matrices the traced
// scorer left behind, collecting what score_haystack[_unicode]_indices collect (src/smith_waterman/algo/mod.rs:49-152) - as a plain
// function for the device AND the host (lane 0 of k2c_generic<.., TRACE = true> calls it with an agent-scope load as `cell`;
// tests/kernel_host/trace_host.cpp compiles it for the CPU over a flat cells array and tests/test_trace_walk_host.py holds it to the
// oracle's walk).  Every decision of the walk - the tie-breaks between the diagonal, left and up moves, the typo count and its budget,
// the step over continuation bytes, one run of positions per matched scalar - is in here; the search for the starting column (first
// column of the last row that holds the score, alignment_iter.rs:52-66) is the caller's: the kernel does it with a ballot per chunk.
#pragma once
#include "fzb_internal.h"

#define TRACE_W (FZB_MAX_HAYSTACK_LEN + 2 * 64)  // columns of a cells row: the zero chunk + up to 1024 bytes rounded up to a chunk

// cell(r, c) -> score | match bit << 16 of needle row r (1-based) at column c; column c holds window byte c - SWL (columns below SWL are
// the zero chunk).  The accessor returns 0 for row 0 and for the zero chunk.
// (rows, col, score): where the walk starts.  mt: max_typos, < 0 = None.  th[0 .. m): the trimmed haystack, sp: its offset in the
// haystack (positions are reported in haystack bytes).  ulen[r - 1]: UTF-8 length of needle scalar r (UNICODE only).
// Writes at most `stride` positions to posv, in walk (= reverse) order; returns how many.
template <bool UNICODE, int SWL, typename Cell>
__device__ __forceinline__ u32 trace_walk(Cell cell, u32 rows, u32 col, u32 score, int mt, const u8* th, u32 m, u32 sp, const u8* ulen, u32* posv, u32 stride) {
    u32 npos = 0;
    u32 r = rows, typos = 0, sc = score, prev = 0xFFFFFFFFu;
    for (;;) {
        if (r == 0) break;
        if (mt >= 0 && typos > (u32)mt) break;
        if (col < (u32)SWL || sc == 0) break;  // at the left edge (only moves up remain) or lost the alignment
        const u32 hidx = col - SWL;
        if (UNICODE && hidx < m && (th[hidx] & 0xC0) == 0x80) {  // continuation byte: walk left
            col--;
            sc = cell(r, col) & 0xFFFFu;
            continue;
        }
        if (cell(r, col) >> 16) {
            const u32 p = hidx + sp;
            if (UNICODE) {
                if (prev != p) {
                    for (int off = (int)ulen[r - 1] - 1; off >= 0; off--)
                        if (npos < stride) posv[npos++] = p + (u32)off;
                    prev = p;
                }
            } else if (npos < stride) {
                posv[npos++] = p;
            }
            r--;
            col--;
            sc = cell(r, col) & 0xFFFFu;
            continue;
        }
        const u32 dg = cell(r - 1, col - 1) & 0xFFFFu, lf = cell(r, col - 1) & 0xFFFFu, upv = cell(r - 1, col) & 0xFFFFu;
        if (dg >= lf && dg >= upv) { r--; col--; typos++; sc = dg; }
        else if (lf >= upv) { col--; sc = lf; }
        else { typos++; r--; sc = upv; }
    }
    return npos;
}
