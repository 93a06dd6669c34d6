// TEST INFRASTRUCTURE: frizbee_amd/csrc/trace_walk.h - the walk back through the score / match matrices that lane 0 of the traced scorer
// (k2c_generic<.., TRACE = true>, kernels_generic.hip) runs - compiled for the host.  tw_walk takes one wave's cells slot in the kernel's
// layout ((rows + 1) x TRACE_W dwords, score | match bit << 16, column c = window byte c - swl), finds the first column of the last row
// that holds the score with a plain scan (the kernel: one ballot per chunk) and hands the rest to the header's walk.
// tests/test_trace_walk_host.py fills the cells from the second transcription's matrices and compares with the oracle's walk.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trace_walk.h"

namespace {

template <bool UNICODE, int SWL>
int walk(const uint32_t* cells, uint32_t rows, uint32_t nchunks, uint32_t score, int max_typos, const uint8_t* th, uint32_t m, uint32_t sp, const uint8_t* ulen,
         uint32_t* posv, uint32_t stride) {
    uint32_t col = 0xFFFFFFFFu;
    for (uint32_t c = SWL; c < (nchunks + 1) * SWL && col == 0xFFFFFFFFu; c++)
        if ((cells[(size_t)rows * TRACE_W + c] & 0xFFFFu) == score) col = c;
    if (col == 0xFFFFFFFFu) return -1;
    auto cell = [&](uint32_t r, uint32_t c) -> uint32_t {
        if (r == 0 || c < (uint32_t)SWL) return 0u;  // row 0 and the zero chunk
        return cells[(size_t)r * TRACE_W + c];
    };
    return (int)trace_walk<UNICODE, SWL>(cell, rows, col, score, max_typos, th, m, sp, ulen, posv, stride);
}

}  // namespace

extern "C" {

int tw_trace_w() { return TRACE_W; }

// -> positions written (<= stride), -1: no column of the last row holds `score`, -2: unsupported lane count.  score != 0, as in the kernel.
int tw_walk(const uint32_t* cells, uint32_t rows, uint32_t nchunks, int swl, int unicode, uint32_t score, int max_typos, const uint8_t* th, uint32_t m, uint32_t sp,
            const uint8_t* ulen, uint32_t* posv, uint32_t stride) {
#define TW(U, L) return walk<U, L>(cells, rows, nchunks, score, max_typos, th, m, sp, ulen, posv, stride)
#define TW_U(L) do { if (unicode) TW(true, L); else TW(false, L); } while (0)
    switch (swl) {
        case 64: TW_U(64);
        case 32: TW_U(32);
        case 16: TW_U(16);
        case 8: TW_U(8);
        default: return -2;
    }
#undef TW_U
#undef TW
}

}  // extern "C"
