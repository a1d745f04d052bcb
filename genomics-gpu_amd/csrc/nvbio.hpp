// nvbio.hpp — scoring kernels behind the second front-end: nvbio's batched
// alignment score (NvB/nvbio/alignment/batched.h:44-87, sw-benchmark.cu:355-443).
//
// Semantics (TextBlockingTag, score only, BestSink):
//   Gotoh  (gotoh/gotoh_inl.h:985-1110 cell update, :1140-1260 + :1395-1420 boundaries
//          and sinks; utils.h:114-135 SimpleGotohScheme):
//     F(i,c) = max(F(i-1,c) + Ge, H(i-1,c) + Go)     E(i,c) = max(E(i,c-1) + Ge, H(i,c-1) + Go)
//     H(i,c) = max3(E, F, H(i-1,c-1) + S(p_i, t_c))   LOCAL: max(H, 0)
//     H(i,-1) = LOCAL ? 0 : Go + Ge*i,  E(i,-1) = LOCAL ? 0 : -inf   (gotoh_inl.h:80-86)
//     H(-1,c) = GLOBAL ? (c >= 0 ? Go + Ge*c : 0) : 0,  F(-1,c) = -inf
//   Smith-Waterman, linear gaps (sw/sw_inl.h:895-970, :1085-1215, utils.h:92-110):
//     H(i,c) = max3(H(i-1,c) + Ins, H(i,c-1) + Del, H(i-1,c-1) + S)   LOCAL: max(H, 0)
//     H(i,-1) = LOCAL ? 0 : Ins*(i+1),  H(-1,c) = GLOBAL ? Del*(c+1) : 0
//   Edit distance = Smith-Waterman with (0, -1, -1, -1) (ed/ed_inl.h:97, ed_utils.h:45-52).
//   S(p, t) = p == t ? match : mismatch.  Sinks (sink_inl.h:59-68, the best score is all
//   that sw-benchmark's stream writes out, sw-benchmark.cu:203-209): LOCAL every cell,
//   SEMI_GLOBAL the last pattern row, GLOBAL H(M-1, N-1).
//
// Layout: the pattern is the register axis (G lanes per pair, R rows per lane),
// the text the step axis, staged in LDS as 16-bit codes (pads never match: pattern
// pad 0xFFFE, text pad 0xFFFF); one text per block when every pair shares it (the
// sw-benchmark case: all reads against one reference).  int32 arithmetic; the host
// bounds |values| so the -inf stand-in never wins, as nvbio's infimum never does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gx {

enum NvAligner { NV_ED = 0, NV_SW = 1, NV_GOTOH = 2 };
enum NvType { NV_GLOBAL = 0, NV_LOCAL = 1, NV_SEMI = 2 };   // nvbio AlignmentType order (alignment_base.h:54)

struct NvArgs {
    const uint32_t *pw, *poff;      // pattern words, n + 1 symbol offsets
    uint32_t pbits, pbig;
    const uint32_t *tw, *toff;      // text words, n + 1 symbol offsets (NULL: one shared text of tlen0)
    uint32_t tbits, tbig, tlen0;
    int32_t *score;
    int16_t *score16;
    uint32_t n;
    int32_t match, mismatch, go, ge, del, ins;
    uint32_t lds_stride;            // 16-bit codes per text slot (>= padded max text + G)
};

constexpr int32_t kNvInf = -(1 << 29);

__device__ __forceinline__ uint32_t nv_symbol(const uint32_t *w, uint32_t bits, uint32_t big, uint32_t s) {
    if (bits == 8) return (w[s >> 2] >> (big ? 24 - 8 * (s & 3) : 8 * (s & 3))) & 0xFFu;
    const uint32_t per = 32u / bits, p = s % per;
    const uint32_t sh = big ? 32u - bits * (p + 1) : bits * p;
    return (w[s / per] >> sh) & ((1u << bits) - 1u);
}

__device__ __forceinline__ int32_t nv_shr(int32_t v) {   // lane i <- lane i-1 (DPP wave_shr:1)
    return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xF, 0xF, false);
}

template <int ALN, int TYPE, int G, int R, bool MASK>
__global__ __launch_bounds__(256) void nv_kernel(NvArgs A) {
    constexpr bool SINK = false;   // the sink-tracking instances: nvbio_sink.hpp
    uint32_t *const sinks = nullptr;
#include "nv_body.inc"
}

}  // namespace gx
