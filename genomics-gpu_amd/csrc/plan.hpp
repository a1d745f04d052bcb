// plan.hpp — what the launch code (dispatch.hip) shares with the planner (plan.cpp; make_plan and
// make_semi_cigar_plan: engine.hpp).  Host only: no kernel header.
#pragma once
#include <algorithm>

#include "engine.hpp"
#include "shapes.hpp"

namespace gx {

// The packed kernels' launch arithmetic, each formula written once: the planner, the tail shape,
// the launch and the walk must agree on them, or a packed kernel overflows silently.
// two pairs per group of G lanes
inline uint32_t pairs_per_wave(int G) { return 2 * (64 / G); }
inline uint32_t pairs_per_block(int G) { return kWavesPerBlock * (64 / G) * 2; }
// largest row + column of any cell a G x R launch computes over y8 step-axis positions
inline int64_t packed_span(int G, int R, int64_t y8) { return (int64_t)G * R + y8 + 2 * G + 8; }
// LDS per pair slot: uint2 per position, with the odd-step tail and the prefetch; and per block
inline uint32_t packed_lds_stride(uint32_t y8, int G) { return ((y8 + 2 * G + 4 + 3) & ~3u) * 8; }
inline size_t packed_lds_bytes(uint32_t y8, int G) {
    return (size_t)kWavesPerBlock * (64 / std::max(G, 1)) * packed_lds_stride(y8, G);
}
// band traceback: the window of a lane with R rows and half width w, columns [max(lg*R - w, 0), + R + 2w)
inline uint32_t band_window(int R, uint32_t w) { return ((uint32_t)(R + 2 * w) + 3u) & ~3u; }
// ceil(2^32 / R): the walk's division by R (generic.hpp TbArgs::pk_rmagic)
inline uint32_t rmagic(int R) { return (uint32_t)((0x100000000ull + R - 1) / R); }

// GLOBAL's value window over q8 x t8 padded cells and a span (packed_span): false refuses, true sets
// *vmin (WfArgs::vmin).  The tail shape asks again for its second shape.
bool global_window(const gasalx_params &p, int64_t q8, int64_t t8, int64_t span, int32_t *vmin);

// LOCAL in the e-drift frame (wavefront16.hpp step_local_dr) for a shape G x R over q8 rows and y8
// target columns: values B + H + e(r + c) over the shape's span stay in the window (`window`), the
// top lane's first diagonal B - 2e stays above 0x0400 (`floor`), and the keys H*C + (C-1-c), which
// rank kc = C + G steps (row k's carry e*k more, wf16_body.inc KA0, taken off after the sweep), fit
// f16 patterns (`f16`)
struct LocalDrift {
    int64_t hmax, kc;
    bool window, floor, f16;
};
LocalDrift local_drift_frame(const gasalx_params &p, int64_t q8, int64_t y8, int G, int R);

// The 16-bit prepass launches' stored value of 0 (banded16.hpp, local16.hpp), score of an N cell and table
// offset K = max(0, b, N_PENALTY); the KSW admission and its *kofs (ksw16.hpp; KSW has no plan field)
inline uint32_t band16_base(const gasalx_params &p) { return 0x400u + (uint32_t)(p.gap_open + p.gap_extend + p.mismatch); }
inline int32_t local16_sn(const gasalx_params &p) { return p.has_n_penalty ? -p.n_penalty : 0; }
inline uint32_t local16_k(const gasalx_params &p) { return (uint32_t)std::max({0, p.mismatch, -local16_sn(p)}); }
inline uint32_t local16_base(const gasalx_params &p) { return 0x400u + (uint32_t)(p.gap_open + p.gap_extend) + local16_k(p); }
bool ksw16_ok(const gasalx_params &p, uint32_t max_q, int32_t *kofs);

}  // namespace gx
