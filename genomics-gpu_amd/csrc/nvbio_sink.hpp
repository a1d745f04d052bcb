// nvbio_sink.hpp — the sink-tracking forms of the nvbio front-end's scoring kernels (nvbio.hpp,
// int32; nvbio16.hpp, two pairs per lane in 16-bit halves): per pair the BestSink score and the cell (x = text, y = pattern) where
// nvbio's alignment_score(aligner, pattern, text, min_score, sink) leaves it.
//
// BestSink keeps the last maximum in report order (best <= h, sink_inl.h:59-68).  The
// TextBlockingTag score functions report (gotoh_inl.h:1075-1092, :1224-1229, :1403-1420;
// sw_inl.h:949-966, :1132-1137, :1192-1209):
//   LOCAL        every cell: text stripes of BAND_LEN columns left to right, inside a stripe
//                the pattern rows top to bottom, inside a row the stripe's columns left to
//                right; columns past N are not reported.  BAND_LEN is 8 for Gotoh
//                (gotoh_bandlen_selector, gotoh_inl.h:1492-1495) and 16 for Smith-Waterman
//                (sw_bandlen_selector, sw_inl.h:1330-1334, instantiated at :1397) and for
//                edit distance, which takes Smith-Waterman's selector (ed_inl.h:95)
//   SEMI_GLOBAL  the last pattern row, stripe by stripe: columns left to right
//   GLOBAL       the one cell (N, M)
// with position (block + j, i + 1): one-based text column x and pattern row y.
//
// LOCAL: the lanes sweep anti-diagonals, not report order, so every cell carries its rank
// in report order,  key(i, c) = (((c >> SB) * M + i) << SB) | (c & (2^SB - 1))  (row i,
// column c, zero-based; SB = log2 BAND_LEN: 3 for Gotoh, 4 for SW and ED), and a lane keeps the lexicographic maximum of (H, key) over its own cells:
// one signed 64-bit compare on (H << 32 | key).  The last maximum in report order is the
// greatest key among the cells that hold the score, whatever the visit order; the lane
// group reduces the 64-bit pair once per pair (ds_bpermute butterflies) and lane 0
// decodes the key.  wavefront16.hpp's strip-major key is the model, with the opposite
// tie rule: GASAL2 keeps the first maximum, nvbio the last.  Pad rows (>= M) and pad
// columns (>= N) are masked out of the maximum: a pad cell may tie with a real one.
// The key stays below 2^32: ((c >> SB) * M + i) < (N / 2^SB + 1) * M, so key < N * M + 2^SB * M;
// texts are bounded by the LDS slot (80 K codes) and patterns by 1024 rows: below
// 2^26.4 + 2^14 at SB = 4 (2^26.4 + 2^13 at SB = 3).
//
// SEMI_GLOBAL: the lane that owns row M - 1 meets its columns in increasing order and
// takes a column when h >= best: the rightmost maximum.  GLOBAL: (N, M).
//
// Pairs that report no cell (an empty text; LOCAL: an empty pattern) keep BestSink's
// INT32_MIN and get the sink (0xFFFFFFFF, 0xFFFFFFFF), as gasalx_nv_traceback_* writes it.
// An empty pattern reports the band initialisation H(-1, c) with y = M = 0.
//
// The packed form (nv16_body) tracks the same per half.  Both halves of a lane sit on the same
// row and column, so one key serves both pairs, built without the pattern length:
// (c >> SB) << (SB + 10) | i << SB | (c & (2^SB - 1)), the same order for rows below 1024 (10
// bits; c >> SB < 2^13 for 80 K columns: 27 bits at SB = 4, 27 at SB = 3).  LOCAL keeps
// H << 32 | key per half (the 16-bit stored score extracted from the packed H) in place of the
// packed running maximum; SEMI_GLOBAL a column per half on the lane that owns the half's last
// row (one shared text: lane G - 1 for both).
//
// nv_sink_kernel includes nv_kernel's own body (nv_body.inc, as wf16_body.inc is shared) with
// SINK set: the int32 recurrences, boundaries, LDS staging and DPP hand-off exist once, and
// nv_kernel (SINK false) keeps its code.  The packed body is a copy (nv16_body.inc says why).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nvbio.hpp"
#include "nvbio16.hpp"

namespace gx {

// a.score / a.score may be NULL, score16 is not written (NULL); sinks: 2 per pair, x = text
// column, y = pattern row, one-based; may be NULL
struct NvSinkArgs { NvArgs a; uint32_t *sinks; };
struct Nv16SinkArgs { Nv16Args a; uint32_t *sinks; };

template <int ALN, int TYPE, int G, int R>
__global__ __launch_bounds__(256) void nv_sink_kernel(NvSinkArgs S) {
    constexpr bool SINK = true, MASK = true;
    const NvArgs &A = S.a;
    uint32_t *const sinks = S.sinks;
#include "nv_body.inc"
}

template <int ALN, int TYPE, int G, int R, bool SHARED>
__global__ __launch_bounds__(256) void nv16_sink_kernel(Nv16SinkArgs S) {
    constexpr bool SINK = true;
    const Nv16Args &A = S.a;
    uint32_t *const sinks = S.sinks;
#include "nv16_body.inc"
}

}  // namespace gx
