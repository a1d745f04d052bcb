// nvmyers.hpp — nvbio's banded Myers bit-vector edit distance, the function behind
// EditDistanceAligner<TYPE, MyersTag<ALPHABET_SIZE>> in BatchedBandedAlignmentScore<BAND_LEN>
// (NvB/nvbio/alignment/myers/myers_banded_inl.h:311-324 enters banded_myers<BAND_LEN, 0, TYPE,
// ALPHABET_SIZE>, :226-288).  One pair per thread; VP, VN and the alphabet's match masks are
// 32-bit registers whose bit BAND_LEN - 1 is the cell on the main diagonal.  Restated exactly,
// with C = 0:
//   :245        a text shorter than its pattern reports nothing (INT32_MIN, the empty sink)
//   :250-253    VP = ~0, VN = 0, dist = 0, every mask 0
//   :261-269    phase 1, last = min(N - 1, M) columns down the diagonal: the masks shift right,
//               pattern[i] enters at bit BAND_LEN - 1, dist -= 1 - D0[BAND_LEN - 1]; no report
//   :272-284    phase 2, columns last .. N - 1 while s >= 0, s = BAND_LEN - 1 + M - last counting
//               down: the masks shift, dist -= HP[s] - HN[s]; SEMI_GLOBAL reports
//               (dist, (i + 1, M)) at every column
//   :285-286    GLOBAL reports (dist, (N, M)) once, after the loop
//   :196-224    the column: X = Eq | VN; D0 = ((VP + (X & VP)) ^ VP) | X; HN = VP & D0;
//               HP = VN | ~(VP | D0); X = D0 >> 1; VN = X & HP; VP = HN | ~(X | HP)
//   :72-194     MyersBitVectors<N>: <2> masks the symbol with 1, <4> with 3; <5>::load ignores
//               symbols above 4 and <5>::get answers B[4] for them
// The sink is a BestSink (sink_inl.h:59-68: `score <= new` keeps the last maximum); min_score is
// the sink type's minimum, so every reached column is reported.  There is no LOCAL form.
// Two points the reference leaves open are settled here:
//   - MyersBitVectors<5>'s constructor zeroes B[0..3] only (:160-164); here B[4] starts at 0.
//   - With N == M phase 2 starts at s = BAND_LEN, which is 32 at BAND_LEN 32: the report bits
//     are HP >> 32 and HN >> 32.  Read as the device code the reference compiles to does
//     (a shift by the register width gives 0): both bits are 0 there.
// All 32 bits of the registers take part at every band length, as in the reference (the carry
// of VP + (X & VP) runs past bit BAND_LEN - 1 and comes back through D0 >> 1).
// pattern[i] is read for i < last <= M and text[i] for i < N, both in order: each string is read
// through an NvSymReader (nvbanded.hpp), one packed word ahead and never past the string's last
// word, so pattern[M] and text[N] are never fetched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nvbanded.hpp"   // NvSymReader

namespace gx {

struct NvMyersArgs {
    const uint32_t *pw, *poff;      // pattern words, n + 1 symbol offsets
    uint32_t pbits, pbig;
    const uint32_t *tw, *toff;      // text words, n + 1 symbol offsets (NULL: one shared text of tlen0)
    uint32_t tbits, tbig, tlen0;
    int32_t *score;                 // BestSink score per pair, or NULL
    uint32_t *sinks;                // sinks[2k] = x (text column), sinks[2k + 1] = y (pattern row), or NULL
    uint32_t n, band;
};

// MyersBitVectors<ALPHABET> (:42-194)
template <int ALPHABET>
struct NvMyersMasks {
    static constexpr int K = ALPHABET == 2 ? 2 : ALPHABET == 4 ? 4 : 5;
    uint32_t B[K];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int c = 0; c < K; ++c) B[c] = 0u;
    }
    // shift() then load(sym, top)
    __device__ __forceinline__ void shift_load(uint32_t sym, uint32_t top) {
        const uint32_t cc = ALPHABET == 2 ? sym & 1u : ALPHABET == 4 ? sym & 3u : sym;
#pragma unroll
        for (int c = 0; c < K; ++c) B[c] = (B[c] >> 1) | (cc == (uint32_t)c ? top : 0u);
    }
    __device__ __forceinline__ void shift() {
#pragma unroll
        for (int c = 0; c < K; ++c) B[c] >>= 1;
    }
    __device__ __forceinline__ uint32_t get(uint32_t sym) const {
        const uint32_t cc = ALPHABET == 2 ? sym & 1u : ALPHABET == 4 ? sym & 3u : min(sym, 4u);
        // an and-or over all K masks: a chain of selects on cc reads to the compiler as B[cc], an
        // indexed load, and it then keeps the array in LDS instead of registers
        uint32_t v = 0u;
#pragma unroll
        for (int c = 0; c < K; ++c) v |= B[c] & (0u - (uint32_t)(cc == (uint32_t)c));
        return v;
    }
};

// the shared column of diagonal_column / horizontal_column (:196-224)
__device__ __forceinline__ void nv_myers_column(uint32_t eq, uint32_t &VP, uint32_t &VN, uint32_t &D0, uint32_t &HP,
                                                uint32_t &HN) {
    uint32_t X = eq | VN;
    D0 = ((VP + (X & VP)) ^ VP) | X;
    HN = VP & D0;
    HP = VN | ~(VP | D0);
    X = D0 >> 1;
    VN = X & HP;
    VP = HN | ~(X | HP);
}

template <int TYPE, int ALPHABET>
__global__ __launch_bounds__(256) void nv_myers_kernel(NvMyersArgs A) {
    static_assert(TYPE == NV_GLOBAL || TYPE == NV_SEMI, "banded_myers has no LOCAL branch");
    static_assert(ALPHABET == 2 || ALPHABET == 4 || ALPHABET == 5, "MyersBitVectors<2 / 4 / 5>");
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= A.n) return;
    const uint32_t po = A.poff[tid], M = A.poff[tid + 1] - po;
    const bool shared = A.toff == nullptr;
    const uint32_t to = shared ? 0u : A.toff[tid], N = shared ? A.tlen0 : A.toff[tid + 1] - to;
    int32_t best = INT32_MIN;                              // BestSink (sink_inl.h:38-40)
    uint32_t bx = 0xFFFFFFFFu, by = 0xFFFFFFFFu;
    if (N >= M) {                                          // :245
        const uint32_t B = A.band, top = 1u << (B - 1);
        NvSymReader pr, tr;
        pr.init(A.pw, A.pbits, A.pbig, po, M);
        tr.init(A.tw, A.tbits, A.tbig, to, N);
        NvMyersMasks<ALPHABET> m;
        m.clear();
        uint32_t VP = 0xFFFFFFFFu, VN = 0u, D0, HP, HN;
        int32_t dist = 0;
        const uint32_t last = min(N - 1u, M);              // :261 (uint32, as the reference)
        for (uint32_t i = 0; i < last; ++i) {
            m.shift_load(pr.next(), top);
            nv_myers_column(m.get(tr.next()), VP, VN, D0, HP, HN);
            dist -= 1 - (int32_t)((D0 >> (B - 1)) & 1u);
        }
        int32_t s = (int32_t)(B - 1u + M - last);          // :272
        for (uint32_t i = last; i < N && s >= 0; ++i, --s) {
            m.shift();
            nv_myers_column(m.get(tr.next()), VP, VN, D0, HP, HN);
            if (s < 32) dist -= (int32_t)((HP >> s) & 1u) - (int32_t)((HN >> s) & 1u);
            if (TYPE == NV_SEMI && best <= dist) { best = dist; bx = i + 1; by = M; }
        }
        if (TYPE == NV_GLOBAL) { best = dist; bx = N; by = M; }
    }
    if (A.score) A.score[tid] = best;
    if (A.sinks) { A.sinks[2 * (size_t)tid] = bx; A.sinks[2 * (size_t)tid + 1] = by; }
}

}  // namespace gx
