// nvbanded_sink.hpp — the sink-tracking forms of the banded scoring kernels (nvbanded.hpp): per
// pair the BestSink score and the cell (x = text, y = pattern, one-based) where nvbio's
// banded_alignment_score<BAND_LEN>(aligner, pattern, quals, text, min_score, sink) leaves it.
//
// BestSink keeps the last maximum in report order (best <= h, sink_inl.h:59-68).  The banded
// score pass reports (sw/sw_banded_inl.h:436, :465, :494-510; gotoh/gotoh_banded_inl.h:642-659):
//   LOCAL        every cell at (i + j + 1, i + 1): rows top to bottom, band slots j = 0 .. B-1
//                inside a row; slots whose text symbol lies past N (read as 255) are reported
//                too, so x may exceed N
//   SEMI_GLOBAL  band[0] at (M, M), then band[j] at (M + j, M) for 1 <= j < m,
//                m = min(M + B - 1, N) - (M - 1) in uint32: the rightmost maximum
//   GLOBAL       band[B-1] once, at (M + B - 1, M)
// A pair with N < M reports nothing: INT32_MIN and (0xFFFFFFFF, 0xFFFFFFFF), as does a LOCAL
// pair with an empty pattern.
//
// The recurrences are nv_banded_kernel's and nv_banded16_kernel's, restated here so that the
// score-only kernels keep their code (as nv16_body.inc does for the full-DP packed kernel).
// GLOBAL and SEMI_GLOBAL add nothing to the row loop: the position is read off the last row.
//
// LOCAL, int32: report order is row-major, so the answer is the last row that holds the maximum
// and the last slot holding it in that row.  Per cell one compare, one max and one select of the
// slot number (a constant) into a row-local register; per row one test of that register.
//
// LOCAL, packed: a key per cell does not fit beside H in 16 bits, so the work is per row.  The
// packed row maximum is formed two cells per v_pk_maximum3 (B/2 per row, where the score-only
// kernel spends B on its running best); per half the row qualifies when its maximum is >= the
// running best (and the row is one of the half's own), and a qualifying row is copied, under a
// per-half mask, into a second band array (one v_bfi per slot, skipped by a wave in which no
// half qualifies).  After the loop the copy holds each half's last qualifying row: the last slot
// equal to the best is found once per pair.  Cost per row: B/2 maxima, about ten scalar-like
// VALU operations for the two tests, and B v_bfi on qualifying rows; B more VGPRs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nvbanded.hpp"

namespace gx {

// a.score may be NULL; sinks: 2 per pair (x, y), may be NULL
struct NvBandSinkArgs { NvBandArgs a; uint32_t *sinks; };
struct NvBand16SinkArgs { NvBand16Args a; uint32_t *sinks; };

template <class Args>
__device__ __forceinline__ void nvb_put(const Args &S, uint32_t pair, int32_t score, uint32_t x, uint32_t y) {
    if (S.a.score) S.a.score[pair] = score;
    if (S.sinks) { S.sinks[2 * pair] = x; S.sinks[2 * pair + 1] = y; }
}

template <int ALN, int TYPE, int BMAX, bool EX = false>
__global__ __launch_bounds__(256) void nv_banded_sink_kernel(NvBandSinkArgs S) {
    const NvBandArgs &A = S.a;
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= A.n) return;
    const uint32_t po = A.poff[tid], M = A.poff[tid + 1] - po;
    const bool shared = A.toff == nullptr;
    const uint32_t to = shared ? 0u : A.toff[tid], N = shared ? A.tlen0 : A.toff[tid + 1] - to;
    int32_t best = INT32_MIN;
    uint32_t bx = 0xFFFFFFFFu, by = 0xFFFFFFFFu;
    const uint32_t B = EX ? (uint32_t)BMAX : A.band;
    if (N < M) { nvb_put(S, tid, best, bx, by); return; }
    constexpr bool GOTOH = ALN == NV_GOTOH;
    const int32_t S_eq = A.match, S_ne = A.mismatch;
    const int32_t Go = A.go, Ge = A.ge, Del = A.del, Ins = A.ins;
    const int32_t infimum = -32768 - max(Go, Ge);
    int32_t H[BMAX], F[BMAX];
    uint32_t tc[BMAX];
    NvSymReader pr, tr;
    pr.init(A.pw, A.pbits, A.pbig, po, M);
    tr.init(A.tw, A.tbits, A.tbig, to, N);
#pragma unroll
    for (int j = 0; j < BMAX; ++j) {
        if (GOTOH) H[j] = j == 0 ? 0 : (TYPE == NV_GLOBAL ? Go + (j - 1) * Ge : 0);
        else H[j] = TYPE == NV_GLOBAL ? j * Del : 0;
        F[j] = infimum;
        tc[j] = 255u;
    }
    uint32_t tnext = 0;
#pragma unroll
    for (int j = 0; j < BMAX - 1; ++j)
        if ((uint32_t)j + 1 < B) { tc[j] = tnext < N ? tr.next() : 255u; ++tnext; }
    for (uint32_t i = 0; i < M; ++i) {
        const uint32_t q = pr.next();
        const uint32_t g_last = tnext < N ? tr.next() : 255u;
        ++tnext;
#pragma unroll
        for (int j = 0; j < BMAX; ++j)
            if ((uint32_t)j + 1 == B) tc[j] = g_last;
        int32_t E = 0, hprev = 0;
        int32_t rj = -1;                                       // LOCAL: the row's last slot with h >= best
#pragma unroll
        for (int j = 0; j < BMAX; ++j) {
            if ((uint32_t)j >= B) break;
            const bool last = (uint32_t)j + 1 == B;
            const int32_t diag = H[j] + (tc[j] == q ? S_eq : S_ne);
            int32_t hi;
            if (GOTOH) {
                if (!last) F[j] = max(F[j + (j + 1 < BMAX ? 1 : 0)] + Ge, H[j + (j + 1 < BMAX ? 1 : 0)] + Go);
                else F[j] = infimum;
                hi = j == 0 ? max(F[0], diag) : last ? max(E, diag) : max(max(F[j], E), diag);
            } else {
                const int32_t top = last ? INT32_MIN / 2 : H[j + (j + 1 < BMAX ? 1 : 0)] + Del;
                hi = j == 0 ? max(top, diag) : max(max(top, hprev + Ins), diag);
            }
            if (TYPE == NV_LOCAL) {
                hi = max(hi, 0);
                rj = hi >= best ? j : rj;
                best = max(best, hi);
            }
            H[j] = hi;
            hprev = hi;
            if (GOTOH) E = j == 0 ? hi + Go : max(hi + Go, E + Ge);
        }
        if (TYPE == NV_LOCAL && rj >= 0) { bx = i + (uint32_t)rj + 1; by = i + 1; }
#pragma unroll
        for (int j = 0; j + 1 < BMAX; ++j)
            if ((uint32_t)j + 1 < B) tc[j] = tc[j + 1];
    }
    if (TYPE == NV_GLOBAL) {
#pragma unroll
        for (int j = 0; j < BMAX; ++j)
            if ((uint32_t)j + 1 == B) best = H[j];
        bx = M + B - 1; by = M;
    } else if (TYPE == NV_SEMI) {
        const uint32_t m = min(M + B - 1, N) - (M - 1);       // uint32 as the reference; >= 1 here
        best = H[0]; bx = M; by = M;
#pragma unroll
        for (int j = 1; j < BMAX; ++j)
            if ((uint32_t)j < B && (uint32_t)j < m && H[j] >= best) { best = H[j]; bx = M + j; }
    }
    nvb_put(S, tid, best, bx, by);
}

// nv_banded16_kernel with the position of each half (nvbanded.hpp describes the arithmetic and
// the host's conditions, batched.hip nvb16_ok).
template <int ALN, int TYPE, int BMAX, bool EX = false>
__global__ __launch_bounds__(256) void nv_banded16_sink_kernel(NvBand16SinkArgs S) {
    const NvBand16Args &A = S.a;
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= A.n_lanes) return;
    constexpr bool GOTOH = ALN == NV_GOTOH, LOCAL = TYPE == NV_LOCAL;
    const bool shared = A.toff == nullptr;
    uint32_t M[2], N[2], po[2], to[2];
    bool valid[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t pr = 2 * lane + h;
        valid[h] = pr < A.n;
        const uint32_t pp = valid[h] ? pr : 2 * lane;
        po[h] = A.poff[pp]; M[h] = A.poff[pp + 1] - po[h];
        to[h] = shared ? 0u : A.toff[pp];
        N[h] = shared ? A.tlen0 : A.toff[pp + 1] - to[h];
    }
    const uint32_t Bn = EX ? (uint32_t)BMAX : A.band;
    const int32_t Bs = (int32_t)A.base;
    const uint32_t BB = A.base * 0x10001u, NEG = 0x04000400u;
    const uint32_t FLOOR = LOCAL ? BB : NEG;
    const uint32_t MIS = (uint32_t)A.mismatch * 0x10001u;
    const uint32_t GO = (uint32_t)(-A.go) * 0x10001u, GE = (uint32_t)(-A.ge) * 0x10001u;   // gaps <= 0
    const uint32_t DEL = (uint32_t)(-A.del) * 0x10001u, INS = (uint32_t)(-A.ins) * 0x10001u;
    const uint32_t dm = (uint32_t)(A.match - A.mismatch);
    uint32_t H[BMAX], F[BMAX], sel[BMAX];
    uint32_t Hs[LOCAL ? BMAX : 1];                             // LOCAL: each half's last qualifying row
    NvSymReader tr[2], prd[2];
    uint32_t tnext[2] = {0u, 0u};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        prd[h].init(A.pw, A.pbits, A.pbig, po[h], M[h]);
        tr[h].init(A.tw, 2u, A.tbig, to[h], N[h]);
    }
    auto next_sel = [&]() {
        uint32_t sa = 0x0Cu, sb = 0x0Cu;
        if (tnext[0] < N[0]) sa = tr[0].next();
        if (tnext[1] < N[1]) sb = tr[1].next() + 4u;
        ++tnext[0]; ++tnext[1];
        return sa | 0x0C00u | (sb << 16) | 0x0C000000u;
    };
#pragma unroll
    for (int j = 0; j < BMAX; ++j) {
        int32_t v;
        if (GOTOH) v = j == 0 ? 0 : (TYPE == NV_GLOBAL ? A.go + (j - 1) * A.ge : 0);
        else v = TYPE == NV_GLOBAL ? j * A.del : 0;
        H[j] = (uint32_t)(v + Bs) * 0x10001u;
        F[j] = FLOOR;
        sel[j] = 0x0C0C0C0Cu;
        if constexpr (LOCAL) Hs[j] = 0u;
    }
#pragma unroll
    for (int j = 0; j < BMAX - 1; ++j)
        if ((uint32_t)j + 1 < Bn) sel[j] = next_sel();
    // per-half results; stored 16-bit values until the end.  have: the half reported a cell
    uint32_t ov[2] = {0u, 0u}, ox[2] = {0u, 0u}, oy[2] = {0u, 0u};
    bool have[2] = {false, false};
    uint32_t best = BB;                                        // LOCAL: packed running best, from 0
    uint32_t brow[2] = {0u, 0u};                               // LOCAL: the last qualifying row
    // GLOBAL / SEMI_GLOBAL: at the half's last row (M == 0: from the row-zero band)
    auto take = [&](int h) {
        uint32_t v = 0, bj = 0;
        if (TYPE == NV_GLOBAL) {
#pragma unroll
            for (int j = 0; j < BMAX; ++j)
                if ((uint32_t)j + 1 == Bn) v = (H[j] >> (16 * h)) & 0xFFFFu;
            bj = Bn - 1;
        } else {
            const uint32_t m = min(M[h] + Bn - 1, N[h]) - (M[h] - 1);   // uint32 as the reference
            v = (H[0] >> (16 * h)) & 0xFFFFu;
#pragma unroll
            for (int j = 1; j < BMAX; ++j) {
                const uint32_t hv = (H[j] >> (16 * h)) & 0xFFFFu;
                if ((uint32_t)j < Bn && (uint32_t)j < m && hv >= v) { v = hv; bj = j; }
            }
        }
        ov[h] = v; ox[h] = M[h] + bj; oy[h] = M[h];
        have[h] = true;
    };
    if (!LOCAL) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (M[h] == 0) take(h);
    }
    const uint32_t Mmax = max(M[0], M[1]);
    for (uint32_t i = 0; i < Mmax; ++i) {
        const uint32_t qa = i < M[0] ? prd[0].next() : 4u, qb = i < M[1] ? prd[1].next() : 4u;
        const uint32_t TA = qa < 4 ? dm << (8 * qa) : 0u, TB = qb < 4 ? dm << (8 * qb) : 0u;
        const uint32_t snew = next_sel();
#pragma unroll
        for (int j = 0; j < BMAX; ++j)
            if ((uint32_t)j + 1 == Bn) sel[j] = snew;
        uint32_t E = 0, hprev = 0;
        uint32_t rm = BB;                                      // LOCAL: the row's packed maximum (h >= 0)
#pragma unroll
        for (int j = 0; j < BMAX; ++j) {
            if ((uint32_t)j >= Bn) break;
            const bool last = (uint32_t)j + 1 == Bn;
            const int jn = j + 1 < BMAX ? j + 1 : j;
            const uint32_t tmp = H[j] + __builtin_amdgcn_perm(TB, TA, sel[j]) + MIS;
            uint32_t hi;
            if (GOTOH) {
                F[j] = last ? NEG : pk_max3(F[jn] - GE, H[jn] - GO, FLOOR);
                if (j == 0) hi = pk_max3(F[0], tmp, LOCAL ? BB : tmp);
                else if (last) hi = pk_max3(E, tmp, LOCAL ? BB : tmp);
                else hi = pk_max3(F[j], E, tmp);
                E = j == 0 ? (LOCAL ? pk_max3(hi - GO, BB, BB) : hi - GO) : pk_max3(hi - GO, E - GE, FLOOR);
            } else {
                if (j == 0) hi = pk_max3(H[jn] - DEL, tmp, tmp);
                else if (last) hi = pk_max3(hprev - INS, tmp, tmp);
                else hi = pk_max3(H[jn] - DEL, hprev - INS, tmp);
                if (LOCAL) hi = pk_max3(hi, BB, BB);
            }
            if (LOCAL) {   // two cells per maximum3: hprev is still slot j - 1's h here
                if (j & 1) rm = pk_max3(rm, hprev, hi);
                else if (last) rm = pk_max3(rm, hi, hi);
            }
            H[j] = hi;
            hprev = hi;
        }
        if constexpr (LOCAL) {
            // per half: rm >= best (the last maximum: ties move the sink) on one of the half's own rows
            const uint32_t below = pk_max3(rm, best, best) ^ rm;   // a zero half: rm >= best
            const uint32_t mask = ((below & 0xFFFFu) == 0 && i < M[0] ? 0x0000FFFFu : 0u) |
                                  ((below >> 16) == 0 && i < M[1] ? 0xFFFF0000u : 0u);
            if (mask) {
                best = (rm & mask) | (best & ~mask);
                if (mask & 0x0000FFFFu) brow[0] = i;
                if (mask & 0xFFFF0000u) brow[1] = i;
#pragma unroll
                for (int j = 0; j < BMAX; ++j)
                    if ((uint32_t)j < Bn) Hs[j] = (H[j] & mask) | (Hs[j] & ~mask);
            }
        }
#pragma unroll
        for (int j = 0; j + 1 < BMAX; ++j)
            if ((uint32_t)j + 1 < Bn) sel[j] = sel[j + 1];
        if (!LOCAL) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (i + 1 == M[h]) take(h);
        }
    }
    if constexpr (LOCAL) {
        // every row holds a cell >= 0 = the initial best, so a half with rows has a qualifying row
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (M[h] == 0) continue;
            const uint32_t v = (best >> (16 * h)) & 0xFFFFu;
            uint32_t bj = 0;
#pragma unroll
            for (int j = 0; j < BMAX; ++j)
                if ((uint32_t)j < Bn && ((Hs[j] >> (16 * h)) & 0xFFFFu) == v) bj = j;
            ov[h] = v; ox[h] = brow[h] + bj + 1; oy[h] = brow[h] + 1;
            have[h] = true;
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (!valid[h]) continue;
        const bool reported = N[h] >= M[h] && have[h];
        nvb_put(S, 2 * lane + h, reported ? (int32_t)ov[h] - Bs : INT32_MIN, reported ? ox[h] : 0xFFFFFFFFu,
                reported ? oy[h] : 0xFFFFFFFFu);
    }
}

}  // namespace gx
