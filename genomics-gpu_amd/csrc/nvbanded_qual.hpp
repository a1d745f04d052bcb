// nvbanded_qual.hpp — the banded Gotoh kernels under a quality-aware scheme: what nvBowtie's
// aligners run, GotohAligner over SmithWatermanScoringScheme<QualCost, ConstantCost>
// (NvB/nvBowtie/bowtie2/cuda/scoring.h:203-346), whose substitution(r_i, q_j, r, q, qq) is
// r == q ? m_match(qq) : -m_mmp(qq) (:289).  The reference's banded Gotoh reads the quality of
// the pattern symbol once per row (gotoh/gotoh_banded_inl.h:470) and hands it to the scheme in
// every cell of that row (:492, :544, :591), so here the two kernel-wide constants S_eq / S_ne of
// nv_banded_sink_kernel and nv_banded_traceback_kernel become two per-row values: per row one
// quality byte and one table read, and a cell loop that does not change.
//
// The three kernels restate nvbanded_sink.hpp's two scorers and nvtrace.hpp's banded traceback
// for the Gotoh aligner, the way nvbanded_sink.hpp restates nvbanded.hpp: the existing kernels
// keep their code and instances.  What differs:
//   * The table.  match[l] and mismatch[l] travel by value in the kernel arguments as one word per
//     quality byte (match in the low, mismatch in the high 16 bits; the host fills entries >=
//     levels with entry levels - 1, so the byte indexes the table as it is) and every block copies
//     the 256 words to LDS once, thread t word t.  A row reads one word by its quality byte.
//   * The barrier.  Every thread of a block stages its word and reaches the barrier; threads past
//     the batch and pairs that report nothing leave after it.
//   * Quality bytes are read along the pattern a 32-bit word at a time (NvQualReader, as
//     NvSymReader reads 8-bit symbols), from the aligned word holding byte offsets[k] on: pattern
//     offsets need not be multiples of 4.
//   * Packed kernel: the halves of a lane carry different rows, so dm = match - mismatch is per
//     half (a byte in each half's selector table) and the mismatch addend is built per row as
//     (uint32)mis_lo + ((uint32)mis_hi << 16) from the sign-extended values: the 32-bit sum of two
//     sign-extended halves, as (uint32)mismatch * 0x10001u is, so the low half's sign bits cancel
//     the carry its addition sends into the high half.  A half past its last row adds nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nvbanded_sink.hpp"
#include "nvtrace.hpp"

namespace gx {

constexpr uint32_t kNvQualLevels = 256;

// tab[b]: the scores of a row whose quality byte is b
struct NvQualTable { uint32_t tab[kNvQualLevels]; };
struct NvBandQualArgs { NvBandSinkArgs s; const uint8_t *quals; NvQualTable q; };
struct NvBand16QualArgs { NvBand16SinkArgs s; const uint8_t *quals; NvQualTable q; };
struct NvBandTbQualArgs { NvBandTbArgs t; const uint8_t *quals; NvQualTable q; };

// sequential reader of the quality bytes quals[off .. off + len), one aligned word ahead
// (never past the word holding the last byte)
struct NvQualReader {
    const uint32_t *w;
    uint32_t word, lastw, cur, nxt, p;
    __device__ __forceinline__ void init(const uint8_t *quals, uint32_t off, uint32_t len) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(quals) + off;
        w = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
        p = (uint32_t)(a & 3u);
        word = 0;
        lastw = len ? (p + len - 1) / 4 : 0u;
        cur = len ? w[0] : 0u;
        nxt = len && 1 <= lastw ? w[1] : 0u;
    }
    __device__ __forceinline__ uint32_t next() {
        const uint32_t b = (cur >> (8u * p)) & 255u;
        if (++p == 4) {
            p = 0; ++word; cur = nxt;
            nxt = word + 1 <= lastw ? w[word + 1] : 0u;
        }
        return b;
    }
};

__device__ __forceinline__ int32_t nvq_match(uint32_t e) { return (int32_t)(int16_t)(e & 0xFFFFu); }
__device__ __forceinline__ int32_t nvq_mismatch(uint32_t e) { return (int32_t)e >> 16; }

// nv_banded_sink_kernel<NV_GOTOH> with per-row S_eq / S_ne
template <int TYPE, int BMAX, bool EX = false>
__global__ __launch_bounds__(256) void nv_banded_qual_sink_kernel(NvBandQualArgs Q) {
    __shared__ uint32_t qtab[kNvQualLevels];
    qtab[threadIdx.x] = Q.q.tab[threadIdx.x];
    __syncthreads();
    const NvBandSinkArgs &S = Q.s;
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
    const int32_t Go = A.go, Ge = A.ge;
    const int32_t infimum = -32768 - max(Go, Ge);
    int32_t H[BMAX], F[BMAX];
    uint32_t tc[BMAX];
    NvSymReader pr, tr;
    NvQualReader qr;
    pr.init(A.pw, A.pbits, A.pbig, po, M);
    tr.init(A.tw, A.tbits, A.tbig, to, N);
    qr.init(Q.quals, po, M);
#pragma unroll
    for (int j = 0; j < BMAX; ++j) {
        H[j] = j == 0 ? 0 : (TYPE == NV_GLOBAL ? Go + (j - 1) * Ge : 0);
        F[j] = infimum;
        tc[j] = 255u;
    }
    uint32_t tnext = 0;
#pragma unroll
    for (int j = 0; j < BMAX - 1; ++j)
        if ((uint32_t)j + 1 < B) { tc[j] = tnext < N ? tr.next() : 255u; ++tnext; }
    for (uint32_t i = 0; i < M; ++i) {
        const uint32_t q = pr.next();
        const uint32_t e = qtab[qr.next()];                    // the row's scores (gotoh_banded_inl.h:470)
        const int32_t S_eq = nvq_match(e), S_ne = nvq_mismatch(e);
        const uint32_t g_last = tnext < N ? tr.next() : 255u;
        ++tnext;
#pragma unroll
        for (int j = 0; j < BMAX; ++j)
            if ((uint32_t)j + 1 == B) tc[j] = g_last;
        int32_t E = 0;
        int32_t rj = -1;                                       // LOCAL: the row's last slot with h >= best
#pragma unroll
        for (int j = 0; j < BMAX; ++j) {
            if ((uint32_t)j >= B) break;
            const bool last = (uint32_t)j + 1 == B;
            const int32_t diag = H[j] + (tc[j] == q ? S_eq : S_ne);
            if (!last) F[j] = max(F[j + (j + 1 < BMAX ? 1 : 0)] + Ge, H[j + (j + 1 < BMAX ? 1 : 0)] + Go);
            else F[j] = infimum;
            int32_t hi = j == 0 ? max(F[0], diag) : last ? max(E, diag) : max(max(F[j], E), diag);
            if (TYPE == NV_LOCAL) {
                hi = max(hi, 0);
                rj = hi >= best ? j : rj;
                best = max(best, hi);
            }
            H[j] = hi;
            E = j == 0 ? hi + Go : max(hi + Go, E + Ge);
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

// nv_banded16_sink_kernel<NV_GOTOH> with per-row, per-half dm and mismatch addend (the host's
// conditions: batched.hip nvq16_ok)
template <int TYPE, int BMAX, bool EX = false>
__global__ __launch_bounds__(256) void nv_banded16_qual_sink_kernel(NvBand16QualArgs Q) {
    __shared__ uint32_t qtab[kNvQualLevels];
    qtab[threadIdx.x] = Q.q.tab[threadIdx.x];
    __syncthreads();
    const NvBand16SinkArgs &S = Q.s;
    const NvBand16Args &A = S.a;
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= A.n_lanes) return;
    constexpr bool LOCAL = TYPE == NV_LOCAL;
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
    const uint32_t GO = (uint32_t)(-A.go) * 0x10001u, GE = (uint32_t)(-A.ge) * 0x10001u;   // gaps <= 0
    uint32_t H[BMAX], F[BMAX], sel[BMAX];
    uint32_t Hs[LOCAL ? BMAX : 1];                             // LOCAL: each half's last qualifying row
    NvSymReader tr[2], prd[2];
    NvQualReader qrd[2];
    uint32_t tnext[2] = {0u, 0u};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        prd[h].init(A.pw, A.pbits, A.pbig, po[h], M[h]);
        tr[h].init(A.tw, 2u, A.tbig, to[h], N[h]);
        qrd[h].init(Q.quals, po[h], M[h]);
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
        const int32_t v = j == 0 ? 0 : (TYPE == NV_GLOBAL ? A.go + (j - 1) * A.ge : 0);
        H[j] = (uint32_t)(v + Bs) * 0x10001u;
        F[j] = FLOOR;
        sel[j] = 0x0C0C0C0Cu;
        if constexpr (LOCAL) Hs[j] = 0u;
    }
#pragma unroll
    for (int j = 0; j < BMAX - 1; ++j)
        if ((uint32_t)j + 1 < Bn) sel[j] = next_sel();
    uint32_t ov[2] = {0u, 0u}, ox[2] = {0u, 0u}, oy[2] = {0u, 0u};
    bool have[2] = {false, false};
    uint32_t best = BB;                                        // LOCAL: packed running best, from 0
    uint32_t brow[2] = {0u, 0u};                               // LOCAL: the last qualifying row
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
        const bool ra = i < M[0], rb = i < M[1];
        const uint32_t qa = ra ? prd[0].next() : 4u, qb = rb ? prd[1].next() : 4u;
        // the halves' own rows: dm in a byte, the mismatch sign-extended; a half past its rows adds 0
        const uint32_t ea = ra ? qtab[qrd[0].next()] : 0u, eb = rb ? qtab[qrd[1].next()] : 0u;
        const uint32_t dma = (uint32_t)(nvq_match(ea) - nvq_mismatch(ea)), dmb = (uint32_t)(nvq_match(eb) - nvq_mismatch(eb));
        const uint32_t MIS = (uint32_t)nvq_mismatch(ea) + ((uint32_t)nvq_mismatch(eb) << 16);
        const uint32_t TA = qa < 4 ? dma << (8 * qa) : 0u, TB = qb < 4 ? dmb << (8 * qb) : 0u;
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
            F[j] = last ? NEG : pk_max3(F[jn] - GE, H[jn] - GO, FLOOR);
            if (j == 0) hi = pk_max3(F[0], tmp, LOCAL ? BB : tmp);
            else if (last) hi = pk_max3(E, tmp, LOCAL ? BB : tmp);
            else hi = pk_max3(F[j], E, tmp);
            E = j == 0 ? (LOCAL ? pk_max3(hi - GO, BB, BB) : hi - GO) : pk_max3(hi - GO, E - GE, FLOOR);
            if (LOCAL) {   // two cells per maximum3: hprev is still slot j - 1's h here
                if (j & 1) rm = pk_max3(rm, hprev, hi);
                else if (last) rm = pk_max3(rm, hi, hi);
            }
            H[j] = hi;
            hprev = hi;
        }
        if constexpr (LOCAL) {
            const uint32_t below = pk_max3(rm, best, best) ^ rm;   // a zero half: rm >= best
            const uint32_t mask = ((below & 0xFFFFu) == 0 && ra ? 0x0000FFFFu : 0u) |
                                  ((below >> 16) == 0 && rb ? 0xFFFF0000u : 0u);
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

// nv_banded_traceback_kernel<GOTOH> with per-row S_eq / S_ne; the walk reads flags only and is
// nvtrace.hpp's
template <int TYPE, int BMAX, bool EX = false>
__global__ __launch_bounds__(256) void nv_banded_qual_traceback_kernel(NvBandTbQualArgs Q) {
    __shared__ uint32_t qtab[kNvQualLevels];
    qtab[threadIdx.x] = Q.q.tab[threadIdx.x];
    __syncthreads();
    const NvBandTbArgs &A = Q.t;
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n) return;
    constexpr uint32_t SUB = 0, INS = 1, DEL = 2, SNK = 3, INS_EXT = 4, DEL_EXT = 8;
    const uint32_t po = A.poff[k], M = A.poff[k + 1] - po;
    const bool shared = A.toff == nullptr;
    const uint32_t to = shared ? 0u : A.toff[k], N = shared ? A.tlen0 : A.toff[k + 1] - to;
    const uint32_t B = EX ? (uint32_t)BMAX : A.band, n = A.n;
    const uint32_t words = EX ? (uint32_t)(BMAX + 3) / 4 : A.words;
    uint32_t *src = A.src + 2 * (size_t)k, *snk = A.snk + 2 * (size_t)k;
    src[0] = src[1] = snk[0] = snk[1] = 0xFFFFFFFFu;
    A.n_ops[k] = 0;
    if (N < M || M > A.max_m || 2 * M + B > A.ops_stride) { A.score[k] = INT32_MIN; return; }
    const int32_t Go = A.go, Ge = A.ge;
    const int32_t infimum = -32768 - max(Go, Ge);   // gotoh_banded_inl.h:446-448
    int32_t H[BMAX], F[BMAX];
    uint32_t tc[BMAX];
    NvSymReader pr, tr;
    NvQualReader qr;
    pr.init(A.pw, A.pbits, A.pbig, po, M);
    tr.init(A.tw, A.tbits, A.tbig, to, N);
    qr.init(Q.quals, po, M);
#pragma unroll
    for (int j = 0; j < BMAX; ++j) {
        H[j] = j == 0 ? 0 : (TYPE == 0 ? Go + (j - 1) * Ge : 0);
        F[j] = infimum;
        tc[j] = 255u;
    }
    uint32_t tnext = 0;
#pragma unroll
    for (int j = 0; j < BMAX - 1; ++j)
        if ((uint32_t)j + 1 < B) { tc[j] = tnext < N ? tr.next() : 255u; ++tnext; }
    int32_t best = INT32_MIN;
    uint32_t bx = 0xFFFFFFFFu, by = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < M; ++i) {
        const uint32_t q = pr.next();
        const uint32_t e = qtab[qr.next()];                    // the row's scores (gotoh_banded_inl.h:470)
        const int32_t S_eq = nvq_match(e), S_ne = nvq_mismatch(e);
        const uint32_t g_last = tnext < N ? tr.next() : 255u;
        ++tnext;
#pragma unroll
        for (int j = 0; j < BMAX; ++j)
            if ((uint32_t)j + 1 == B) tc[j] = g_last;
        int32_t E = 0;
        uint32_t edir = SUB;
        uint32_t fw[(BMAX + 3) / 4];
#pragma unroll
        for (int w = 0; w < (BMAX + 3) / 4; ++w) fw[w] = 0;
#pragma unroll
        for (int j = 0; j < BMAX; ++j) {
            if ((uint32_t)j >= B) continue;   // (not break: the loop must unroll fully)
            const bool last = (uint32_t)j + 1 == B;
            const int jn = j + 1 < BMAX ? j + 1 : j;
            const int32_t diag = H[j] + (tc[j] == q ? S_eq : S_ne);
            int32_t hi;
            uint32_t fdir = SUB;
            if (!last) {
                const int32_t ftop = F[jn] + Ge, htop = H[jn] + Go;
                F[j] = max(ftop, htop);
                fdir = ftop > htop ? DEL_EXT : SUB;
            } else {
                F[j] = infimum;
            }
            uint32_t hdir;
            if (j == 0) { hi = max(F[0], diag); hdir = F[0] > diag ? INS : SUB; }
            else if (!last) { hi = max(max(F[j], E), diag); hdir = F[j] > E ? (F[j] > diag ? INS : SUB) : (E > diag ? DEL : SUB); }
            else { hi = max(E, diag); hdir = E > diag ? DEL : SUB; }
            if (TYPE == 1) {
                hi = max(hi, 0);
                if (hi == 0) hdir = SNK;
                if (best <= hi) { best = hi; bx = i + j + 1; by = i + 1; }
            }
            const uint32_t d = hdir | (j == 0 ? SUB : edir) | fdir;
            H[j] = hi;
            if (j == 0) { E = hi + Go; edir = SUB; }
            else {
                const int32_t eleft = E + Ge, ediag = hi + Go;
                edir = eleft > ediag ? INS_EXT : SUB;
                E = max(ediag, eleft);
            }
            fw[j / 4] |= d << (8 * (j % 4));
        }
#pragma unroll
        for (int w = 0; w < (BMAX + 3) / 4; ++w)
            if ((uint32_t)w < words) A.dir[((size_t)i * words + w) * n + k] = fw[w];
#pragma unroll
        for (int j = 0; j + 1 < BMAX; ++j)
            if ((uint32_t)j + 1 < B) tc[j] = tc[j + 1];
    }
    if (TYPE == 0) {
#pragma unroll
        for (int j = 0; j < BMAX; ++j)
            if ((uint32_t)j + 1 == B && best <= H[j]) { best = H[j]; bx = M + B - 1; by = M; }
    } else if (TYPE == 2) {
        const uint32_t m = min(M + B - 1, N) - (M - 1u);
#pragma unroll
        for (int j = 0; j < BMAX; ++j)
            if ((uint32_t)j < B && (j == 0 || (uint32_t)j < m) && best <= H[j]) { best = H[j]; bx = M + j; by = M; }
    }
    A.score[k] = best;
    snk[0] = bx; snk[1] = by;
    if (bx == 0xFFFFFFFFu || by == 0xFFFFFFFFu) return;
    // the walk of nv_banded_traceback_kernel: flags P rows at a time
    constexpr int P = 8, WW = (BMAX + 3) / 4;
    uint32_t held[P][WW];
    NvPushes out(A.ops + (size_t)k * A.ops_stride);
    int32_t e = (int32_t)(bx - by), row = (int32_t)by - 1;
    int32_t base = 0x7FFFFFFF;   // rows [base, base + P) held (none yet)
    int state = 0;   // H / E / F
    bool found = false;
    while (row >= 0) {
        if (__any(row < base)) {
            base = max(row - (P - 1), 0);
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int w = 0; w < WW; ++w)
                    if ((uint32_t)w < words)
                        held[p][w] = base + p <= row ? A.dir[((size_t)(base + p) * words + w) * n + k] : 0u;
        }
        const int32_t rr = row - base;
        uint32_t rowv[WW];
#pragma unroll
        for (int w = 0; w < WW; ++w) {
            rowv[w] = held[0][w];
#pragma unroll
            for (int p = 1; p < P; ++p) rowv[w] = rr == p ? held[p][w] : rowv[w];
        }
        const uint32_t wi = (uint32_t)e >> 2;
        uint32_t word = rowv[0];
#pragma unroll
        for (int w = 1; w < WW; ++w) word = wi == (uint32_t)w ? rowv[w] : word;
        const uint8_t op = (uint8_t)(word >> (8u * ((uint32_t)e & 3u)));
        const uint8_t h_op = op & 3u;
        if (TYPE == 1 && state == 0 && h_op == SNK) { found = true; break; }
        if (state == 1) {
            if ((op & INS_EXT) == 0) state = 0;
            --e; out.push(DEL);
        } else if (state == 2) {
            if ((op & DEL_EXT) == 0) state = 0;
            ++e; --row; out.push(INS);
        } else if (h_op == DEL) {
            state = 1;
        } else if (h_op == INS) {
            state = 2;
        } else {
            --row; out.push(SUB);
        }
    }
    out.flush();
    const uint32_t sy = found ? (uint32_t)row + 1 : 0u;
    src[0] = (uint32_t)e + sy; src[1] = sy;
    A.n_ops[k] = out.cnt;
}

}  // namespace gx
