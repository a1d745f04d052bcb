// nvmatrix.hpp — the nvbio front-end's Gotoh kernels with a substitution matrix: what
// GotohAligner runs when its scheme answers substitution(i, j, r, q, qq) from a table
// (NvB/nvbio/alignment/gotoh/gotoh_inl.h:534, :1042; the proteinsw example's BlosumScheme,
// m_matrix[r + q*24] with r the text symbol and q the pattern symbol).  Score only, or score and
// BestSink position in the TextBlockingTag report order with nvbio_sink.hpp's key at Gotoh's
// stripe width (8 columns, SB = 3).
//
// nv_kernel's layout and recurrences (nvbio.hpp: G lanes per pair, R pattern rows per lane, the
// text on the step axis, int32, DPP hand-off); what differs is where S comes from:
//   * The table form.  The n x n table travels by value in the kernel arguments as a 32 x 32 image
//     (row = pattern symbol, column = text symbol, 1 KB) and every block copies it to the head of
//     its LDS once; a cell reads one byte, tab[32 * p + t].  The lane keeps 32 * p of its rows in
//     registers and the text slot holds t, so a cell's address is one add.  No cell loads from
//     global memory.  (A per-pair query profile would read R scores per step with one wide load,
//     but takes n * G * R bytes of LDS per pair: 96 KB per block at proteinsw's shape, beside the
//     text slots.)
//   * The clamp.  Symbols come from caller memory: a symbol >= n is read as n - 1 before any
//     address is formed (the reference indexes past its table there), so no LDS index leaves the
//     n x n corner of the image.
//   * Pads.  Pad rows (>= M) and pad columns (>= N) carry symbol 0, a real one: with a table
//     there is no code that "never matches".  LOCAL therefore masks them out of the maximum in
//     both forms, as nv_kernel's SINK path does; GLOBAL and SEMI_GLOBAL read row M - 1 at real
//     columns only, and a real cell never depends on a pad cell (pads lie right of and below it).
//   * The text slot holds 8-bit codes (symbols < 32): one byte per column.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nvbio.hpp"

namespace gx {

constexpr uint32_t kNvMatrixDim = 32;                                  // rows and columns of the image
constexpr uint32_t kNvMatrixBytes = kNvMatrixDim * kNvMatrixDim;       // its bytes, the head of the LDS

struct NvMatrixArgs {
    const uint32_t *pw, *poff;      // the string sets, as NvArgs
    uint32_t pbits, pbig;
    const uint32_t *tw, *toff;
    uint32_t tbits, tbig, tlen0;
    int32_t *score;                 // may be NULL
    uint32_t *sinks;                // SINK: 2 per pair, may be NULL
    uint32_t n;
    int32_t go, ge;
    uint32_t lds_stride;            // 8-bit codes per text slot (the padded max text)
    uint32_t nsym;                  // n: symbols are clamped to n - 1
    uint32_t tab[kNvMatrixBytes / 4];   // int8 image, tab[32 * p + t]
};

template <int TYPE, int G, int R, bool SINK>
__global__ __launch_bounds__(256) void nv_matrix_kernel(NvMatrixArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t nvmlds[];
    constexpr int P = 64 / G;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t lg = lane & (G - 1), slot = lane / G;
    const uint32_t pair = (blockIdx.x * 4 + wave) * P + slot;
    const bool valid = pair < A.n;
    const bool shared_text = A.toff == nullptr;
    uint32_t M = 0, N = 0, po = 0, to = 0;
    if (valid) {
        po = A.poff[pair]; M = A.poff[pair + 1] - po;
        if (shared_text) N = A.tlen0;
        else { to = A.toff[pair]; N = A.toff[pair + 1] - to; }
    }
    const uint32_t stride = A.lds_stride, top = A.nsym - 1;
    // ---- the table (256 threads, 256 words), then the text codes (one copy per block when shared) ----
    reinterpret_cast<uint32_t *>(nvmlds)[threadIdx.x] = A.tab[threadIdx.x];
    const int8_t *const tab = reinterpret_cast<const int8_t *>(nvmlds);
    uint8_t *const text = nvmlds + kNvMatrixBytes;
    const uint8_t *mine;
    if (shared_text) {
        for (uint32_t i = threadIdx.x; i < stride; i += blockDim.x)
            text[i] = i < A.tlen0 ? (uint8_t)min(nv_symbol(A.tw, A.tbits, A.tbig, i), top) : (uint8_t)0;
        mine = text;
    } else {
        uint8_t *wl = text + (size_t)wave * P * stride;
        for (uint32_t ps = 0; ps < (uint32_t)P; ps++) {   // uniform trip counts: shuffles see all lanes
            const uint32_t pN = __shfl(N, ps * G), pto = __shfl(to, ps * G);
            for (uint32_t i = lane; i < stride; i += 64)
                wl[ps * stride + i] = i < pN ? (uint8_t)min(nv_symbol(A.tw, A.tbits, A.tbig, pto + i), top) : (uint8_t)0;
        }
        mine = wl + slot * stride;
    }
    __syncthreads();

    // ---- the lane's pattern rows: 32 * symbol, the row of the image ----
    const uint32_t r0 = lg * R;
    const uint32_t nrow = M > r0 ? min(M - r0, (uint32_t)R) : 0u;   // real rows of this lane
    uint32_t pc[R];
    int32_t Hk[R], Ek[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const uint32_t r = r0 + k;
        pc[k] = (valid && r < M) ? min(nv_symbol(A.pw, A.pbits, A.pbig, po + r), top) * kNvMatrixDim : 0u;
        Hk[k] = TYPE == NV_LOCAL ? 0 : A.go + A.ge * (int32_t)r;
        Ek[k] = TYPE == NV_LOCAL ? 0 : kNvInf;
    }
    uint32_t nmax = N;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) nmax = max(nmax, (uint32_t)__shfl_xor(nmax, m));
    const uint32_t nsteps = nmax + G - 1;
    const uint32_t last_lane = M ? (M - 1) / R : 0, last_k = M ? (M - 1) - last_lane * R : 0;
    int32_t best = INT32_MIN;                     // BestSink() (sink_inl.h:38-40)
    uint32_t bcol = 0xFFFFFFFFu;                  // SINK, SEMI_GLOBAL: zero-based column of `best`
    long long bc = -1;                            // SINK, LOCAL: H << 32 | key; H >= 0, so -1 is "no cell"
    // from the lane above, as in nv_body.inc: H(r0-1, c), F(r0-1, c), H(r0-1, c-1); rH starts as
    // the left boundary H(r0-1, -1)
    const int32_t rb = (int32_t)r0 - 1;
    int32_t rH = (TYPE == NV_LOCAL || lg == 0) ? 0 : A.go + A.ge * rb;
    int32_t rF = kNvInf, pH = 0;
    for (uint32_t s = 0; s < nsteps; ++s) {
        const int32_t c = (int32_t)s - (int32_t)lg;
        int32_t Hup, Fup, Hdg;
        if (lg == 0) {
            if (TYPE == NV_GLOBAL) {
                Hup = A.go + A.ge * c;
                Hdg = c >= 1 ? A.go + A.ge * (c - 1) : 0;
            } else { Hup = 0; Hdg = 0; }
            Fup = kNvInf;
        } else { Hup = rH; Fup = rF; Hdg = pH; }
        if (c >= 0 && (uint32_t)c < stride) {
            const int8_t *const col = tab + mine[c];   // the image's column of this text symbol
            const bool cin = (uint32_t)c < N;
            // SINK: report-order key of (r0, c); row r0 + k adds 8k (nvbio_sink.hpp, Gotoh: SB = 3)
            const uint32_t kb = ((((uint32_t)c >> 3) * M + r0) << 3) | ((uint32_t)c & 7u);
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int32_t S = col[pc[k]];
                const int32_t F = max(Fup + A.ge, Hup + A.go);
                const int32_t E = max(Ek[k] + A.ge, Hk[k] + A.go);
                int32_t H = max(max(E, F), Hdg + S);
                Ek[k] = E;
                Fup = F;
                if (TYPE == NV_LOCAL) {
                    H = max(H, 0);
                    const bool real = cin && (uint32_t)k < nrow;   // pads carry a real symbol: never report them
                    if constexpr (SINK) {
                        const long long cand = ((long long)H << 32) | (long long)(kb + 8u * (uint32_t)k);
                        bc = (real && cand > bc) ? cand : bc;
                    } else best = real ? max(best, H) : best;
                }
                Hdg = Hk[k];
                Hk[k] = H;
                Hup = H;
            }
            if (TYPE != NV_LOCAL && lg == last_lane && cin) {
                int32_t h = 0;
#pragma unroll
                for (int k = 0; k < R; ++k) h = (k == (int)last_k) ? Hk[k] : h;
                if (TYPE == NV_SEMI && SINK) {
                    if (h >= best) { best = h; bcol = (uint32_t)c; }   // columns come in order: the last maximum
                } else if (TYPE == NV_SEMI) best = max(best, h);
                else if ((uint32_t)c == N - 1) best = h;
            }
        }
        pH = rH;
        rH = nv_shr(Hk[R - 1]);
        rF = nv_shr(Fup);
    }
    // LOCAL: the pair's best over its lanes
    if (TYPE == NV_LOCAL && SINK) {   // the greatest (H, key)
#pragma unroll
        for (int m = 1; m < G; m <<= 1) {
            const long long o = __shfl_xor(bc, m);
            bc = o > bc ? o : bc;
        }
    } else if (TYPE == NV_LOCAL) {
#pragma unroll
        for (int m = 1; m < G; m <<= 1) best = max(best, __shfl_xor(best, m));
    }
    const bool writer = TYPE == NV_LOCAL ? lg == 0 : lg == last_lane;
    if (valid && writer) {
        int32_t v = best;
        uint32_t x = N, y = M;                    // SINK: the cell, one-based; GLOBAL: (N, M)
        if constexpr (SINK) {
            if (TYPE == NV_SEMI) x = bcol + 1;
            if (TYPE == NV_LOCAL && bc >= 0) {
                v = (int32_t)(bc >> 32);
                const uint32_t key = (uint32_t)bc, q = key >> 3, sb = q / M;   // bc >= 0: a real row, M >= 1
                x = sb * 8 + (key & 7u) + 1;
                y = q - sb * M + 1;
            }
        }
        if (M == 0) {   // no pattern rows: only the band initialisation reaches the sink
            v = TYPE == NV_SEMI ? (N ? 0 : INT32_MIN)
              : TYPE == NV_GLOBAL ? (N ? A.go + A.ge * (int32_t)(N - 1) : INT32_MIN) : INT32_MIN;
        } else if (N == 0) v = INT32_MIN;
        if (A.score) A.score[pair] = v;
        if constexpr (SINK) {
            if (M == 0) x = N;                    // the band initialisation, reported at y = 0
            if (N == 0 || (TYPE == NV_LOCAL && M == 0)) x = y = 0xFFFFFFFFu;   // no cell was reported
            if (A.sinks) { A.sinks[2 * (size_t)pair] = x; A.sinks[2 * (size_t)pair + 1] = y; }
        }
    }
}

}  // namespace gx
