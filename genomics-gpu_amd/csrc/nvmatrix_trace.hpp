// nvmatrix_trace.hpp — the nvbio front-end's full-DP Gotoh traceback with a substitution matrix:
// what BatchedAlignmentTraceback runs over a GotohAligner whose scheme answers
// substitution(i, j, r, q, qq) from a table (NvB/nvbio/alignment/gotoh/gotoh_inl.h:534; the
// proteinsw example's BlosumScheme, m_matrix[r + q*24] with r the text symbol and q the pattern
// symbol).  GLOBAL / LOCAL / SEMI_GLOBAL, one pair per thread.
//
// nv_traceback_kernel<true, TYPE>'s pass and walk (nvtrace.hpp: stripes of 8 pattern columns with H
// and F in registers, the (H, E) hand-off through A.row, one 8-byte flag store per row and stripe,
// the flag bits with strict comparisons, infimum, the BestSink rules, the H / E / F walk, the
// first-row and first-column tails, NvPushes); what differs is where S comes from:
//   * The table.  nvmatrix.hpp's 32 x 32 int8 image (row = pattern symbol, column = text symbol,
//     1 KB) travels by value in the kernel arguments and every block copies it to the head of its
//     LDS once, before any thread returns (the barrier sees all 256).  A thread keeps 32 * q of its
//     stripe's 8 pattern symbols in registers and reads the row's text symbol once: a cell's score
//     is one add and one signed byte read from LDS, tab[32 * q + r].  No cell loads from global
//     memory for its score.
//   * The clamp.  Symbols come from caller memory: a symbol >= n is read as n - 1 before any LDS
//     address is formed, the pattern symbols when a stripe loads them and the text symbol when a
//     row reads it, so no index leaves the n x n corner of the image.
//   * Pads.  The pad columns of the last stripe (c0 + j > M) carry symbol 0, a real one: under a
//     table there is no code that "never matches", so nv_traceback_kernel's 0xFFFF has no
//     counterpart.  This is safe because nothing real ever reads a pad cell:
//       - a cell depends on its left, upper and upper-left neighbours only, and pads lie to the
//         right of every real cell of their row; the stripe holding them is the last, so the
//         (H, E) it hands on through A.row is read by no stripe;
//       - the LOCAL report is masked by c0 + j <= M, last_h (SEMI_GLOBAL, GLOBAL) is taken at
//         c0 + j == M: a pad's value, however high an all-positive table drives it, never becomes
//         the best;
//       - the walk starts at column <= M - 1 and only moves left or up: it never reads a pad's flags.
// The model is tests/nvbio_matrix_traceback_model.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nvmatrix.hpp"   // the image: kNvMatrixDim, kNvMatrixBytes
#include "nvtrace.hpp"    // NvTbArgs, nvtb_symbol, NvPushes

namespace gx {

struct NvMatrixTbArgs {
    NvTbArgs t;                         // match, mismatch, del and ins are not read
    uint32_t nsym;                      // n: symbols are clamped to n - 1
    uint32_t tab[kNvMatrixBytes / 4];   // int8 image, tab[32 * p + t]
};

// TYPE: 0 GLOBAL, 1 LOCAL, 2 SEMI_GLOBAL (nvbio AlignmentType)
template <int TYPE>
__global__ __launch_bounds__(256) void nv_matrix_traceback_kernel(NvMatrixTbArgs B) {
    __shared__ __attribute__((aligned(16))) uint32_t nvmtb_tab[kNvMatrixBytes / 4];
    nvmtb_tab[threadIdx.x] = B.tab[threadIdx.x];   // 256 threads, 256 words
    __syncthreads();
    const int8_t *const tab = reinterpret_cast<const int8_t *>(nvmtb_tab);
    const NvTbArgs &A = B.t;
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n) return;
    constexpr uint8_t SUB = 0, INS = 1, DEL = 2, SNK = 3, INS_EXT = 4, DEL_EXT = 8;
    constexpr uint32_t BAND = 8;   // gotoh_bandlen_selector (and the LOCAL report order)
    const uint32_t p0 = A.poff[k], M = A.poff[k + 1] - p0;
    const uint32_t t0 = A.toff ? A.toff[k] : 0u, N = A.toff ? A.toff[k + 1] - t0 : A.tlen0;
    const uint32_t n = A.n, top = B.nsym - 1;
    uint32_t *src = A.src + 2 * (size_t)k, *snk = A.snk + 2 * (size_t)k;
    A.n_ops[k] = 0;
    if (M == 0 || N == 0 || M > A.max_m || N > A.max_n || M + N > A.ops_stride) {
        src[0] = src[1] = snk[0] = snk[1] = 0xFFFFFFFFu;
        A.score[k] = INT32_MIN;
        return;
    }
    const int32_t Go = A.go, Ge = A.ge;
    const int32_t infimum = -32768 - (Go < Ge ? Go : Ge);
    const uint32_t stripes = (A.max_m + BAND - 1) / BAND;
    int2 *temp = reinterpret_cast<int2 *>(A.row) + k;   // [row][pair]
    uint2 *dir8 = reinterpret_cast<uint2 *>(A.dir);       // [row][stripe][pair]
    for (uint32_t i = 0; i < N; i++)   // the first column's left neighbours (the checkpoint context's init)
        temp[(size_t)i * n] = make_int2(TYPE == 0 ? Go + Ge * (int32_t)i : 0, TYPE == 1 ? 0 : infimum);
    int32_t best = INT32_MIN;
    uint32_t bx = 0xFFFFFFFFu, by = 0xFFFFFFFFu;
    int32_t last_h = 0;   // H(i, M-1) of the stripe holding column M-1
    for (uint32_t blk = 0; blk * BAND < M; blk++) {
        const uint32_t c0 = blk * BAND;
        uint32_t q[BAND];   // 32 * pattern symbol: the image's row; pads take symbol 0
        int32_t Hb[BAND + 1], Fb[BAND + 1];
#pragma unroll
        for (uint32_t j = 0; j < BAND; j++)
            q[j] = c0 + j < M ? min(nvtb_symbol(A.pw, A.pbits, A.pbig, p0 + c0 + j), top) * kNvMatrixDim : 0u;
#pragma unroll
        for (uint32_t j = 0; j <= BAND; j++) {   // row -1: H(-1, c0 + j - 1)
            const int32_t cc = (int32_t)(c0 + j) - 1;
            Hb[j] = TYPE == 1 || cc < 0 ? 0 : Go + Ge * cc;
            Fb[j] = infimum;
        }
        int32_t diag0 = Hb[0];
        for (uint32_t i = 0; i < N; i++) {
            const int8_t *const col = tab + min(nvtb_symbol(A.tw, A.tbits, A.tbig, t0 + i), top);
            const int2 tv = temp[(size_t)i * n];
            int32_t diagH = diag0;     // H(i-1, c0-1)
            diag0 = tv.x;
            Hb[0] = tv.x;              // H(i, c0-1)
            int32_t E = tv.y;          // E(i, c0-1)
            uint32_t flo = 0, fhi = 0;
#pragma unroll
            for (uint32_t j = 1; j <= BAND; j++) {
                const int32_t S = col[q[j - 1]];
                const int32_t up = Hb[j];
                const int32_t diag = diagH + S;
                const int32_t ftop = Fb[j] + Ge, htop = up + Go;
                const int32_t F = max(ftop, htop);
                const uint32_t fdir = ftop > htop ? DEL_EXT : SUB;
                const int32_t eleft = E + Ge, hleft = Hb[j - 1] + Go;
                E = max(eleft, hleft);
                const uint32_t edir = eleft > hleft ? INS_EXT : SUB;
                Fb[j] = F;
                int32_t h = max(max(E, F), diag);
                if (TYPE == 1) h = max(h, 0);
                const uint32_t hdir = F > E ? (F > diag ? DEL : SUB) : (E > diag ? INS : SUB);
                const uint32_t d = (TYPE == 1 && h == 0 ? SNK : hdir) | edir | fdir;
                diagH = up;
                Hb[j] = h;
                if (j <= 4) flo |= d << (8 * (j - 1)); else fhi |= d << (8 * (j - 5));
                if (TYPE == 1 && c0 + j <= M && best <= h) {   // report order: stripe, row, column; the last maximum wins
                    best = h; bx = i + 1; by = c0 + j;
                }
                if (c0 + j == M) last_h = h;
            }
            dir8[((size_t)i * stripes + blk) * n + k] = make_uint2(flo, fhi);
            temp[(size_t)i * n] = make_int2(Hb[BAND], E);
            if (TYPE == 2 && c0 + BAND >= M && best <= last_h) { best = last_h; bx = i + 1; by = M; }
        }
    }
    if (TYPE == 0) { best = last_h; bx = N; by = M; }
    snk[0] = bx; snk[1] = by;
    const uint8_t *dir = A.dir;
    auto dcell = [&](uint32_t i, uint32_t j) -> uint8_t {
        return dir[(((size_t)i * stripes + j / BAND) * n + k) * 8 + (j % BAND)];
    };
    NvPushes out(A.ops + (size_t)k * A.ops_stride);
    int32_t row = (int32_t)bx, col = (int32_t)by - 1;
    int state = 0;   // H / E / F
    while (row > 0 && col >= 0) {
        const uint8_t op = dcell((uint32_t)(row - 1), (uint32_t)col);
        const uint8_t h_op = op & 3u;
        if (TYPE == 1 && state == 0 && h_op == SNK) break;
        if (state == 1) {
            if ((op & INS_EXT) == 0) state = 0;
            --col; out.push(INS);
        } else if (state == 2) {
            if ((op & DEL_EXT) == 0) state = 0;
            --row; out.push(DEL);
        } else if (h_op == INS) {
            state = 1;
        } else if (h_op == DEL) {
            state = 2;
        } else {
            --col; --row; out.push(SUB);
        }
    }
    uint32_t sx = (uint32_t)row, sy = (uint32_t)(col + 1);
    if (TYPE != 1 && sx == 0)
        for (; sy > 0; --sy) out.push(INS);
    if (TYPE == 0 && sy == 0)
        for (; sx > 0; --sx) out.push(DEL);
    out.flush();
    src[0] = sx; src[1] = sy;
    A.n_ops[k] = out.cnt;
    A.score[k] = best;
}

}  // namespace gx
