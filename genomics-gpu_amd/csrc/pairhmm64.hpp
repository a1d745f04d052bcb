// pairhmm64.hpp — PairHMM forward in float64: the rescue path of the fp32 kernel (pairhmm.hpp).
//
// A read that fits its haplotype badly underflows the fp32 range (initial constant 2^120) and
// the fp32 kernel returns 0.  This kernel evaluates the same recurrence with the same boundary
// in double, from the initial constant 2^1020: the fp32 parameter arrays (or the fp32 ph2pr
// entries of the quality form) and the constants 0.9f / 0.1f are widened as given, and 1 - Qm,
// Qm / 3, c0 / H and everything after them are double operations.  Nothing here is bit-exact
// against a reference; the three FMA sites of the fp32 kernel are fma() here too.
//
// Structure as pairhmm.hpp: G lanes per pair, RR read rows per lane, rows bottom-aligned (the
// read's last row is the bottom row of lane G-1), haplotype bytes staged in LDS, the bottom
// row's (M, I, D) handed to the next lane with DPP wave_shr:1, a double as its two 32-bit
// halves.  The prior of a cell is the compare form, (hb == rb) ? 1 - Qm : Qm / 3: a per-lane
// table would hold 8 bytes per entry (64 KB per block at 8 rows) and save one compare and two
// selects beside nine double operations per cell ("PairHMM in float64").
//
// Launch form: slots [slot0, n) through perm as the fp32 kernel, and n_dev, a pair count in
// device memory (the length of a list built on the device): slots from *n_dev on are not run,
// and a block whose first slot is past it returns as a whole before its first barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gx {

struct Hmm64Args {
    const uint8_t *reads;
    const uint32_t *roff, *rlen;
    const float *qm, *delta, *xiksi, *alpha;
    const uint8_t *haps;
    const uint32_t *hoff, *hlen;
    const uint8_t *bq, *iq, *dq;   // QUALS: Phred qualities at the read offsets
    const float *ph2pr;            // 128 entries
    double *result;                // by pair index
    const uint32_t *perm;          // slot -> pair, or NULL
    const uint32_t *n_dev;         // device-side slot count, or NULL
    uint32_t n, slot0;
    uint32_t lds_stride;           // bytes per pair slot (>= max haplotype length, multiple of 4)
    uint32_t log10_out;            // write log10(value) - log10(2^1020) instead of the value
};

constexpr double kHmm64C0 = 0x1p1020;
constexpr double kHmm64Log10C0 = 1020.0 * 0.30102999566398119521;   // 1020 log10(2)
constexpr double kHmm32Log10C0 = 120.0 * 0.30102999566398119521;    // the fp32 kernel's 2^120

// lane i takes lane i-1's value (wave_shr:1); lane 0 of the wave reads 0
__device__ __forceinline__ double shr_lane_d(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, 0x138, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), 0x138, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

template <int G, int RR, bool QUALS>
__global__ __launch_bounds__(256) void pairhmm64_kernel(Hmm64Args A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds64[];
    constexpr int P = 64 / G;
    const double c0 = kHmm64C0, c09 = (double)0.9f, c01 = (double)0.1f;
    uint32_t n = A.n;
    if (A.n_dev) n = min(n, *A.n_dev);
    if (A.slot0 + blockIdx.x * (4 * P) >= n) return;       // block-uniform, before any barrier
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t lg = lane & (G - 1), slot = lane / G;
    const uint32_t idx = A.slot0 + (blockIdx.x * 4 + wave) * P + slot;
    const bool valid = idx < n;
    const uint32_t pair = (valid && A.perm) ? A.perm[idx] : idx;
    uint32_t R = 0, H = 0, ro = 0, ho = 0;
    if (valid) { R = A.rlen[pair]; H = A.hlen[pair]; ro = A.roff[pair]; ho = A.hoff[pair]; }

    // stage the wave's haplotypes
    const uint32_t stride = A.lds_stride;
    uint8_t *wl = lds64 + (size_t)wave * P * stride;
    const uint32_t words = stride >> 2;
    for (uint32_t base = 0; base < P * words; base += 64) {
        const uint32_t wi = base + lane;
        const uint32_t ps = min(wi / words, (uint32_t)P - 1), w = wi - ps * words;
        const uint32_t pH = __shfl(H, ps * G), pho = __shfl(ho, ps * G);
        if (wi < P * words) {
            uint32_t v = 0;
            for (int b = 0; b < 4; ++b)
                if (4 * w + b < pH) v |= (uint32_t)A.haps[pho + 4 * w + b] << (8 * b);
            reinterpret_cast<uint32_t *>(wl + ps * stride)[w] = v;
        }
    }
    __syncthreads();
    const uint8_t *hap = wl + slot * stride;

    // the lane's rows [r0, r0 + RR) of the group's [R - G*RR, R); rows above row 0 are virtual
    // (prior 0, delta 0, xi 0, D decay 1) and pass (0, 0, D0) down unchanged (pairhmm.hpp)
    const int32_t r0 = (int32_t)(lg * RR) - (int32_t)(G * RR) + (int32_t)R;
    uint32_t rb[RR];
    double qm1[RR], qm3[RR], de[RR], al[RR], xi[RR], dk[RR];
    double Mk[RR], Dk[RR], MM[RR];
    const double D0 = valid && H ? c0 / (double)H : 0.0;
#pragma unroll
    for (int k = 0; k < RR; ++k) {
        const int32_t i = r0 + k;
        const bool in = valid && i >= 0;
        float q = 0.f, d = 0.f, x = 0.f, a = 0.f;
        if (in) {
            if (QUALS) {
                const uint32_t b = A.bq[ro + i] & 127u, iqv = A.iq[ro + i] & 127u, dqv = A.dq[ro + i] & 127u;
                q = A.ph2pr[b];
                d = A.ph2pr[iqv];
                x = A.ph2pr[dqv];
                a = __fsub_rn(1.0f, A.ph2pr[(iqv + dqv) & 127u]);   // the host's fp32 alpha (gasalx_pairhmm_params)
            } else {
                q = A.qm[ro + i]; d = A.delta[ro + i]; x = A.xiksi[ro + i]; a = A.alpha[ro + i];
            }
        }
        rb[k] = in ? A.reads[ro + i] : 0x100u;
        qm1[k] = in ? 1.0 - (double)q : 0.0;
        qm3[k] = in ? (double)q / 3.0 : 0.0;
        de[k] = (double)d; al[k] = (double)a; xi[k] = (double)x;
        dk[k] = in ? c01 : 1.0;
        Mk[k] = 0.0;
        Dk[k] = in ? 0.0 : D0;
        MM[k] = i == 0 ? c09 * D0 : 0.0;
    }

    const bool bottom = lg == G - 1;
    double acc = 0.0;
    double rM = 0.0, rI = 0.0, rD = 0.0;    // bottom-row values of the lane above, this column
    // one column of the lane's rows; (MU, IU, DU) in = row r0-1, out = the lane's bottom row
    auto column = [&](uint32_t hb, double &MU, double &IU, double &DU) {
#pragma unroll
        for (int k = 0; k < RR; ++k) {
            const double prior = (hb == rb[k]) ? qm1[k] : qm3[k];
            const double MID = IU + DU;
            const double Mn = prior * MM[k];
            const double In = fma(MU, de[k], IU * c01);
            const double Dn = fma(Dk[k], dk[k], Mk[k] * xi[k]);
            MM[k] = fma(al[k], MU, c09 * MID);
            Mk[k] = Mn; Dk[k] = Dn;
            MU = Mn; IU = In; DU = Dn;
        }
    };
    auto checked_step = [&](uint32_t s) {
        const int32_t j = (int32_t)s - (int32_t)lg;
        double MU = rM, IU = rI, DU = rD;
        if (lg == 0) { MU = 0.0; IU = 0.0; DU = D0; }                   // row -1: M = I = 0, D = D0
        if (valid && j >= 0 && (uint32_t)j < H) {
            column(hap[j], MU, IU, DU);
            if (bottom) acc += MU + IU;                                 // row R-1, column j
        }
        rM = shr_lane_d(MU); rI = shr_lane_d(IU); rD = shr_lane_d(DU);
    };
    uint32_t hmax = H, hmin = valid ? H : 0u;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        hmax = max(hmax, (uint32_t)__shfl_xor(hmax, m));
        hmin = min(hmin, (uint32_t)__shfl_xor(hmin, m));
    }
    const uint32_t nsteps = hmax + G - 1;
    const uint32_t s1 = min((uint32_t)G - 1, nsteps), s2 = max(s1, hmin);
    for (uint32_t s = 0; s < s1; ++s) checked_step(s);
    // steps [G-1, hmin): every lane of the wave is inside its pair's columns
    for (uint32_t s = s1; s < hmin; ++s) {
        double MU = rM, IU = rI, DU = rD;
        if (lg == 0) { MU = 0.0; IU = 0.0; DU = D0; }
        column(hap[s - lg], MU, IU, DU);
        acc += MU + IU;                                                 // kept by the bottom lane only
        rM = shr_lane_d(MU); rI = shr_lane_d(IU); rD = shr_lane_d(DU);
    }
    for (uint32_t s = s2; s < nsteps; ++s) checked_step(s);
    if (valid && bottom) A.result[pair] = A.log10_out ? log10(acc) - kHmm64Log10C0 : acc;
}

}  // namespace gx
