// pairhmm64.hip — the float64 PairHMM kernel's launches and the log10 rescue pass.
//
// Its own translation unit: the fp32 kernel (dispatch.hip, pairhmm.hpp) is compiled exactly as
// before.  Three things live here:
//   * pairhmm64_device: the raw float64 forward value of every pair (initial constant 2^1020);
//   * hmm_select_kernel: after an fp32 launch, log10 of every result the caller accepts, and the
//     list of the pairs it does not;
//   * pairhmm_log10_device: select, then the float64 kernel over that list, sized for the worst
//     case (the list's length stays on the device; surplus blocks return at once).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "engine.hpp"
#include "pairhmm64.hpp"

namespace gx {

#define HIPCHK(x)                                                                        \
    do {                                                                                 \
        hipError_t e__ = (x);                                                            \
        if (e__ != hipSuccess) {                                                         \
            set_error(std::string(#x) + ": " + hipGetErrorString(e__));                  \
            return GASALX_EDEVICE;                                                       \
        }                                                                                \
    } while (0)

// Pairs whose fp32 result r is accepted (r >= min_accepted and finite): their log10 likelihood,
// used[i] = 0.  The others: index appended to list (count: *count, zeroed by the host before
// the launch), used[i] = 1; the float64 kernel writes their output.  One atomic per wave: the
// wave's rescued lanes take consecutive list entries from the first such lane's add.
__global__ __launch_bounds__(256) void hmm_select_kernel(const float *r32, uint32_t n, float min_accepted,
                                                         double *out, uint8_t *used, uint32_t *list,
                                                         uint32_t *count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool in = i < n;
    const float r = in ? r32[i] : 0.f;
    const bool ok = r >= min_accepted && r < __builtin_inff();   // false for NaN
    const bool rescue = in && !ok;
    if (in && ok) out[i] = log10((double)r) - kHmm32Log10C0;
    if (in && used) used[i] = rescue ? 1 : 0;
    const uint64_t mask = __ballot(rescue);
    if (mask) {
        const uint32_t lane = threadIdx.x & 63u;
        const int leader = __ffsll((long long)mask) - 1;
        uint32_t base = 0;
        if ((int)lane == leader) base = atomicAdd(count, (uint32_t)__popcll(mask));
        base = __shfl(base, leader);
        if (rescue) list[base + __popcll(mask & ((1ull << lane) - 1ull))] = i;
    }
}

using Hmm64Fn = void (*)(Hmm64Args);
template <bool QUALS>
static Hmm64Fn hmm64_lookup(int G, int rows) {
    if (rows == 8) return G == 64 ? &pairhmm64_kernel<64, 8, QUALS> : nullptr;
    switch (G) {
        case 4: return &pairhmm64_kernel<4, 4, QUALS>;
        case 8: return &pairhmm64_kernel<8, 4, QUALS>;
        case 16: return &pairhmm64_kernel<16, 4, QUALS>;
        case 32: return &pairhmm64_kernel<32, 4, QUALS>;
        case 64: return &pairhmm64_kernel<64, 4, QUALS>;
        default: return nullptr;
    }
}

// 4 read rows per lane up to 256 rows (G = 4 .. 64), 8 rows on 64 lanes up to 512
int pairhmm64_shape(uint32_t max_r, int *rows) {
    *rows = max_r > 256 ? 8 : 4;
    if (max_r > 512) return 0;
    for (int g : {4, 8, 16, 32, 64})
        if ((uint32_t)g * *rows >= max_r) return g;
    return 0;
}

static void hmm64_fill(Hmm64Args &A, const Hmm64Src &s) {
    std::memset(&A, 0, sizeof(A));
    if (s.quals) {
        const gasalx_hmm_qual_batch &b = *s.quals;
        A.reads = b.reads; A.roff = b.read_offsets; A.rlen = b.read_lens;
        A.bq = b.base_quals; A.iq = b.ins_quals; A.dq = b.del_quals; A.ph2pr = s.ph2pr;
        A.haps = b.haps; A.hoff = b.hap_offsets; A.hlen = b.hap_lens;
    } else {
        const gasalx_hmm_batch &b = *s.params;
        A.reads = b.reads; A.roff = b.read_offsets; A.rlen = b.read_lens;
        A.qm = b.qm; A.delta = b.delta; A.xiksi = b.xiksi; A.alpha = b.alpha;
        A.haps = b.haps; A.hoff = b.hap_offsets; A.hlen = b.hap_lens;
    }
}

// One launch over slots [0, n) (through A.perm, up to *A.n_dev when set).
static int pairhmm64_launch(Hmm64Args A, bool quals, uint32_t n, uint32_t max_r, uint32_t max_h, hipStream_t st) {
    if (n == 0) return GASALX_OK;
    int rows;
    const int G = pairhmm64_shape(max_r, &rows);
    if (!G) { set_error("PairHMM read longer than 512"); return GASALX_ERANGE; }
    A.slot0 = 0;
    A.n = n;
    A.lds_stride = (std::max<uint32_t>(max_h, 4) + 3) & ~3u;
    // haplotype slots only: 4 waves x 64/G pairs
    const size_t lds = ((size_t)4 * (64 / G) * A.lds_stride + 15) & ~(size_t)15;
    if (lds > 160 * 1024) { set_error("PairHMM haplotype too long"); return GASALX_ERANGE; }
    Hmm64Fn fn = quals ? hmm64_lookup<true>(G, rows) : hmm64_lookup<false>(G, rows);
    const uint32_t ppb = 4 * (64 / G);
    HIPCHK(launch_lds(fn, dim3((n + ppb - 1) / ppb), dim3(256), lds, st, A));
    return GASALX_OK;
}

int pairhmm64_device(const Hmm64Src &src, uint32_t n, double *result, hipStream_t st, uint32_t max_r,
                     uint32_t max_h) {
    Hmm64Args A;
    hmm64_fill(A, src);
    A.result = result;
    return pairhmm64_launch(A, src.quals != nullptr, n, max_r, max_h, st);
}

int pairhmm_log10_device(const Hmm64Src &src, uint32_t n, const float *r32, float min_accepted, double *out,
                         uint8_t *used, uint32_t *count, uint32_t *list, hipStream_t st, uint32_t max_r,
                         uint32_t max_h) {
    if (n == 0) return GASALX_OK;
    if (!(min_accepted > 0.f)) min_accepted = 1e-28f;
    // a denormal fp32 result has lost mantissa bits: never accepted, whatever the caller's bound
    min_accepted = std::max(min_accepted, 1.17549435e-38f);
    HIPCHK(hipMemsetAsync(count, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(hmm_select_kernel, dim3((n + 255) / 256), dim3(256), 0, st, r32, n, min_accepted, out, used,
                       list, count);
    HIPCHK(hipGetLastError());
    Hmm64Args A;
    hmm64_fill(A, src);
    A.result = out;
    A.perm = list;
    A.n_dev = count;
    A.log10_out = 1;
    return pairhmm64_launch(A, src.quals != nullptr, n, max_r, max_h, st);
}

}  // namespace gx
