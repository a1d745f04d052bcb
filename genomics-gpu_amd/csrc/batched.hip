// batched.hip — launcher of the nvbio-style batched scoring front-end (nvbio.hpp).
// Replaces BatchedAlignmentScore<stream, scheduler>::enact (NvB/nvbio/alignment/
// batched_inl.h) and the scheduler tags (batched.h:44-87): every scheduler maps to
// the same lane-group wavefront launch; there is no temporary storage.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>

#include "engine.hpp"
#include "nvbio.hpp"
#include "nvbio_sink.hpp"
#include "nvtrace.hpp"
#include "nvbio16.hpp"
#include "nvbanded.hpp"
#include "nvbanded_sink.hpp"
#include "nvmyers.hpp"
#include "nvmatrix.hpp"
#include "nvmatrix_trace.hpp"
#include "nvbanded_qual.hpp"

namespace gx {

namespace {

struct NvShape { int G, R; };
// the smallest G*R >= the longest pattern: 150-bp reads take (8, 19), 152 rows
constexpr NvShape kNvShapes[] = {{8, 8}, {8, 12}, {8, 16}, {8, 19}, {8, 24}, {16, 16}, {16, 20}, {32, 16}, {64, 16}};
constexpr size_t kNvShapeCount = sizeof(kNvShapes) / sizeof(kNvShapes[0]);

// ---- run-time values as template arguments: every kernel lookup goes through these ----
template <int V> using ic = std::integral_constant<int, V>;

// f(ic<ALN>, ic<TYPE>, bool_constant<FLAG>) for the aligner kind (Gotoh, or linear gaps: ED runs
// as SW), the alignment type and one flag
template <class F>
auto nv_static(int aligner, int type, bool flag, F f) {
    auto by_type = [&](auto a, auto fl) {
        return type == NV_GLOBAL ? f(a, ic<NV_GLOBAL>{}, fl)
             : type == NV_SEMI ? f(a, ic<NV_SEMI>{}, fl) : f(a, ic<NV_LOCAL>{}, fl);
    };
    auto by_aligner = [&](auto fl) {
        return aligner == NV_GOTOH ? by_type(ic<NV_GOTOH>{}, fl) : by_type(ic<NV_SW>{}, fl);
    };
    return flag ? by_aligner(std::true_type{}) : by_aligner(std::false_type{});
}
template <class F, size_t... I>
auto nv_shape_table(F f, std::index_sequence<I...>) {
    return std::array{f(ic<kNvShapes[I].G>{}, ic<kNvShapes[I].R>{})...};
}
// f(ic<ALN>, ic<TYPE>, bool_constant<FLAG>, ic<G>, ic<R>) at shape kNvShapes[shape].  The table is
// built from the shape list itself, so every shape the planner can choose has its instance of
// every kernel family: no lookup returns null.
template <class F>
auto nv_instance(int aligner, int type, bool flag, int shape, F f) {
    return nv_static(aligner, type, flag, [&](auto a, auto t, auto fl) {
        return nv_shape_table([&](auto g, auto r) { return f(a, t, fl, g, r); },
                              std::make_index_sequence<kNvShapeCount>{})[shape];
    });
}

using NvFn = void (*)(NvArgs);
using Nv16Fn = void (*)(Nv16Args);
// the sink-tracking forms (nvbio_sink.hpp): one instance per score-only instance, MASK apart
using NvSinkFn = void (*)(NvSinkArgs);
using Nv16SinkFn = void (*)(Nv16SinkArgs);
NvFn nv_lookup(int aligner, int type, bool mask, int shape) {   // MASK exists for LOCAL only
    return nv_instance(aligner, type, mask, shape, [](auto a, auto t, auto m, auto g, auto r) -> NvFn {
        return &nv_kernel<a, t, g, r, m && t == NV_LOCAL>; });
}
NvSinkFn nv_sink_lookup(int aligner, int type, int shape) {
    return nv_instance(aligner, type, false, shape, [](auto a, auto t, auto, auto g, auto r) -> NvSinkFn {
        return &nv_sink_kernel<a, t, g, r>; });
}
Nv16Fn nv16_lookup(int aligner, int type, bool shared, int shape) {
    return nv_instance(aligner, type, shared, shape, [](auto a, auto t, auto s, auto g, auto r) -> Nv16Fn {
        return &nv16_kernel<a, t, g, r, s>; });
}
Nv16SinkFn nv16_sink_lookup(int aligner, int type, bool shared, int shape) {
    return nv_instance(aligner, type, shared, shape, [](auto a, auto t, auto s, auto g, auto r) -> Nv16SinkFn {
        return &nv16_sink_kernel<a, t, g, r, s>; });
}

// ---- the scheme, the kernel arguments, checks and the launch, each written once ----
struct NvScheme { int32_t match, mismatch, go, ge, del, ins; };
// ED runs as SW with EditDistanceSWScheme's scores (ed_utils.h:45-52, ed_banded_inl.h:63-78,
// ed_inl.h:347-365); gap_open / gap_ext are passed on as given
NvScheme nv_scheme(const gasalx_nv_aligner &al) {
    if (al.aligner == NV_ED) return {0, -1, al.gap_open, al.gap_ext, -1, -1};
    return {al.match, al.mismatch, al.gap_open, al.gap_ext, al.deletion, al.insertion};
}
// The largest score magnitude.  Not capi.cpp's nv_score_mag, which is 1 for ED: here an ED aligner's
// gap_open / gap_ext count although no ED kernel reads them (tests/golden/nv_plan_names.json pins it).
int64_t nv_score_mag(const NvScheme &s) {
    return std::max<int64_t>({std::abs((int64_t)s.match), std::abs((int64_t)s.mismatch), std::abs((int64_t)s.go),
                              std::abs((int64_t)s.ge), std::abs((int64_t)s.del), std::abs((int64_t)s.ins), 1});
}
int64_t nv_gap_sum(const NvScheme &s) {
    return std::abs((int64_t)s.go) + std::abs((int64_t)s.ge) + std::abs((int64_t)s.del) + std::abs((int64_t)s.ins);
}

template <class Args, class = void> struct has_tbits : std::false_type {};
template <class Args> struct has_tbits<Args, std::void_t<decltype(Args::tbits)>> : std::true_type {};
// the string sets, the scheme and the pair count of any kernel argument struct (the packed
// kernels' have no tbits: their texts are 2-bit)
template <class Args>
void nv_fill_strings(Args &A, const gasalx_nv_strings &pat, const gasalx_nv_strings &txt, uint32_t n) {
    A.pw = pat.words; A.poff = pat.offsets; A.pbits = pat.bits; A.pbig = pat.big_endian;
    A.tw = txt.words; A.toff = txt.offsets; A.tbig = txt.big_endian; A.tlen0 = txt.offsets ? 0 : txt.length;
    if constexpr (has_tbits<Args>::value) A.tbits = txt.bits;
    A.n = n;
}
template <class Args>
void nv_fill(Args &A, const gasalx_nv_strings &pat, const gasalx_nv_strings &txt, const NvScheme &s, uint32_t n) {
    nv_fill_strings(A, pat, txt, n);
    A.match = s.match; A.mismatch = s.mismatch; A.go = s.go; A.ge = s.ge; A.del = s.del; A.ins = s.ins;
}

int nv_fail(int rc, const std::string &msg) { set_error(msg); return rc; }
// Aligner, type, band (where there is one) and symbol bits, in the order every entry point checks
// them; the traceback forms have a text of their own for the aligner and one for the type.
int nv_check(const gasalx_nv_aligner &al, const char *aligner_msg, const char *type_msg, const uint32_t *band,
             const gasalx_nv_strings &pat, const gasalx_nv_strings &txt) {
    if (al.aligner < 0 || al.aligner > 2) return nv_fail(GASALX_EINVAL, aligner_msg);
    if (al.type < 0 || al.type > 2) return nv_fail(GASALX_EINVAL, type_msg);
    if (band && (*band < 2 || *band > 32)) return nv_fail(GASALX_EINVAL, "band length must be 2..32");
    for (uint32_t b : {pat.bits, txt.bits})
        if (b != 2 && b != 4 && b != 8) return nv_fail(GASALX_EINVAL, "symbol bits must be 2, 4 or 8");
    return GASALX_OK;
}
int nv_check_ptrs(const gasalx_nv_strings &pat, const gasalx_nv_strings &txt, bool outputs) {
    if (!pat.words || !pat.offsets || !txt.words || !outputs) return nv_fail(GASALX_EINVAL, "null argument");
    return GASALX_OK;
}

int nv_launched(hipError_t e) { return e == hipSuccess ? GASALX_OK : nv_fail(GASALX_EDEVICE, hipGetErrorString(e)); }
// 256-thread blocks; with dynamic LDS through launch_lds, without as a plain launch
template <class Args>
int launch_checked(void (*fn)(Args), uint32_t blocks, size_t lds, hipStream_t st, const Args &A) {
    return nv_launched(launch_lds(fn, dim3(blocks), dim3(256), lds, st, A));
}
template <class Args>
int launch_checked(void (*fn)(Args), uint32_t blocks, hipStream_t st, const Args &A) {
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(256), 0, st, A);
    return nv_launched(hipGetLastError());
}

// ---- the packed kernels' 16-bit window ----
// Values within +-vabs = span * mag * 2 of the stored zero `base`, and the gap scores below it,
// inside f16's integer range (nvbio16.hpp, nvbanded.hpp).
bool nv_f16_window(int64_t span, int64_t mag, int64_t gap_sum, uint32_t *base) {
    const int64_t vabs = span * mag * 2;
    const int64_t b = 0x400 + 2 * gap_sum + vabs + 64;
    if (b + vabs + 512 > 0x7BFF) return false;
    *base = (uint32_t)b;
    return true;
}

// The packed kernel (nvbio16.hpp): 2-bit texts, gaps and mismatches <= 0, match - mismatch in a
// byte, and every value (bounded by (M + N + 2) * the largest score magnitude) inside the 16-bit
// f16 window.  GASALX_NV16=0: int32 only.
bool nv16_ok(const NvScheme &s, bool gotoh, int type, uint32_t text_bits, uint32_t max_p, uint32_t max_t,
             uint32_t *base) {
    if (!env_flag("GASALX_NV16", true)) return false;
    if (text_bits != 2) return false;
    if (s.match < s.mismatch || s.match - s.mismatch > 255) return false;
    // only the gap scores the aligner reads, and the mismatch: deliberately not nvb16_ok's rule (pinned)
    if (gotoh ? (s.go > 0 || s.ge > 0) : (s.del > 0 || s.ins > 0)) return false;
    if (s.mismatch > 0 || s.mismatch < -255) return false;   // virtual rows score the byte |mismatch|
    const int64_t mag = nv_score_mag(s);
    if (mag > 0x200) return false;   // a gap subtracted from NEG must not borrow across the halves
    if (gotoh && type != NV_LOCAL) {
        // the drift frame (nvbio16.hpp FR): values + g*(r+c) + (go - ge) lie within the
        // all-gap path below and the diagonal above; virtual rows (r >= -G*R, G*R <=
        // 2*max_p + 64) fall by g per row, sink keys add up to g*max_t
        const int64_t g = -(int64_t)s.ge, gr = 2 * (int64_t)max_p + 64;
        const int64_t b = 0x400 + g * (gr + 2) + 4 * (std::abs((int64_t)s.go) + g) + 64;
        const int64_t top = b + std::abs((int64_t)s.go - s.ge) + std::max<int64_t>(s.match, 0) * max_p +
                            g * ((int64_t)max_p + 2 * (int64_t)max_t + 4) + 512;
        if (top > 0x7BFF) return false;
        *base = (uint32_t)b;
        return true;
    }
    return nv_f16_window((int64_t)max_p + max_t + 2, mag, nv_gap_sum(s), base);
}

// the packed banded kernel: as nv16_ok over (M + band + 2); GASALX_NVB16=0: int32 only
bool nvb16_ok(const NvScheme &s, uint32_t text_bits, uint32_t max_p, uint32_t band, uint32_t *base) {
    if (!env_flag("GASALX_NVB16", true)) return false;
    if (text_bits != 2) return false;
    if (s.match < s.mismatch || s.match - s.mismatch > 255) return false;
    // all four gap scores whatever the aligner, no mismatch test: deliberately not nv16_ok's rule (pinned)
    if (s.go > 0 || s.ge > 0 || s.del > 0 || s.ins > 0) return false;
    const int64_t mag = nv_score_mag(s);
    if (mag > 0x200) return false;
    return nv_f16_window((int64_t)max_p + band + 2, mag, nv_gap_sum(s), base);
}

// ---- the plan of a scoring call: nv_plan_name formats it, the entry points launch from it ----
enum NvFamily { NV_FAMILY_NONE, NV_FAMILY_INT32, NV_FAMILY_PACKED };
struct NvPlan {
    NvFamily family = NV_FAMILY_NONE;
    int shape = 0;                      // index into kNvShapes
    size_t lds = 0;                     // dynamic LDS bytes of the family's kernel
    uint32_t per_block = 0;             // pairs per block (packed: two per lane group)
    uint32_t lds_stride = 0;            // int32: 16-bit codes per text slot
    uint32_t base = 0, lds_cols = 0;    // packed: the stored zero, table entries per staged text
    bool mask = false;                  // int32 LOCAL: mask the pad cells
};
constexpr size_t kNvLdsMax = 160 * 1024;

// The lane-group shape is the smallest G*R that covers the patterns whose int32 text slots fit in
// LDS (one shared slot, or one per pair); the packed kernel runs at that shape inside its window
// (nv16_ok) while its tables fit: one per column of the shared text, or of every pair's text
// (two pairs per lane group, 4 waves per block).
NvPlan nv_make_plan(const gasalx_nv_aligner &al, uint32_t max_p, uint32_t max_t, bool per_pair_text,
                    uint32_t text_bits) {
    NvPlan P;
    if (al.aligner < 0 || al.aligner > 2 || al.type < 0 || al.type > 2) return P;
    P.lds_stride = (std::max<uint32_t>(max_t, 1) + 7u) & ~7u;
    for (; P.shape < (int)kNvShapeCount; P.shape++) {
        const NvShape &sh = kNvShapes[P.shape];
        P.per_block = 4 * (64 / sh.G);
        P.lds = per_pair_text ? (size_t)P.per_block * P.lds_stride * 2 : (size_t)P.lds_stride * 2;
        if ((uint32_t)(sh.G * sh.R) >= max_p && P.lds <= kNvLdsMax) break;
    }
    if (P.shape == (int)kNvShapeCount) return P;
    const int G = kNvShapes[P.shape].G;
    const NvScheme s = nv_scheme(al);
    const bool gotoh = al.aligner == NV_GOTOH;
    // LOCAL pads (pattern rows >= M, text columns >= N) never exceed a real cell when no
    // step can raise a score without a match; otherwise mask them
    P.mask = al.type == NV_LOCAL && (s.mismatch > 0 || (gotoh ? (s.go > 0 || s.ge > 0) : (s.del > 0 || s.ins > 0)));
    P.family = NV_FAMILY_INT32;
    const uint32_t cols = per_pair_text ? (max_t + 3u) & ~3u : (max_t + G + 63u) & ~63u;
    const size_t lds16 = (size_t)cols * 4 * (per_pair_text ? 2 * P.per_block : 1);
    if (lds16 <= kNvLdsMax && nv16_ok(s, gotoh, al.type, text_bits, max_p, max_t, &P.base)) {
        P.family = NV_FAMILY_PACKED;
        P.lds = lds16; P.per_block *= 2; P.lds_cols = cols;
    }
    return P;
}

// The checks and the plan both scoring entry points share (outputs apart); a shared text sets max_t.
int nv_score_plan(const gasalx_nv_aligner &al, const gasalx_nv_strings &pat, const gasalx_nv_strings &txt,
                  bool outputs, uint32_t max_p, uint32_t max_t, NvPlan &P) {
    if (int rc = nv_check(al, "bad aligner", "bad aligner", nullptr, pat, txt)) return rc;
    if (int rc = nv_check_ptrs(pat, txt, outputs)) return rc;
    if (!txt.offsets) max_t = txt.length;
    // |values| stay far from the -inf stand-in (nvbio's infimum never wins either)
    if ((int64_t)(max_p + max_t + 2) * nv_score_mag(nv_scheme(al)) * 2 >= (1ll << 28))
        return nv_fail(GASALX_ERANGE, "scores out of the exact range");
    P = nv_make_plan(al, max_p, max_t, txt.offsets != nullptr, txt.bits);
    if (P.family == NV_FAMILY_NONE)
        return nv_fail(GASALX_ERANGE, "pattern longer than 1024 or text too long for LDS (" + std::to_string(max_p) +
                                          ", " + std::to_string(max_t) + ")");
    return GASALX_OK;
}

NvArgs nv_args(const gasalx_nv_aligner &al, uint32_t n, const gasalx_nv_strings &pat, const gasalx_nv_strings &txt,
               const NvPlan &P, int32_t *scores, int16_t *scores16) {
    NvArgs A;
    nv_fill(A, pat, txt, nv_scheme(al), n);
    A.score = scores; A.score16 = scores16; A.lds_stride = P.lds_stride;
    return A;
}
Nv16Args nv16_args(const gasalx_nv_aligner &al, uint32_t n, const gasalx_nv_strings &pat, const gasalx_nv_strings &txt,
                   const NvPlan &P, int32_t *scores, int16_t *scores16) {
    Nv16Args D;
    nv_fill(D, pat, txt, nv_scheme(al), n);
    D.score = scores; D.score16 = scores16; D.base = P.base; D.lds_cols = P.lds_cols;
    return D;
}

}  // namespace

std::string nv_plan_name(const gasalx_nv_aligner &al, uint32_t max_p, uint32_t max_t, bool per_pair_text,
                         uint32_t text_bits) {
    static const char *an[] = {"ed", "sw", "gotoh"}, *tn[] = {"global", "local", "semi"};
    const NvPlan P = nv_make_plan(al, max_p, max_t, per_pair_text, text_bits);
    if (P.family == NV_FAMILY_NONE) return "none";
    return std::string(P.family == NV_FAMILY_PACKED ? "nvbio16_" : "nvbio_") + an[al.aligner] + "_" + tn[al.type] +
           (per_pair_text ? "" : "_shared") + "_G" + std::to_string(kNvShapes[P.shape].G) + "R" +
           std::to_string(kNvShapes[P.shape].R);
}

int nv_score_device(const gasalx_nv_aligner &al, uint32_t n, const gasalx_nv_strings &pat,
                    const gasalx_nv_strings &txt, int32_t *scores, int16_t *scores16, uint32_t max_p, uint32_t max_t,
                    hipStream_t st) {
    if (n == 0) return GASALX_OK;
    NvPlan P;
    if (int rc = nv_score_plan(al, pat, txt, scores || scores16, max_p, max_t, P)) return rc;
    const uint32_t blocks = (n + P.per_block - 1) / P.per_block;
    if (P.family == NV_FAMILY_PACKED)
        return launch_checked(nv16_lookup(al.aligner, al.type, !txt.offsets, P.shape), blocks, P.lds, st,
                              nv16_args(al, n, pat, txt, P, scores, scores16));
    return launch_checked(nv_lookup(al.aligner, al.type, P.mask, P.shape), blocks, P.lds, st,
                          nv_args(al, n, pat, txt, P, scores, scores16));
}

// Score and BestSink position per pair (nvbio_sink.hpp).  The plan is the score-only one: the
// packed sink kernel where the packed kernel would run, the int32 sink kernel otherwise, at the
// same lane-group shape; "_sink" marks the name.
std::string nv_sinks_plan_name(const gasalx_nv_aligner &al, uint32_t max_p, uint32_t max_t, bool per_pair_text,
                               uint32_t text_bits) {
    const std::string name = nv_plan_name(al, max_p, max_t, per_pair_text, text_bits);
    return name == "none" ? name : name + "_sink";
}

int nv_score_sinks_device(const gasalx_nv_aligner &al, uint32_t n, const gasalx_nv_strings &pat,
                          const gasalx_nv_strings &txt, int32_t *scores, uint32_t *sinks, uint32_t max_p,
                          uint32_t max_t, hipStream_t st) {
    if (n == 0) return GASALX_OK;
    NvPlan P;
    if (int rc = nv_score_plan(al, pat, txt, scores || sinks, max_p, max_t, P)) return rc;
    const uint32_t blocks = (n + P.per_block - 1) / P.per_block;
    if (P.family == NV_FAMILY_PACKED)
        return launch_checked(nv16_sink_lookup(al.aligner, al.type, !txt.offsets, P.shape), blocks, P.lds, st,
                              Nv16SinkArgs{nv16_args(al, n, pat, txt, P, scores, nullptr), sinks});
    return launch_checked(nv_sink_lookup(al.aligner, al.type, P.shape), blocks, P.lds, st,
                          NvSinkArgs{nv_args(al, n, pat, txt, P, scores, nullptr), sinks});
}

// ---- GotohAligner over a substitution matrix (nvmatrix.hpp): int32, full DP, the score-only or the
//      sink-tracking form at the smallest lane-group shape that covers the patterns.  The LDS budget
//      is this family's own: the table image, then one byte per column of every text slot. ----
namespace {

struct NvMatrixPlan {
    bool ok = false;
    int shape = 0;
    size_t lds = 0;
    uint32_t per_block = 0, lds_stride = 0;
};
NvMatrixPlan nv_matrix_make_plan(uint32_t max_p, uint32_t max_t, bool per_pair_text) {
    NvMatrixPlan P;
    P.lds_stride = (std::max<uint32_t>(max_t, 1) + 7u) & ~7u;
    for (; P.shape < (int)kNvShapeCount; P.shape++) {
        const NvShape &sh = kNvShapes[P.shape];
        P.per_block = 4 * (64 / sh.G);
        P.lds = kNvMatrixBytes + (size_t)P.lds_stride * (per_pair_text ? P.per_block : 1);
        if ((uint32_t)(sh.G * sh.R) >= max_p && P.lds <= kNvLdsMax) { P.ok = true; break; }
    }
    return P;
}

// the checks that need no strings: the aligner, then the table's size
int nv_matrix_check(const gasalx_nv_aligner &al, uint32_t matrix_n) {
    if (al.aligner < 0 || al.aligner > 2 || al.type < 0 || al.type > 2) return nv_fail(GASALX_EINVAL, "bad aligner");
    if (al.aligner != NV_GOTOH)
        return nv_fail(GASALX_EUNSUPPORTED, "only the Gotoh aligner takes a substitution matrix");
    if (matrix_n < 2 || matrix_n > kNvMatrixDim) return nv_fail(GASALX_EINVAL, "matrix size must be 2..32");
    return GASALX_OK;
}

// The caller's table (scores[t + p * n]) as the kernels' 32 x 32 image (tab[32 * p + t], zero outside
// the n x n corner); returns the largest |entry|.
int32_t nv_matrix_image(const gasalx_nv_matrix &mat, uint32_t (&tab)[kNvMatrixBytes / 4]) {
    int8_t image[kNvMatrixBytes] = {};
    int32_t entry_mag = 0;
    for (uint32_t p = 0; p < mat.n; p++)
        for (uint32_t t = 0; t < mat.n; t++) {
            const int8_t v = mat.scores[t + p * mat.n];
            image[p * kNvMatrixDim + t] = v;
            entry_mag = std::max(entry_mag, std::abs((int32_t)v));
        }
    std::memcpy(tab, image, sizeof(image));
    return entry_mag;
}

using NvMatrixFn = void (*)(NvMatrixArgs);
NvMatrixFn nv_matrix_lookup(int type, bool sink, int shape) {
    return nv_instance(NV_GOTOH, type, sink, shape, [](auto, auto t, auto s, auto g, auto r) -> NvMatrixFn {
        return &nv_matrix_kernel<t, g, r, s>; });
}

}  // namespace

int nv_matrix_plan_name(const gasalx_nv_aligner &al, uint32_t matrix_n, uint32_t max_p, uint32_t max_t,
                        bool per_pair_text, bool sinks, std::string &name) {
    static const char *tn[] = {"global", "local", "semi"};
    if (int rc = nv_matrix_check(al, matrix_n)) return rc;
    const NvMatrixPlan P = nv_matrix_make_plan(max_p, max_t, per_pair_text);
    name = !P.ok ? "none"
                 : std::string("nvbio_matrix_gotoh_") + tn[al.type] + (per_pair_text ? "" : "_shared") + "_G" +
                       std::to_string(kNvShapes[P.shape].G) + "R" + std::to_string(kNvShapes[P.shape].R) +
                       (sinks ? "_sink" : "");
    return GASALX_OK;
}

int nv_matrix_score_device(const gasalx_nv_aligner &al, const gasalx_nv_matrix &mat, uint32_t n,
                           const gasalx_nv_strings &pat, const gasalx_nv_strings &txt, int32_t *scores, uint32_t *sinks,
                           uint32_t max_p, uint32_t max_t, hipStream_t st) {
    if (int rc = nv_matrix_check(al, mat.n)) return rc;
    if (!mat.scores) return nv_fail(GASALX_EINVAL, "null argument");
    if (int rc = nv_check(al, "bad aligner", "bad aligner", nullptr, pat, txt)) return rc;
    if (n == 0) return GASALX_OK;
    if (int rc = nv_check_ptrs(pat, txt, scores || sinks)) return rc;
    if (!txt.offsets) max_t = txt.length;
    // the table's image, by value in the arguments: read now, no device copy to reuse across streams
    NvMatrixArgs A;
    const int32_t entry_mag = nv_matrix_image(mat, A.tab);
    // nv_score_plan's range check, the largest |entry| standing for match and mismatch
    const NvScheme s = {entry_mag, entry_mag, al.gap_open, al.gap_ext, al.deletion, al.insertion};
    if ((int64_t)(max_p + max_t + 2) * nv_score_mag(s) * 2 >= (1ll << 28))
        return nv_fail(GASALX_ERANGE, "scores out of the exact range");
    const NvMatrixPlan P = nv_matrix_make_plan(max_p, max_t, txt.offsets != nullptr);
    if (!P.ok)
        return nv_fail(GASALX_ERANGE, "pattern longer than 1024 or text too long for LDS (" + std::to_string(max_p) +
                                          ", " + std::to_string(max_t) + ")");
    nv_fill_strings(A, pat, txt, n);
    A.score = scores; A.sinks = sinks; A.go = al.gap_open; A.ge = al.gap_ext;
    A.lds_stride = P.lds_stride; A.nsym = mat.n;
    return launch_checked(nv_matrix_lookup(al.type, sinks != nullptr, P.shape), (n + P.per_block - 1) / P.per_block,
                          P.lds, st, A);
}

// ---- BatchedBandedAlignmentScore<band> (nvbanded.hpp): thread per pair, band in registers,
//      instances for bands up to 8, 16 and 32; a band length of an instance's own size takes the
//      EX instance, whose slot tests fold ----
#define GX_BAND_PICK(K, a, t, ex) (band <= 8 ? &K<a, t, 8, ex> : band <= 16 ? &K<a, t, 16, ex> : &K<a, t, 32, ex>)

int nv_banded_score_device(const gasalx_nv_aligner &al, uint32_t band, uint32_t n, const gasalx_nv_strings &pat,
                           const gasalx_nv_strings &txt, int32_t *scores, hipStream_t st, uint32_t max_p) {
    if (int rc = nv_check(al, "bad aligner", "bad aligner", &band, pat, txt)) return rc;
    if (n == 0) return GASALX_OK;
    if (int rc = nv_check_ptrs(pat, txt, scores)) return rc;
    const NvScheme s = nv_scheme(al);
    const bool ex = band == 8 || band == 16 || band == 32;
    uint32_t base = 0;
    if (max_p && nvb16_ok(s, txt.bits, max_p, band, &base)) {
        NvBand16Args D;
        nv_fill(D, pat, txt, s, n);
        D.score = scores; D.n_lanes = (n + 1) / 2; D.band = band; D.base = base;
        using Fn = void (*)(NvBand16Args);
        const Fn fn = nv_static(al.aligner, al.type, ex, [band](auto a, auto t, auto e) -> Fn {
            return GX_BAND_PICK(nv_banded16_kernel, a, t, e); });
        return launch_checked(fn, (D.n_lanes + 255) / 256, st, D);
    }
    NvBandArgs A;
    nv_fill(A, pat, txt, s, n);
    A.score = scores; A.band = band;
    using Fn = void (*)(NvBandArgs);
    const Fn fn = nv_static(al.aligner, al.type, ex, [band](auto a, auto t, auto e) -> Fn {
        return GX_BAND_PICK(nv_banded_kernel, a, t, e); });
    return launch_checked(fn, (n + 255) / 256, st, A);
}

// ---- The same scorer with the BestSink position (nvbanded_sink.hpp).  nv_banded_score_device's
//      checks in its order and its choice of family: the packed kernel inside nvb16_ok's
//      conditions, the int32 kernel otherwise, at the same BMAX; "_sink" marks the name. ----
int nv_banded_sinks_plan_name(const gasalx_nv_aligner &al, uint32_t band, uint32_t max_p, uint32_t text_bits,
                              std::string &name) {
    static const char *an[] = {"ed", "sw", "gotoh"}, *tn[] = {"global", "local", "semi"};
    const gasalx_nv_strings pat = {nullptr, nullptr, 0, 2, 0}, txt = {nullptr, nullptr, 0, text_bits, 0};
    if (int rc = nv_check(al, "bad aligner", "bad aligner", &band, pat, txt)) return rc;
    uint32_t base = 0;
    const bool packed = max_p && nvb16_ok(nv_scheme(al), text_bits, max_p, band, &base);
    name = std::string(packed ? "nvbio_banded16_" : "nvbio_banded_") + an[al.aligner] + "_" + tn[al.type] + "_b" +
           std::to_string(band <= 8 ? 8 : band <= 16 ? 16 : 32) + "_sink";
    return GASALX_OK;
}

int nv_banded_score_sinks_device(const gasalx_nv_aligner &al, uint32_t band, uint32_t n, const gasalx_nv_strings &pat,
                                 const gasalx_nv_strings &txt, int32_t *scores, uint32_t *sinks, hipStream_t st,
                                 uint32_t max_p) {
    if (int rc = nv_check(al, "bad aligner", "bad aligner", &band, pat, txt)) return rc;
    if (n == 0) return GASALX_OK;
    if (int rc = nv_check_ptrs(pat, txt, scores || sinks)) return rc;
    const NvScheme s = nv_scheme(al);
    const bool ex = band == 8 || band == 16 || band == 32;
    uint32_t base = 0;
    if (max_p && nvb16_ok(s, txt.bits, max_p, band, &base)) {
        NvBand16SinkArgs D;
        nv_fill(D.a, pat, txt, s, n);
        D.a.score = scores; D.a.n_lanes = (n + 1) / 2; D.a.band = band; D.a.base = base; D.sinks = sinks;
        using Fn = void (*)(NvBand16SinkArgs);
        const Fn fn = nv_static(al.aligner, al.type, ex, [band](auto a, auto t, auto e) -> Fn {
            return GX_BAND_PICK(nv_banded16_sink_kernel, a, t, e); });
        return launch_checked(fn, (D.a.n_lanes + 255) / 256, st, D);
    }
    NvBandSinkArgs A;
    nv_fill(A.a, pat, txt, s, n);
    A.a.score = scores; A.a.band = band; A.sinks = sinks;
    using Fn = void (*)(NvBandSinkArgs);
    const Fn fn = nv_static(al.aligner, al.type, ex, [band](auto a, auto t, auto e) -> Fn {
        return GX_BAND_PICK(nv_banded_sink_kernel, a, t, e); });
    return launch_checked(fn, (n + 255) / 256, st, A);
}

// ---- EditDistanceAligner<TYPE, MyersTag<ALPHABET>> under BatchedBandedAlignmentScore<band>
//      (nvmyers.hpp): thread per pair, one instance per type and alphabet, the band length a
//      launch argument.  The checks of nv_banded_score_device in its order, then the alphabet;
//      LOCAL, which the reference's function does not have, is refused last. ----
static int nv_myers_check(int32_t type, uint32_t alphabet, uint32_t band, const gasalx_nv_strings &pat,
                   const gasalx_nv_strings &txt) {
    const gasalx_nv_aligner al = {NV_ED, type, 0, -1, 0, 0, -1, -1};
    if (int rc = nv_check(al, "bad aligner", "bad aligner", &band, pat, txt)) return rc;
    if (alphabet != 2 && alphabet != 4 && alphabet != 5) return nv_fail(GASALX_EINVAL, "alphabet size must be 2, 4 or 5");
    if (type == NV_LOCAL) return nv_fail(GASALX_EUNSUPPORTED, "banded Myers has no LOCAL form");
    return GASALX_OK;
}

int nv_myers_plan_name(int32_t type, uint32_t alphabet, uint32_t band, std::string &name) {
    const gasalx_nv_strings any = {nullptr, nullptr, 0, 2, 0};
    if (int rc = nv_myers_check(type, alphabet, band, any, any)) return rc;
    name = std::string("nvbio_myers_") + (type == NV_GLOBAL ? "global" : "semi") + "_a" + std::to_string(alphabet);
    return GASALX_OK;
}

int nv_banded_myers_device(int32_t type, uint32_t alphabet, uint32_t band, uint32_t n, const gasalx_nv_strings &pat,
                           const gasalx_nv_strings &txt, int32_t *scores, uint32_t *sinks, hipStream_t st) {
    if (int rc = nv_myers_check(type, alphabet, band, pat, txt)) return rc;
    if (n == 0) return GASALX_OK;
    if (int rc = nv_check_ptrs(pat, txt, scores || sinks)) return rc;
    NvMyersArgs A;
    nv_fill_strings(A, pat, txt, n);
    A.score = scores; A.sinks = sinks; A.band = band;
    using Fn = void (*)(NvMyersArgs);
    auto by_alphabet = [alphabet](auto t) -> Fn {
        return alphabet == 2 ? &nv_myers_kernel<t, 2> : alphabet == 4 ? &nv_myers_kernel<t, 4> : &nv_myers_kernel<t, 5>;
    };
    const Fn fn = type == NV_GLOBAL ? by_alphabet(ic<NV_GLOBAL>{}) : by_alphabet(ic<NV_SEMI>{});
    return launch_checked(fn, (n + 255) / 256, st, A);
}

// nvbio BatchedAlignmentTraceback (nvtrace.hpp): one pair per thread, flags and the previous row in
// the caller's workspace (dir: pad8(max_p) * max_t bytes per pair, row: max_t int2 per pair)
int nv_traceback_device(const gasalx_nv_aligner &al, uint32_t n, const gasalx_nv_strings &pat,
                        const gasalx_nv_strings &txt, uint32_t max_p, uint32_t max_t, uint8_t *dir, int32_t *row,
                        int32_t *score, uint32_t *src, uint32_t *snk, uint8_t *ops, uint32_t ops_stride,
                        uint32_t *n_ops, hipStream_t st) {
    if (int rc = nv_check(al, "traceback: unknown aligner", "bad alignment type", nullptr, pat, txt)) return rc;
    if (n == 0) return GASALX_OK;
    if (int rc = nv_check_ptrs(pat, txt, score && src && snk && ops && n_ops && dir && row)) return rc;
    NvTbArgs A;
    nv_fill(A, pat, txt, nv_scheme(al), n);
    A.max_m = max_p; A.max_n = max_t;
    A.dir = dir; A.row = row; A.score = score; A.src = src; A.snk = snk; A.ops = ops; A.ops_stride = ops_stride;
    A.n_ops = n_ops;
    using Fn = void (*)(NvTbArgs);
    const Fn fn = nv_static(al.aligner, al.type, false, [](auto a, auto t, auto) -> Fn {
        return &nv_traceback_kernel<a == NV_GOTOH, t>; });
    return launch_checked(fn, (n + 255) / 256, st, A);
}

// The same traceback of a GotohAligner over a substitution matrix (nvmatrix_trace.hpp): the checks
// that need no lengths, in the entry points' order (the aligner and the table's size, the table,
// the symbol bits), and the largest |entry|, which stands for match and mismatch in the range rule
int nv_matrix_traceback_check(const gasalx_nv_aligner &al, const gasalx_nv_matrix &mat, const gasalx_nv_strings &pat,
                              const gasalx_nv_strings &txt, int32_t *entry_mag) {
    if (int rc = nv_matrix_check(al, mat.n)) return rc;
    if (!mat.scores) return nv_fail(GASALX_EINVAL, "null argument");
    if (int rc = nv_check(al, "bad aligner", "bad aligner", nullptr, pat, txt)) return rc;
    if (entry_mag) {
        uint32_t tab[kNvMatrixBytes / 4];
        *entry_mag = nv_matrix_image(mat, tab);
    }
    return GASALX_OK;
}

// Workspace and outputs as nv_traceback_device; one instance per type, named
// nvbio_matrix_traceback_gotoh_<global|local|semi> in traces.  The table is read now.
int nv_matrix_traceback_device(const gasalx_nv_aligner &al, const gasalx_nv_matrix &mat, uint32_t n,
                               const gasalx_nv_strings &pat, const gasalx_nv_strings &txt, uint32_t max_p,
                               uint32_t max_t, uint8_t *dir, int32_t *row, int32_t *score, uint32_t *src,
                               uint32_t *snk, uint8_t *ops, uint32_t ops_stride, uint32_t *n_ops, hipStream_t st) {
    if (int rc = nv_matrix_traceback_check(al, mat, pat, txt, nullptr)) return rc;
    if (n == 0) return GASALX_OK;
    if (int rc = nv_check_ptrs(pat, txt, score && src && snk && ops && n_ops && dir && row)) return rc;
    NvMatrixTbArgs B;
    nv_matrix_image(mat, B.tab);
    B.nsym = mat.n;
    NvTbArgs &A = B.t;
    nv_fill(A, pat, txt, NvScheme{0, 0, al.gap_open, al.gap_ext, 0, 0}, n);
    A.max_m = max_p; A.max_n = max_t;
    A.dir = dir; A.row = row; A.score = score; A.src = src; A.snk = snk; A.ops = ops; A.ops_stride = ops_stride;
    A.n_ops = n_ops;
    using Fn = void (*)(NvMatrixTbArgs);
    const Fn fn = nv_static(NV_GOTOH, al.type, false, [](auto, auto t, auto) -> Fn {
        return &nv_matrix_traceback_kernel<t>; });
    return launch_checked(fn, (n + 255) / 256, st, B);
}

// BatchedBandedAlignmentTraceback<band> (nvtrace.hpp nv_banded_traceback_kernel); ED runs as
// SW with EditDistanceSWScheme (ed_banded_inl.h:175-295).  The band's register arrays come in
// 8, 16 and 32 cells with the band length as a kernel argument, and exactly 7, 15 and 31 cells
// (nvBowtie's BAND_LEN values, traceback_inl.h:239-257) with the length folded in.
int nv_banded_traceback_device(const gasalx_nv_aligner &al, uint32_t band, uint32_t n, const gasalx_nv_strings &pat,
                               const gasalx_nv_strings &txt, uint32_t max_p, uint32_t *dir, int32_t *score,
                               uint32_t *src, uint32_t *snk, uint8_t *ops, uint32_t ops_stride, uint32_t *n_ops,
                               hipStream_t st) {
    if (int rc = nv_check(al, "banded traceback: unknown aligner", "bad alignment type", &band, pat, txt)) return rc;
    if (n == 0) return GASALX_OK;
    if (int rc = nv_check_ptrs(pat, txt, score && src && snk && ops && n_ops && dir)) return rc;
    NvBandTbArgs A;
    nv_fill(A, pat, txt, nv_scheme(al), n);
    A.band = band; A.words = (band + 3) / 4; A.max_m = max_p;
    A.dir = dir; A.score = score; A.src = src; A.snk = snk; A.ops = ops; A.ops_stride = ops_stride; A.n_ops = n_ops;
    using Fn = void (*)(NvBandTbArgs);
    const bool exact = band == 7 || band == 15 || band == 31;
    const Fn fn = nv_static(al.aligner, al.type, exact, [band](auto a, auto t, auto ex) -> Fn {
        constexpr bool g = a == NV_GOTOH;
        if constexpr (ex)
            return band == 7 ? &nv_banded_traceback_kernel<g, t, 7, true>
                 : band == 15 ? &nv_banded_traceback_kernel<g, t, 15, true> : &nv_banded_traceback_kernel<g, t, 31, true>;
        else
            return GX_BAND_PICK(nv_banded_traceback_kernel, g, t, false);
    });
    return launch_checked(fn, (n + 255) / 256, st, A);
}
#undef GX_BAND_PICK

// ---- The banded Gotoh kernels under a quality-aware scheme (nvbanded_qual.hpp): the scorer with
//      sinks, packed or int32 by nvb16_ok's rule over the tables' extremes, and the banded traceback
//      with its exact 7 / 15 / 31 instances.  Both families make their checks in nv_qual_check. ----
namespace {

// the two tables as the kernels read them, and what the planner and the range rules need of them
struct NvQualPlan {
    NvQualTable tab;
    int32_t max_match = 0, min_mismatch = 0, entry_mag = 0;
    bool byte_steps = true;   // at every level match >= mismatch and match - mismatch <= 255
};

// The checks both families share, in the order gasalx.h states: the struct and its tables (the
// quality bytes too where a call reads them), the aligner and type, the Gotoh aligner alone, the
// number of levels, the band, the symbol bits.  The range rules follow in the callers.
int nv_qual_check(const gasalx_nv_aligner &al, const gasalx_nv_quals *q, bool bytes, uint32_t band,
                  const gasalx_nv_strings &pat, const gasalx_nv_strings &txt, NvQualPlan &P) {
    if (!q || !q->match || !q->mismatch || (bytes && !q->quals)) return nv_fail(GASALX_EINVAL, "null argument");
    if (al.aligner < 0 || al.aligner > 2 || al.type < 0 || al.type > 2) return nv_fail(GASALX_EINVAL, "bad aligner");
    if (al.aligner != NV_GOTOH)
        return nv_fail(GASALX_EUNSUPPORTED, "only the Gotoh aligner scores with qualities: edit distance has no scheme, "
                                            "and nothing in the tree drives Smith-Waterman with qualities");
    if (q->levels < 1 || q->levels > kNvQualLevels) return nv_fail(GASALX_EINVAL, "quality levels must be 1..256");
    if (int rc = nv_check(al, "bad aligner", "bad aligner", &band, pat, txt)) return rc;
    P.max_match = q->match[0]; P.min_mismatch = q->mismatch[0];
    for (uint32_t b = 0; b < kNvQualLevels; b++) {
        const uint32_t l = std::min(b, q->levels - 1);   // a quality byte >= levels reads the last entry
        const int32_t m = q->match[l], x = q->mismatch[l];
        P.tab.tab[b] = (uint32_t)(uint16_t)m | ((uint32_t)(uint16_t)x << 16);
        P.max_match = std::max(P.max_match, m); P.min_mismatch = std::min(P.min_mismatch, x);
        P.entry_mag = std::max({P.entry_mag, std::abs(m), std::abs(x)});
        if (m < x || m - x > 255) P.byte_steps = false;
    }
    return GASALX_OK;
}

// the packed kernel: nvb16_ok with the largest match and the smallest mismatch (every entry lies
// between them when each level has match >= mismatch), and a step that fits a byte at every level
bool nvq16_ok(const gasalx_nv_aligner &al, const NvQualPlan &P, uint32_t text_bits, uint32_t max_p, uint32_t band,
              uint32_t *base) {
    const NvScheme s = {P.max_match, P.min_mismatch, al.gap_open, al.gap_ext, al.deletion, al.insertion};
    return max_p && P.byte_steps && nvb16_ok(s, text_bits, max_p, band, base);
}

}  // namespace

int nv_banded_qual_check(const gasalx_nv_aligner &al, const gasalx_nv_quals *q, bool bytes, uint32_t band,
                         const gasalx_nv_strings &pat, const gasalx_nv_strings &txt, int32_t *entry_mag) {
    NvQualPlan P;
    if (int rc = nv_qual_check(al, q, bytes, band, pat, txt, P)) return rc;
    if (entry_mag) *entry_mag = P.entry_mag;
    return GASALX_OK;
}

int nv_banded_qual_plan_name(const gasalx_nv_aligner &al, const gasalx_nv_quals *q, uint32_t band, uint32_t max_p,
                             uint32_t text_bits, bool traceback, std::string &name) {
    static const char *tn[] = {"global", "local", "semi"};
    const gasalx_nv_strings pat = {nullptr, nullptr, 0, 2, 0}, txt = {nullptr, nullptr, 0, text_bits, 0};
    NvQualPlan P;
    if (int rc = nv_qual_check(al, q, false, band, pat, txt, P)) return rc;
    if (traceback) {
        const bool exact = band == 7 || band == 15 || band == 31;
        name = std::string("nvbio_banded_qual_traceback_gotoh_") + tn[al.type] + "_b" +
               std::to_string(exact ? band : band <= 8 ? 8 : band <= 16 ? 16 : 32);
        return GASALX_OK;
    }
    uint32_t base = 0;
    name = std::string(nvq16_ok(al, P, text_bits, max_p, band, &base) ? "nvbio_banded16_qual_gotoh_" : "nvbio_banded_qual_gotoh_") +
           tn[al.type] + "_b" + std::to_string(band <= 8 ? 8 : band <= 16 ? 16 : 32) + "_sink";
    return GASALX_OK;
}

#define GX_QBAND_PICK(K, t, ex) (band <= 8 ? &K<t, 8, ex> : band <= 16 ? &K<t, 16, ex> : &K<t, 32, ex>)

int nv_banded_qual_score_device(const gasalx_nv_aligner &al, const gasalx_nv_quals *q, uint32_t band, uint32_t n,
                                const gasalx_nv_strings &pat, const gasalx_nv_strings &txt, int32_t *scores,
                                uint32_t *sinks, hipStream_t st, uint32_t max_p) {
    NvQualPlan P;
    if (int rc = nv_qual_check(al, q, true, band, pat, txt, P)) return rc;
    if (n == 0) return GASALX_OK;
    if (int rc = nv_check_ptrs(pat, txt, scores || sinks)) return rc;
    const NvScheme s = {0, 0, al.gap_open, al.gap_ext, al.deletion, al.insertion};   // match / mismatch: the tables
    const bool ex = band == 8 || band == 16 || band == 32;
    uint32_t base = 0;
    if (nvq16_ok(al, P, txt.bits, max_p, band, &base)) {
        NvBand16QualArgs D;
        nv_fill(D.s.a, pat, txt, s, n);
        D.s.a.score = scores; D.s.a.n_lanes = (n + 1) / 2; D.s.a.band = band; D.s.a.base = base; D.s.sinks = sinks;
        D.quals = q->quals; D.q = P.tab;
        using Fn = void (*)(NvBand16QualArgs);
        const Fn fn = nv_static(NV_GOTOH, al.type, ex, [band](auto, auto t, auto e) -> Fn {
            return GX_QBAND_PICK(nv_banded16_qual_sink_kernel, t, e); });
        return launch_checked(fn, (D.s.a.n_lanes + 255) / 256, st, D);
    }
    NvBandQualArgs A;
    nv_fill(A.s.a, pat, txt, s, n);
    A.s.a.score = scores; A.s.a.band = band; A.s.sinks = sinks;
    A.quals = q->quals; A.q = P.tab;
    using Fn = void (*)(NvBandQualArgs);
    const Fn fn = nv_static(NV_GOTOH, al.type, ex, [band](auto, auto t, auto e) -> Fn {
        return GX_QBAND_PICK(nv_banded_qual_sink_kernel, t, e); });
    return launch_checked(fn, (n + 255) / 256, st, A);
}

// workspace and outputs as nv_banded_traceback_device
int nv_banded_qual_traceback_device(const gasalx_nv_aligner &al, const gasalx_nv_quals *q, uint32_t band, uint32_t n,
                                    const gasalx_nv_strings &pat, const gasalx_nv_strings &txt, uint32_t max_p,
                                    uint32_t *dir, int32_t *score, uint32_t *src, uint32_t *snk, uint8_t *ops,
                                    uint32_t ops_stride, uint32_t *n_ops, hipStream_t st) {
    NvQualPlan P;
    if (int rc = nv_qual_check(al, q, true, band, pat, txt, P)) return rc;
    if (n == 0) return GASALX_OK;
    if (int rc = nv_check_ptrs(pat, txt, score && src && snk && ops && n_ops && dir)) return rc;
    NvBandTbQualArgs B;
    NvBandTbArgs &A = B.t;
    nv_fill(A, pat, txt, NvScheme{0, 0, al.gap_open, al.gap_ext, 0, 0}, n);
    A.band = band; A.words = (band + 3) / 4; A.max_m = max_p;
    A.dir = dir; A.score = score; A.src = src; A.snk = snk; A.ops = ops; A.ops_stride = ops_stride; A.n_ops = n_ops;
    B.quals = q->quals; B.q = P.tab;
    using Fn = void (*)(NvBandTbQualArgs);
    const bool exact = band == 7 || band == 15 || band == 31;
    const Fn fn = nv_static(NV_GOTOH, al.type, exact, [band](auto, auto t, auto ex) -> Fn {
        if constexpr (ex)
            return band == 7 ? &nv_banded_qual_traceback_kernel<t, 7, true>
                 : band == 15 ? &nv_banded_qual_traceback_kernel<t, 15, true> : &nv_banded_qual_traceback_kernel<t, 31, true>;
        else
            return GX_QBAND_PICK(nv_banded_qual_traceback_kernel, t, false);
    });
    return launch_checked(fn, (n + 255) / 256, st, B);
}
#undef GX_QBAND_PICK

}  // namespace gx
