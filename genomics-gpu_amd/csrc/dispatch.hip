// dispatch.hip — kernel instantiation table and the flat host dispatcher.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "banded16.hpp"
#include "local16.hpp"
#include "engine.hpp"
#include "generic.hpp"
#include "pairhmm.hpp"
#include "ksw16.hpp"
#include "plan.hpp"
#include "start.hpp"
#include "wavefront.hpp"
#include "wavefront16.hpp"

namespace gx {

static thread_local std::string g_last_error;
void set_error(const std::string &msg) { g_last_error = msg; }
const char *last_error() { return g_last_error.c_str(); }

hipError_t DevBuf::reserve(size_t need) {
    if (need <= bytes && p) return hipSuccess;
    release();
    size_t cap = std::max<size_t>(need, 256);
    hipError_t e = hipMalloc(&p, cap);
    if (e != hipSuccess) { p = nullptr; bytes = 0; return e; }
    bytes = cap;
    return hipSuccess;
}
void DevBuf::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
}
void Workspace::release_all() {
    for (DevBuf *b : {&packed_q, &packed_t, &tb, &rows_h, &rows_e, &rev, &ends_q, &ends_t, &misc, &aux,
                      &rev_meta, &sort_meta, &band_cp, &band_stm, &band_fl, &band_fb, &kseg}) b->release();
}

using WfFn = void (*)(WfArgs);

// the int32 kernel's instances (STOP: the SEMI TAIL=TARGET reverse pass, start.hpp)
template <int ALGO, bool KEYS, bool TB, bool STOP = false>
struct WfK {
    template <int G, int R> static WfFn fn() { return &wf_kernel<ALGO, KEYS, TB, G, R, STOP>; }
};
template <int ALGO, bool KEYS, bool TB>
static WfFn wf_pick(int G, int R) { return pick_instance<WfK<ALGO, KEYS, TB>, SHAPES_R4>(G, R); }
template <int ALGO>
static WfFn wf16_pick(int G, int R) { return pick_instance<Wf16K<ALGO>, SHAPES_PK>(G, R); }
// R % 4 == 0 shapes: the packed kernels that store in groups of 4 rows (traceback flags, band windows)
template <int ALGO>
static WfFn wf16_pick_r4(int G, int R) { return pick_instance<Wf16K<ALGO>, SHAPES_R4>(G, R); }

static WfFn wf_lookup(int algo, bool keys, bool tb, int G, int R) {
    if (algo == WF_LOCAL) return tb ? wf_pick<WF_LOCAL, true, true>(G, R) : wf_pick<WF_LOCAL, true, false>(G, R);
    if (algo == WF_GLOBAL) return tb ? wf_pick<WF_GLOBAL, false, true>(G, R) : wf_pick<WF_GLOBAL, false, false>(G, R);
    return keys ? wf_pick<WF_SEMI, true, false>(G, R) : wf_pick<WF_SEMI, false, false>(G, R);
}

// which packed kernel of an algo a launch takes
struct Wf16Variant {
    bool tb = false;     // traceback flags
    bool tbd = false;    // LOCAL + traceback in the e-drift frame (WF16_LOCAL_TBD)
    bool key2 = false;   // LOCAL: second key set (WF16_LOCAL_K2)
    bool ku16 = false;   // LOCAL e-drift: u16 keys
    bool lrs = false;    // LOCAL e-drift: the WITH_START reverse pass (lstop)
    bool kseg = false;   // LOCAL e-drift: keys by step segments
    bool stop = false;   // SEMI TAIL=TARGET reverse pass
};
static WfFn wf16_lookup(int algo, int G, int R, const Wf16Variant &v) {
    if (algo == WF_LOCAL) return v.tb ? (v.tbd ? wf16_pick_r4<WF16_LOCAL_TBD>(G, R) : wf16_pick_r4<WF16_LOCAL_TB>(G, R))
                               : v.key2 ? wf16_pick<WF16_LOCAL_K2>(G, R)
                               : (v.ku16 || v.lrs || v.kseg) ? wf16_local_lookup(G, R, v.ku16, v.lrs, v.kseg)
                                                             : wf16_pick<WF_LOCAL>(G, R);
    if (algo == WF_GLOBAL) return v.tb ? wf16_pick_r4<WF16_GLOBAL_TB>(G, R) : wf16_pick<WF_GLOBAL>(G, R);
    return v.stop ? wf16_pick<WF16_SEMI_STOP>(G, R) : wf16_pick<WF_SEMI>(G, R);
}

#define HIPCHK(x)                                                                        \
    do {                                                                                 \
        hipError_t e__ = (x);                                                            \
        if (e__ != hipSuccess) {                                                         \
            set_error(std::string(#x) + ": " + hipGetErrorString(e__));                  \
            return GASALX_EDEVICE;                                                       \
        }                                                                                \
    } while (0)

static int grid_for(uint32_t n, uint32_t per_block) { return (int)((n + per_block - 1) / per_block); }
// the int32 wavefront kernel's grid: every block, or, as the fallback of a packed launch (A.skip:
// usually few or no declined blocks), at most 8 blocks per CU walking the rest (wavefront.hpp wf_kernel)
static int wf_grid(uint32_t n, int G, bool fallback) {
    const int g = grid_for(n, kWavesPerBlock * (64 / G));
    return fallback ? std::min(g, 8 * 256) : g;
}

// Device-to-device byte copy, 16 bytes per lane (the CIGAR buffer's start as the query batch,
// get_tb.h:94): the runtime's copy ran at ≈0.4 TB/s for the config-3 batch (30 MB, 80 us
// under the two-stream bench, profiles/r04_nw_tb_kernel_stats.csv).  Both pointers 16-byte
// aligned, else the runtime copy.
__global__ __launch_bounds__(256) void copy16_kernel(uint4 *dst, const uint4 *src, uint64_t n16) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * 256) dst[i] = src[i];
}
static hipError_t copy_d2d(void *dst, const void *src, size_t bytes, hipStream_t st) {
    if (((uintptr_t)dst | (uintptr_t)src) & 15u || bytes < 4096)
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
    const uint64_t n16 = bytes / 16;
    copy16_kernel<<<(int)std::min<uint64_t>((n16 + 255) / 256, 8192), 256, 0, st>>>((uint4 *)dst, (const uint4 *)src, n16);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && bytes % 16)
        e = hipMemcpyAsync((uint8_t *)dst + n16 * 16, (const uint8_t *)src + n16 * 16, bytes % 16, hipMemcpyDeviceToDevice, st);
    return e;
}

// The short second shape of a packed score launch (wf16_mix_kernel): more lanes per pair and
// fewer rows per lane, a wave a third as long, over the launch's last slots.  Taken for the
// score plans it is instantiated for (LOCAL in the e-drift frame with f16 keys at G8R19, 150 bp:
// config 2; GLOBAL score at G16R20, 300 bp), when the launch holds at least two rounds of its
// waves and the value window and key range also hold for the second shape's span.  The slots
// past the last whole round of long waves (GASALX_TAIL_K more rounds: 0 by default) take it;
// GASALX_TAIL=0: one shape (A/B).
struct TailShape {
    WfFn fn = nullptr;
    int G2 = 0, R2 = 0;
    uint32_t b0 = 0, p0 = 0, ppb = 1, lds_stride = 0;
    size_t lds_bytes = 0;
    int32_t vmin = 0;   // GLOBAL: the value-window bound for the larger span of the two shapes
};
// launches that are one shape whatever the plan: the WITH_START reverse passes and the band
// traceback's fallback launches (their device-side count excludes the tail)
static bool one_shape_only(const WfArgs &A) { return A.rev || A.n_dev || A.stop || A.lstop; }

// the CU count of the workspace's device, asked once per workspace (256 when the query fails)
static int device_cus(Workspace &ws) {
    if (!ws.cus) (void)hipDeviceGetAttribute(&ws.cus, hipDeviceAttributeMultiprocessorCount, ws.device);
    return ws.cus > 0 ? ws.cus : 256;
}

// Evaluated once per call, for the main launch A over n pairs (run_wavefront): the launch, the band
// buffers and the walk all take this one answer.
static TailShape tail_shape(Workspace &ws, const Plan &pl, const gasalx_params &p, const WfArgs &A, uint32_t n) {
    TailShape t;
    // (read per call, so a test process can compare both)
    const bool on = env_flag("GASALX_TAIL", true);
    const int kextra = env_int("GASALX_TAIL_K", 0);
    if (!on || !pl.packed16 || (pl.tb && !pl.tb_band) || pl.key2 || pl.ku16 || pl.kseg_shift || pl.semi_tq ||
        one_shape_only(A))
        return t;
    int G2 = 0, R2 = 0;
    WfFn fn = nullptr;
    if (pl.wf_algo == WF_LOCAL && pl.kf16 && pl.G16 == 8 && pl.R16 == 19) {
        G2 = 32; R2 = 5; fn = &wf16_mix_kernel<WF_LOCAL, 8, 19, 32, 5>;
    } else if (pl.tb_band) {
        // the band traceback's sweep + band pass (R % 4 == 0 for the band windows); GASALX_CP_TAIL=32: G32R12
        if (pl.wf_algo != WF_GLOBAL || pl.G16 != 16 || pl.R16 != 20) return t;
        if (env_int("GASALX_CP_TAIL", 64) == 32) {
            G2 = 32; R2 = 12; fn = &wf16_mix_kernel<WF16_GLOBAL_CP, 16, 20, 32, 12>;
        } else {
            G2 = 64; R2 = 8; fn = &wf16_mix_kernel<WF16_GLOBAL_CP, 16, 20, 64, 8>;
        }
    } else if (pl.wf_algo == WF_GLOBAL && pl.G16 == 16 && pl.R16 == 20) {
        G2 = 64; R2 = 5; fn = &wf16_mix_kernel<WF_GLOBAL, 16, 20, 64, 5>;
    } else {
        return t;
    }
    const int64_t q8 = pad8(pl.max_q), y8 = pad8(pl.max_t);   // LOCAL / GLOBAL: the target is the step axis
    // the second shape's span and keys must fit the value window too (make_plan checked the first's)
    if (pl.wf_algo == WF_LOCAL) {
        const LocalDrift d = local_drift_frame(p, q8, y8, G2, R2);
        if (!(d.window && d.f16)) return t;
        t.vmin = pl.vmin;
    } else {
        // the window offset for the larger span serves both shapes: their values then sit higher
        // in the same window, whose top global_window checked for that span
        if (!global_window(p, q8, y8, std::max(packed_span(G2, R2, y8), packed_span(pl.G16, pl.R16, y8)), &t.vmin))
            return t;
        t.vmin = std::max(t.vmin, pl.vmin);
    }
    const uint64_t slots = (uint64_t)wf16_waves(pl.wf_algo, pl.R16) * 4 * device_cus(ws);
    const uint32_t ppw = pairs_per_wave(pl.G16), ppb = pairs_per_block(pl.G16);
    const uint64_t waves = (n + ppw - 1) / ppw;
    const uint64_t rounds = waves / slots;
    if (rounds < 2 + (uint64_t)std::max(kextra, 0)) return t;
    const uint64_t long_waves = (rounds - (uint64_t)std::max(kextra, 0)) * slots;
    t.b0 = (uint32_t)(long_waves / kWavesPerBlock);
    t.p0 = t.b0 * ppb;
    if (t.p0 >= n) return TailShape();
    t.ppb = pairs_per_block(G2);
    t.lds_stride = packed_lds_stride((uint32_t)y8, G2);
    t.lds_bytes = packed_lds_bytes((uint32_t)y8, G2);
    t.fn = fn;
    t.G2 = G2;
    t.R2 = R2;
    return t;
}

// the scoring fields every argument struct of the DP kernels and the walk shares
template <class Args>
static void fill_scoring(Args &A, const gasalx_params &p) {
    A.a = p.match; A.b = p.mismatch; A.o = p.gap_open; A.e = p.gap_extend;
    A.nval = p.n_code & 0xF;
    A.has_npen = p.has_n_penalty; A.npen = p.n_penalty;
}
// what the wavefront launches of one plan share (the int32 kernel's; the packed copy overrides its own)
static void wf_common(WfArgs &A, const gasalx_params &p, const Plan &pl) {
    fill_scoring(A, p);
    A.head = p.head; A.tail = p.tail;
    A.lds_stride = pl.lds_stride;
    A.force_exact = (p.mismatch <= 0 || (p.has_n_penalty && p.n_penalty < 0)) ? 1 : 0;
    A.one = 0x00010001u;
}

// the int32 kernel over the blocks the packed launches declined (A.skip), or over every pair
static int launch_int32(const Plan &pl, WfFn fn, const WfArgs &A, hipStream_t st) {
    if (!fn) { set_error("no wavefront instance"); return GASALX_EUNSUPPORTED; }
    HIPCHK(launch_lds(fn, dim3(wf_grid(A.n, pl.G, A.skip != nullptr)), dim3(kBlock), pl.lds_bytes, st, A));
    return GASALX_OK;
}

#ifdef GX_WF16_STAMP
// Probe builds only (wavefront16.hpp GX_WF16_STAMP; never the library that is benchmarked): with
// GASALX_STAMP_OUT=FILE the packed launch's waves stamp their phases, and the call waits for the
// launch and writes the kStampWords words per wave to FILE (the last launch's; tools/stamp_summary.py reads it).
static hipError_t stamp_begin(uint32_t waves, unsigned long long **buf) {
    *buf = nullptr;
    if (!std::getenv("GASALX_STAMP_OUT")) return hipSuccess;
    hipError_t e = hipMalloc((void **)buf, (size_t)waves * kStampWords * 8);
    if (e == hipSuccess) e = hipMemset(*buf, 0, (size_t)waves * kStampWords * 8);
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(gx_wf16_stamp), buf, sizeof *buf);
    return e;
}
static hipError_t stamp_end(uint32_t waves, unsigned long long *buf, hipStream_t st) {
    if (!buf) return hipSuccess;
    std::vector<unsigned long long> h((size_t)waves * kStampWords);
    unsigned long long *none = nullptr;
    hipError_t e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(h.data(), buf, h.size() * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(gx_wf16_stamp), &none, sizeof none);
    (void)hipFree(buf);
    if (e == hipSuccess) {
        if (FILE *f = std::fopen(std::getenv("GASALX_STAMP_OUT"), "wb")) {
            std::fwrite(h.data(), 8, h.size(), f);
            std::fclose(f);
        }
    }
    return e;
}
#endif

// Launch the wavefront kernel(s) of plan `pl` over one device batch: the packed
// kernel first when the plan has one (it flags the blocks it aligned), then the
// int32 kernel, which aligns exactly the pairs of the declined blocks.  main_tail: the
// main launch's second shape (tail_shape), or none.
static int launch_wavefront(Workspace &ws, const Plan &pl, const gasalx_params &p, const WfArgs &base,
                            const TailShape &main_tail, hipStream_t st) {
    WfArgs A = base;
    const uint32_t n = A.n;
    wf_common(A, p, pl);
    if (pl.packed16) {
        // packed kernel first; it marks every block it aligned in ws.misc ...
        WfArgs P16 = A;
        P16.lds_stride = pl.lds16_stride;
        P16.fast16 = 1;
        P16.vmin = pl.vmin;
        P16.kf16 = pl.kf16;
        const uint32_t ppb16 = pairs_per_block(pl.G16);
        uint32_t grid16 = grid_for(n, ppb16);
        // the launch's last slots on a shorter shape (wavefront16.hpp wf16_mix_kernel), so that its
        // end is not a fraction of a round of long waves running alone; never for a reverse pass or
        // a fallback launch, whoever calls
        const TailShape tail = one_shape_only(A) ? TailShape() : main_tail;
        size_t lds16 = pl.lds16_bytes;
        if (tail.fn) {
            P16.tail_b0 = tail.b0; P16.tail_p0 = tail.p0; P16.tail_lds = tail.lds_stride;
            P16.vmin = tail.vmin;
            grid16 = tail.b0 + grid_for(n - tail.p0, tail.ppb);
            lds16 = std::max(lds16, tail.lds_bytes);
        }
        HIPCHK(ws.misc.reserve(grid16 + 64));
        P16.handled = ws.misc.as<uint8_t>();
        ws.pk_flags = grid16; ws.pk_ppb = ppb16; ws.pk_pairs = n;
        ws.pk_p1 = tail.fn ? tail.p0 : 0xFFFFFFFFu; ws.pk_b1 = tail.b0; ws.pk_ppb2 = tail.fn ? tail.ppb : 1;
        if (pl.tb) {
            HIPCHK(ws.aux.reserve((size_t)n * 4));
            P16.tbfix = ws.aux.as<int32_t>();
        }
        Wf16Variant v;
        v.tb = pl.tb; v.tbd = pl.tb && pl.kf16 != 0;
        v.key2 = pl.key2; v.ku16 = pl.ku16; v.kseg = pl.kseg_shift != 0;
        v.lrs = pl.wf_algo == WF_LOCAL && !pl.tb && !pl.key2 && A.lstop != nullptr && pl.kf16 != 0 && !pl.kseg_shift;
        v.stop = A.stop != nullptr;
        WfFn f16 = pl.semi_tb   ? wf16_semi_tb_lookup(pl.G16, pl.R16, pl.semi_heads)
                   : pl.tb_band ? wf16_pick_r4<WF16_GLOBAL_CP>(pl.G16, pl.R16)
                                : wf16_lookup(pl.wf_algo, pl.G16, pl.R16, v);
        // WITH_START reverse passes: the register axis sized per block (rclass.hip)
        if (A.rev && !pl.tb_band && (v.stop || v.lrs)) {
            const int ra = A.stop ? WF16_SEMI_STOP : pl.ku16 ? WF16_LOCAL_U16_RS : WF16_LOCAL_RS;
            if (WfFn rc = wf16_rclass_lookup(ra, pl.G16, pl.R16)) f16 = rc;
        }
        if (pl.kseg_shift) {
            // the finished segments' keys per wave: saves at steps M, 2M, ... < nsteps <= C + G - 1
            const uint32_t nsave = std::max<uint32_t>(1u, (pl.kf16 + (uint32_t)pl.G16 - 2u) >> pl.kseg_shift);
            const uint64_t waves = (uint64_t)grid16 * kWavesPerBlock;
            HIPCHK(ws.kseg.reserve(waves * nsave * (uint64_t)pl.R16 * 64 * 4 + 64));
            P16.kseg = ws.kseg.as<uint32_t>();
            P16.kseg_shift = pl.kseg_shift;
            P16.kseg_n = nsave;
        }
        if (tail.fn) f16 = tail.fn;
        if (!f16) { set_error("no packed wavefront instance"); return GASALX_EUNSUPPORTED; }
#ifdef GX_WF16_STAMP
        unsigned long long *stamps = nullptr;
        HIPCHK(stamp_begin(grid16 * kWavesPerBlock, &stamps));
#endif
        HIPCHK(launch_lds(f16, dim3(grid16), dim3(kBlock), lds16, st, P16));
#ifdef GX_WF16_STAMP
        HIPCHK(stamp_end(grid16 * kWavesPerBlock, stamps, st));
#endif
        // ... and the int32 kernel aligns the pairs of the blocks it declined
        A.skip = ws.misc.as<uint8_t>();
        A.skip_ppb = ppb16;
        A.skip_p1 = tail.fn ? tail.p0 : 0xFFFFFFFFu;
        A.skip_b1 = tail.b0;
        A.skip_ppb2 = tail.fn ? tail.ppb : 1;
    }
    // (the band path's int32 launch aligns its declined blocks without direction words: the walk sends
    // those pairs to the fallback list, whose launch writes them into the capped buffer)
    return launch_int32(pl, pl.semi_tb ? wf_semi_tb_lookup(pl.G, pl.R, pl.semi_heads)
                            : A.stop   ? pick_instance<WfK<WF_SEMI, true, false, true>, SHAPES_R4>(pl.G, pl.R)
                                       : wf_lookup(pl.wf_algo, pl.keys, pl.tb && !pl.tb_band, pl.G, pl.R), A, st);
}

// The counting sort's arrays in ws.sort_meta: perm[n], then (two) a second array of n words -- the
// inverse permutation, or the caller's keys --, then the histogram and the cursor, nkeys + 1 words
// each (sh bytes).  Keys are lengths, bucketed by their 8-base words (start.hpp REV_PLAIN: longest first).
struct SortMeta {
    uint32_t *perm, *second, *hist, *cursor;
    size_t sh;
};
static int sort_reserve(Workspace &ws, uint32_t n, uint32_t nkeys, bool two, SortMeta *m) {
    m->sh = (size_t)(nkeys + 1) * 4;
    HIPCHK(ws.sort_meta.reserve((size_t)n * (two ? 8 : 4) + 2 * m->sh + 64));
    m->perm = ws.sort_meta.as<uint32_t>();
    m->second = two ? m->perm + n : nullptr;
    m->hist = m->perm + (two ? 2 : 1) * (size_t)n;
    m->cursor = m->hist + nkeys + 1;
    return GASALX_OK;
}
static int sort_histogram(const SortMeta &m, const uint32_t *keys, uint32_t n, uint32_t nkeys, hipStream_t st) {
    HIPCHK(hipMemsetAsync(m.hist, 0, m.sh, st));
    rev_hist_kernel<<<sort_grid(n), 256, m.sh, st>>>(REV_PLAIN, keys, nullptr, n, nkeys, m.hist);
    HIPCHK(hipGetLastError());
    return GASALX_OK;
}
static int sort_scatter(const SortMeta &m, const uint32_t *keys, uint32_t n, uint32_t nkeys, uint32_t *inv,
                        hipStream_t st) {
    rev_scan_kernel<<<1, 256, 0, st>>>(m.hist, m.cursor, nkeys + 1);
    rev_scatter_kernel<<<sort_grid(n), 256, 2 * m.sh, st>>>(REV_PLAIN, keys, nullptr, n, nkeys, m.cursor, m.perm, inv);
    HIPCHK(hipGetLastError());
    return GASALX_OK;
}
// The whole sort of n slots by keys: *perm (slot -> pair) and, when wanted, *inv (pair -> slot).
static int counting_sort(Workspace &ws, const uint32_t *keys, uint32_t n, uint32_t nkeys, hipStream_t st,
                         bool want_inv, const uint32_t **perm, const uint32_t **inv) {
    SortMeta m;
    int rc = sort_reserve(ws, n, nkeys, want_inv, &m);
    if (!rc) rc = sort_histogram(m, keys, n, nkeys, st);
    if (!rc) rc = sort_scatter(m, keys, n, nkeys, m.second, st);
    if (rc) return rc;
    *perm = m.perm;
    if (want_inv) *inv = m.second;
    return GASALX_OK;
}

// SEMI TAIL=QUERY/BOTH, packed (wavefront16.hpp WF16_SEMI_TQ): one launch per class of
// pairs with the same padded target length 8R, over a slot range (slots sorted by target
// words when the batch holds more than one class; the class sizes are read back, one
// synchronisation of the stream), flags per slot; then the int32 kernel over the slots
// the packed launches declined.
static int launch_semi_tq(Workspace &ws, const Plan &pl, const gasalx_params &p, const WfArgs &base,
                          hipStream_t st, bool one_class) {
    WfArgs A = base;
    const uint32_t n = A.n;
    wf_common(A, p, pl);
    const uint32_t t8w = (uint32_t)pl.R16;                  // largest class
    SortMeta m;
    int rc = sort_reserve(ws, n, t8w, false, &m);
    if (rc) return rc;
    std::vector<uint32_t> h(t8w + 1, 0u);
    if (one_class) {
        h[0] = n;   // every pair in the largest class (host-side lengths, BatchShape::one_t8): no read-back
    } else {
        // the class sizes, read back: one synchronisation of the stream (gasalx.h, max_t_len)
        if ((rc = sort_histogram(m, A.tlen, n, t8w, st))) return rc;
        HIPCHK(hipMemcpyAsync(h.data(), m.hist, m.sh, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    int classes = 0;
    for (uint32_t b = 0; b <= t8w; b++) classes += h[b] != 0;
    A.perm = nullptr;
    if (classes > 1) {                                       // counting sort: longest targets first
        if ((rc = sort_scatter(m, A.tlen, n, t8w, nullptr, st))) return rc;
        A.perm = m.perm;
    }
    HIPCHK(ws.misc.reserve(n + 64));
    HIPCHK(hipMemsetAsync(ws.misc.p, 0, n, st));            // slots no class launch covers stay declined
    ws.pk_flags = n; ws.pk_ppb = 1; ws.pk_pairs = n;
    WfArgs P16 = A;
    P16.lds_stride = pl.lds16_stride;
    P16.fast16 = 1;
    P16.vmin = pl.vmin;
    P16.handled = ws.misc.as<uint8_t>();
    const uint32_t ppb16 = pairs_per_block(8);
    uint32_t slot = 0;
    for (uint32_t b = 0; b <= t8w; slot += h[b], b++) {
        const uint32_t R = t8w - b;                          // bucket b: padded target of 8R
        if (!h[b] || R == 0) continue;
        Wf16Fn fn = wf16_tq_lookup((int)R);
        if (!fn) { set_error("no packed TAIL=QUERY/BOTH instance"); return GASALX_EUNSUPPORTED; }
        P16.slot0 = slot;
        P16.n = slot + h[b];
        HIPCHK(launch_lds(fn, dim3(grid_for(h[b], ppb16)), dim3(kBlock), pl.lds16_bytes, st, P16));
    }
    A.skip = ws.misc.as<uint8_t>();
    A.skip_ppb = 1;
    A.skip_p1 = 0xFFFFFFFFu;
    return launch_int32(pl, wf_lookup(pl.wf_algo, pl.keys, false, pl.G, pl.R), A, st);
}

// SEMI TAIL=NONE outputs (PLAN_CONST): score MINUS_INF, query_batch_end = maxXY_x =
// ref_len, target_batch_end = maxXY_y = read_len (semiglobal_kernel_template.h:49-51,63-64,
// 206-218: Q10's end conventions with no tail block run)
__global__ __launch_bounds__(256) void semi_tail_none_kernel(int32_t *score, int32_t *qend, int32_t *tend,
                                                             const uint32_t *qlen, const uint32_t *tlen, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    score[i] = -32768;
    if (qend) qend[i] = (int32_t)tlen[i];
    if (tend) tend[i] = (int32_t)qlen[i];
}

// WITH_START on the wavefront kernels (start.hpp): the same kernel reading the forward
// sequences backwards over slots sorted by reversed target length, and the map of its ends
// to the start cell.
static int start_reverse(Workspace &ws, int mode, const gasalx_params &p, const uint8_t *q, const uint8_t *t,
                         int packed, const gasalx_batch &b, const BatchShape &shape, const int32_t *score,
                         const int32_t *qend, const int32_t *tend, int32_t *qstart, int32_t *tstart, hipStream_t st) {
    const uint32_t n = b.n_alns;
    const uint32_t q8 = pad8(shape.max_q), t8 = pad8(shape.max_t), t8w = t8 / 8, q8w = q8 / 8;
    // LOCAL: slots that stop early (the drift sweep's lstop) share waves (start.hpp rev_bucket),
    // and the query words come first when the two-key histogram fits LDS
    const bool lstop = mode == REV_LOCAL;
    const bool qkey = lstop && (size_t)(q8w + 1) * (t8w + 1) * 8 <= 64 * 1024;
    const uint32_t nb = qkey ? (q8w + 1) * (t8w + 1) : t8w + 1;
    HIPCHK(ws.rev_meta.reserve((size_t)n * 4 * 6 + (size_t)nb * 8 + 64));
    uint32_t *meta = ws.rev_meta.as<uint32_t>();
    uint32_t *rqlen = meta, *rtlen = meta + n;
    int32_t *rscore = reinterpret_cast<int32_t *>(meta + 2 * (size_t)n);
    int32_t *rqend = rscore + n, *rtend = rscore + 2 * (size_t)n;
    uint32_t *perm = meta + 5 * (size_t)n;
    uint32_t *hist = meta + 6 * (size_t)n, *cursor = hist + nb;
    // counting sort of the pairs by reversed target words (longest first)
    const size_t sh = (size_t)nb * 4;
    if (2 * sh > 64 * 1024) { set_error("WITH_START: target too long for the slot sort"); return GASALX_ERANGE; }
    HIPCHK(hipMemsetAsync(hist, 0, sh, st));
    const int32_t *skey = lstop ? score : nullptr;
    const uint32_t *kql = qkey ? b.q_lens : nullptr;
    rev_hist_kernel<<<sort_grid(n), 256, sh, st>>>(mode, b.t_lens, tend, n, t8w, hist, skey, p.match, kql, qend,
                                                       q8w, nb);
    rev_scan_kernel<<<1, 256, 0, st>>>(hist, cursor, nb);
    rev_scatter_kernel<<<sort_grid(n), 256, 2 * sh, st>>>(mode, b.t_lens, tend, n, t8w, cursor, perm, nullptr,
                                                              skey, p.match, kql, qend, q8w, nb);
    rev_len_kernel<<<grid_for(n, 256), 256, 0, st>>>(mode, q, b.q_offsets, b.q_lens, b.t_lens, qend, tend, packed,
                                                      (uint32_t)(p.n_code & 0xF), n, rqlen, rtlen);
    HIPCHK(hipGetLastError());
    gasalx_params pr = p;
    pr.start_pos = 0;
    BatchShape rs; rs.max_q = q8; rs.max_t = t8; rs.n = n;
    const Plan pl = make_plan(pr, rs, false);
    if (pl.kind != PLAN_WAVEFRONT) { set_error("reverse pass has no wavefront plan"); return GASALX_EUNSUPPORTED; }
    WfArgs A;
    std::memset(&A, 0, sizeof(A));
    A.q = q; A.t = t;
    A.qoff = b.q_offsets; A.toff = b.t_offsets; A.qlen = rqlen; A.tlen = rtlen;
    A.rev = 1;
    A.perm = perm;
    A.perm_xkey = (mode == REV_SEMI || qkey) ? 1 : 0;   // sorted by the register-axis words first
    A.score = rscore; A.qend = rqend; A.tend = rtend;
    A.stop = mode == REV_SEMI ? score : nullptr;     // the forward score per pair
    A.lstop = lstop ? score : nullptr;
    A.n = n;
    A.packed = packed;
    int rc = launch_wavefront(ws, pl, pr, A, TailShape(), st);
    if (rc) return rc;
    start_map_kernel<<<grid_for(n, 256), 256, 0, st>>>(mode, score, b.q_lens, rqlen, b.t_lens, tend, rscore, rqend,
                                                        rtend, qstart, tstart, n);
    HIPCHK(hipGetLastError());
    return GASALX_OK;
}

// GASALX_SORT=0/1 overrides the caller's BatchShape::sort (A/B and probes)
static bool sort_wanted(const BatchShape &s) {
    static const int force = env_int("GASALX_SORT", -1);
    return force < 0 ? s.sort : force != 0;
}

// Uneven lengths, two pairs per lane (banded16 / local16): pair up slots of equal
// tile geometry (QR, TR) by a counting sort on it.  *perm stays NULL (identity)
// for even batches, small ones and geometry counts whose histogram exceeds LDS.
static int geometry_perm(Workspace &ws, const gasalx_batch &b, const BatchShape &shape, uint32_t n, hipStream_t st,
                         const uint32_t **perm_out) {
    *perm_out = nullptr;
    const uint32_t trw = pad8(shape.max_t) / 8, nkeys = (pad8(shape.max_q) / 8) * trw;
    if (!(sort_wanted(shape) && n >= 4096 && 2 * (size_t)(nkeys + 1) * 4 <= 64 * 1024)) return GASALX_OK;
    SortMeta m;   // the keys in its second array
    int rc = sort_reserve(ws, n, nkeys, true, &m);
    if (rc) return rc;
    band16_key_kernel<<<grid_for(n, 256), 256, 0, st>>>(b.q_lens, b.t_lens, n, trw, m.second);
    rc = sort_histogram(m, m.second, n, nkeys, st);
    if (!rc) rc = sort_scatter(m, m.second, n, nkeys, nullptr, st);
    if (rc) return rc;
    *perm_out = m.perm;
    return GASALX_OK;
}

// ----------------------------------------------------------------------------
// One align_body call: its inputs, then what each step leaves for the later ones.
struct Call {
    Workspace &ws;
    const gasalx_params &p;
    const Plan &pl;
    const gasalx_batch &b;
    const gasalx_results &out;
    hipStream_t st;
    const BatchShape &shape;
    uint32_t n;
    bool runs_tb;                 // a traceback walk follows the DP
    const uint8_t *qsrc, *tsrc;   // pack_inputs: the sequences the kernels read, as bytes or packed words
    int packed;
    int32_t *qend, *tend;         // size_traceback: the ends, the caller's or the workspace's;
    uint64_t tb_words;            //   direction words per pair; pair slots of ws.tb
    uint32_t n_tb;
    WfArgs A;                     // run_wavefront: the main launch (the band fallback starts from a copy),
    TailShape tail;               //   its second shape, if any,
    const uint32_t *slot_of;      //   pair -> slot when it ran sorted,
    uint32_t *fb_count;           //   band traceback: the count of pairs handed to the full-matrix fallback
};

// the packed words of the generic kernels and of reverse-complemented batches (Plan::need_pack)
static int pack_inputs(Call &c) {
    Workspace &ws = c.ws;
    const gasalx_batch &b = c.b;
    if (!c.pl.need_pack) return GASALX_OK;
    const uint32_t qw = b.q_bytes / 8, tw = b.t_bytes / 8;
    HIPCHK(ws.packed_q.reserve((size_t)qw * 4 + 16));
    HIPCHK(ws.packed_t.reserve((size_t)tw * 4 + 16));
    if (c.p.is_packed) {
        HIPCHK(hipMemcpyAsync(ws.packed_q.p, b.q_batch, (size_t)qw * 4, hipMemcpyDeviceToDevice, c.st));
        HIPCHK(hipMemcpyAsync(ws.packed_t.p, b.t_batch, (size_t)tw * 4, hipMemcpyDeviceToDevice, c.st));
    } else {
        pack_kernel<<<std::min(grid_for(qw, 256), 4096), 256, 0, c.st>>>(b.q_batch, ws.packed_q.as<uint32_t>(), qw);
        pack_kernel<<<std::min(grid_for(tw, 256), 4096), 256, 0, c.st>>>(b.t_batch, ws.packed_t.as<uint32_t>(), tw);
    }
    if (b.q_ops && b.t_ops) {
        revcomp_kernel<<<grid_for(c.n, 256), 256, 0, c.st>>>(ws.packed_q.as<uint32_t>(), ws.packed_t.as<uint32_t>(),
                                                              b.q_lens, b.t_lens, b.q_offsets, b.t_offsets, b.q_ops,
                                                              b.t_ops, c.n, c.p.n_code);
        // with isPacked the reference's packed buffer aliases the unpacked one, so
        // the reversed words are what the cigar D2H copy sees (ctors.cpp:64-68)
        if (c.p.start_pos == 2 && c.out.cigar && c.p.is_packed)
            HIPCHK(hipMemcpyAsync(c.out.cigar, ws.packed_q.p, (size_t)qw * 4, hipMemcpyDeviceToDevice, c.st));
    }
    c.qsrc = ws.packed_q.as<uint8_t>();
    c.tsrc = ws.packed_t.as<uint8_t>();
    c.packed = 1;
    return GASALX_OK;
}

// the direction words and, where the caller gave none, the end arrays
static int size_traceback(Call &c, bool wf_start) {
    const Plan &pl = c.pl;
    // traceback storage: one word per (8-column strip, padded query row); the
    // packed traceback kernels' skewed uint16 layout needs (t8 + G + 2) / 4 windows
    // of G*R 16-bit entries instead (wavefront16.hpp)
    const uint32_t q8 = pad8(c.shape.max_q), t8 = pad8(c.shape.max_t);
    c.tb_words = (uint64_t)q8 * (t8 / 8);
    if (pl.packed16 && pl.tb)
        c.tb_words = std::max<uint64_t>(c.tb_words, (((uint64_t)pl.G16 * pl.R16 * ((t8 + pl.G16 + 2) / 4) / 2 + 3) & ~3ull));
    // (whole groups of 8 pairs: the packed kernels' interleaved layout, tb_store_window)
    // the band path's full-matrix direction words serve its fallback list only: GASALX_TB_FBCAP slots
    // (131,072 by default), the list then aligned in chunks of that many (the rest reserve every pair)
    const uint32_t fb_cap = std::max(64, env_int("GASALX_TB_FBCAP", 131072));
    c.n_tb = (pl.kind == PLAN_WAVEFRONT && pl.packed16 && pl.tb_band) ? std::min(c.n, fb_cap) : c.n;
    if (c.runs_tb) HIPCHK(c.ws.tb.reserve((size_t)((c.n_tb + 7) & ~7u) * c.tb_words * 4 + 64));
    if ((c.runs_tb || wf_start) && (c.p.algo == 3 || c.p.algo == 2) && (!c.qend || !c.tend)) {
        HIPCHK(c.ws.ends_q.reserve((size_t)c.n * 4));
        HIPCHK(c.ws.ends_t.reserve((size_t)c.n * 4));
        if (!c.qend) c.qend = c.ws.ends_q.as<int32_t>();
        if (!c.tend) c.tend = c.ws.ends_t.as<int32_t>();
    }
    return GASALX_OK;
}

// uneven lengths: a wave's step count is set by its longest step-axis
// sequence (target; query for the transposed SEMI kernel), so run the
// slots in length order (counting sort, longest first)
// (semi_tq sorts by target class itself; a launch whose waves hold fewer than 8 pairs --
// the small-batch shapes, G >= 32 -- gains nothing from the order and would pay the three
// sort launches: a 5,000-pair batch of the reference's sample data, profiles/r06/boundary)
static int forward_length_sort(Call &c) {
    const Plan &pl = c.pl;
    const int gsort = pl.packed16 ? pl.G16 : pl.G;
    if (!(sort_wanted(c.shape) && c.n >= 4096 && !pl.semi_tq && pairs_per_wave(std::max(gsort, 1)) >= 8)) return GASALX_OK;
    const uint32_t s8w = pad8(pl.wf_algo == WF_SEMI ? c.shape.max_q : c.shape.max_t) / 8;
    if (2 * (size_t)(s8w + 1) * 4 > 64 * 1024) return GASALX_OK;
    return counting_sort(c.ws, pl.wf_algo == WF_SEMI ? c.b.q_lens : c.b.t_lens, c.n, s8w, c.st, true, &c.A.perm,
                         &c.slot_of);
}

// band recomputation buffers per wave of the packed launch (wavefront16.hpp); a mixed-
// shape launch (c.tail) keeps its second region's after the first's
static int size_band_buffers(Call &c) {
    Workspace &ws = c.ws;
    const Plan &pl = c.pl;
    const TailShape &tail = c.tail;
    WfArgs &A = c.A;
    const uint32_t n = c.n, grid1 = grid_for(n, pairs_per_block(pl.G16));
    const uint64_t waves = (uint64_t)(tail.fn ? tail.b0 : grid1) * kWavesPerBlock;
    const uint64_t waves2 = tail.fn ? (uint64_t)grid_for(n - tail.p0, tail.ppb) * kWavesPerBlock : 0;
    const uint32_t wd2 = tail.fn ? band_window(tail.R2, pl.band_w) : 4u;
    const uint64_t cpw1 = waves * 2 * pl.R16 * 64, cpw2 = waves2 * 2 * tail.R2 * 64;   // words
    const uint64_t st1 = waves * 64 * band_stream_words(pl.band_wd), st2 = waves2 * 64 * band_stream_words(wd2);
    const uint64_t fl1 = waves * 64 * (pl.band_wd / 4) * (pl.R16 / 4), fl2 = waves2 * 64 * (wd2 / 4) * (tail.R2 / 4);
    HIPCHK(ws.band_cp.reserve((cpw1 + cpw2) * 4 + 64));
    HIPCHK(ws.band_stm.reserve((st1 + st2) * 8 + 64));
    HIPCHK(ws.band_fl.reserve((fl1 + fl2) * 16 + 64));
    HIPCHK(ws.band_fb.reserve((size_t)n * 4 + grid1 + 256));
    A.cp = ws.band_cp.as<uint32_t>();
    A.stm = ws.band_stm.as<uint2>();
    A.bflags = ws.band_fl.as<uint4>();
    A.band_w = pl.band_w;
    A.band_wd = pl.band_wd;
    A.cp2 = A.cp + cpw1;
    A.stm2 = A.stm + st1;
    A.bflags2 = A.bflags + fl1;
    A.band_wd2 = wd2;
    c.fb_count = ws.band_fb.as<uint32_t>();
    return GASALX_OK;
}

// PLAN_WAVEFRONT: the main launch, and the reverse pass of WITH_START
static int run_wavefront(Call &c, bool wf_start) {
    const gasalx_params &p = c.p;
    const Plan &pl = c.pl;
    WfArgs &A = c.A;
    A.q = c.qsrc; A.t = c.tsrc;
    A.qoff = c.b.q_offsets; A.toff = c.b.t_offsets; A.qlen = c.b.q_lens; A.tlen = c.b.t_lens;
    A.score = c.out.aln_score;
    A.qend = (p.algo == 1) ? nullptr : c.qend;
    A.tend = (p.algo == 1) ? nullptr : c.tend;
    A.tb = c.ws.tb.as<uint32_t>();
    A.tb_pair_words = c.tb_words;
    A.n = c.n;
    A.packed = c.packed;
    int rc = forward_length_sort(c);
    if (rc) return rc;
    // unsorted waves hold consecutive pairs: interleave their direction chunks
    A.tb_q8 = (pl.packed16 && pl.tb && !pl.tb_band && !A.perm) ? 1u : 0u;
    // the one evaluation of the tail shape: this launch, its band buffers and the walk share it
    c.tail = tail_shape(c.ws, pl, p, A, c.n);
    if (pl.tb_band && c.runs_tb && (rc = size_band_buffers(c))) return rc;
    rc = pl.semi_tq ? launch_semi_tq(c.ws, pl, p, A, c.st, c.shape.one_t8) : launch_wavefront(c.ws, pl, p, A, c.tail, c.st);
    if (rc || !wf_start) return rc;
    return start_reverse(c.ws, p.algo == 3 ? REV_LOCAL : REV_SEMI, p, c.qsrc, c.tsrc, c.packed, c.b, c.shape,
                         c.out.aln_score, c.qend, c.tend, c.out.q_start, c.out.t_start, c.st);
}

// KSW: 8-bit (h, e) entries, then 16-bit, then int2, each for the pairs whose score
// bound does not fit the level before
static int run_ksw(Call &c, const GenArgs &A) {
    Workspace &ws = c.ws;
    const gasalx_params &p = c.p;
    const gasalx_batch &b = c.b;
    const uint32_t n = c.n, max_q = c.shape.max_q;
    hipStream_t st = c.st;
    HIPCHK(ws.rows_h.reserve((size_t)(max_q + 8) * n * 8));
    HIPCHK(ws.misc.reserve(n));
    HIPCHK(hipMemsetAsync(ws.misc.p, 0, n, st));
    uint8_t *todo = ws.misc.as<uint8_t>();
    // two pairs per lane in 16-bit halves first (ksw16.hpp): the pairs it takes
    // get todo = 0xFF, the rest run the levels below (GASALX_KSW16=0: levels only)
    int32_t kofs;
    if (ksw16_ok(p, max_q, &kofs)) {
        Ksw16Args K;
        std::memset(&K, 0, sizeof(K));
        K.qw = A.qw; K.tw = A.tw;
        K.qoff = b.q_offsets; K.toff = b.t_offsets; K.qlen = b.q_lens; K.tlen = b.t_lens;
        K.seed = b.seed_scores;
        K.score = c.out.aln_score; K.qend = c.qend; K.tend = c.tend;
        K.todo = todo;
        K.n = n; K.n_lanes = (n + 1) / 2; K.cols = (max_q + 3) & ~1u;
        K.stride = grid_for(K.n_lanes, 256) * 256;
        fill_scoring(K, p);
        K.kofs = kofs;
        // the entry row in registers when the padded query fits an instance
        // (selector words in LDS: QC / 2 words per lane), else the global array
        int qc = 0;
        for (int q : {64, 96, 160})
            if (K.cols <= (uint32_t)q) { qc = q; break; }
        if (qc) {
            void (*fn)(Ksw16Args) = qc == 64 ? &ksw16_kernel<64> : qc == 96 ? &ksw16_kernel<96> : &ksw16_kernel<160>;
            HIPCHK(launch_lds(fn, dim3(grid_for(K.n_lanes, 256)), dim3(256), (size_t)4 * (qc / 2) * 64 * 4, st, K));
        } else {
            const size_t ent_words = (size_t)K.cols * K.stride, sel_words = (size_t)(K.cols / 2) * K.stride;
            HIPCHK(ws.rows_e.reserve((ent_words + sel_words) * 4 + 64));
            K.ent = ws.rows_e.as<uint32_t>(); K.sel = K.ent + ent_words;
            ksw16_kernel<0><<<grid_for(K.n_lanes, 256), 256, 0, st>>>(K);
            HIPCHK(hipGetLastError());
        }
    }
    // level 0 with the entries in LDS when two blocks of >= 64 threads fit
    // a CU, for batches of up to 4 waves per SIMD: LDS then holds 2 waves
    // per SIMD, and larger batches run faster on the global array with its
    // higher occupancy (200 K config-2 pairs: 806 -> 890 GCUPS; 1 M: 1,320
    // global, 1,146 LDS).  GASALX_KSW_LDS=0/1 forces either (A/B)
    const bool lds_on = env_flag("GASALX_KSW_LDS", n <= 4u * 1024u * 64u);
    uint32_t tpb = 0;
    size_t lds = 0;
    if (lds_on)
        for (uint32_t t : {256u, 128u, 64u}) {
            lds = (size_t)t * (max_q + 2) * 2;
            if (2 * lds <= 160 * 1024) { tpb = t; break; }
        }
    if (tpb)
        HIPCHK(launch_lds(&gen_ksw_kernel<0, true>, dim3(grid_for(n, tpb)), dim3(tpb), lds, st, A, ws.rows_h.p, todo));
    else
        gen_ksw_kernel<0><<<grid_for(n, 256), 256, 0, st>>>(A, ws.rows_h.p, todo);
    gen_ksw_kernel<1><<<grid_for(n, 256), 256, 0, st>>>(A, ws.rows_h.p, todo);
    gen_ksw_kernel<2><<<grid_for(n, 256), 256, 0, st>>>(A, ws.rows_h.p, todo);
    return GASALX_OK;
}

// LOCAL second best, two pairs per lane (local16.hpp): *todo marks the pairs left to gen_local_kernel
static int run_local16_prepass(Call &c, const GenArgs &A, const uint8_t **todo) {
    Workspace &ws = c.ws;
    const gasalx_params &p = c.p;
    const uint32_t n = c.n, q8 = pad8(c.shape.max_q);
    Local16Args D;
    std::memset(&D, 0, sizeof(D));
    D.qw = A.qw; D.tw = A.tw;
    D.qoff = c.b.q_offsets; D.toff = c.b.t_offsets; D.qlen = c.b.q_lens; D.tlen = c.b.t_lens;
    D.score = c.out.aln_score; D.qend = c.qend; D.tend = c.tend;
    D.score2 = c.out.aln_score2; D.qend2 = c.out.q_end2; D.tend2 = c.out.t_end2;
    D.n = n; D.n_lanes = (n + 1) / 2;
    D.a = p.match; D.b = p.mismatch; D.oe = p.gap_open + p.gap_extend; D.e = p.gap_extend;
    D.nval = A.nval; D.sn = local16_sn(p); D.k = local16_k(p); D.base = local16_base(p);
    HIPCHK(ws.misc.reserve(n));
    HIPCHK(hipMemsetAsync(ws.misc.p, 0, n, c.st));
    D.todo = ws.misc.as<uint8_t>();
    D.rows_cap = q8;
    HIPCHK(ws.aux.reserve((size_t)q8 * ((D.n_lanes + 63) / 64) * 64 * 8 + 64));
    D.rows = ws.aux.as<uint2>();
    const int rc = geometry_perm(ws, c.b, c.shape, n, c.st, &D.perm);
    if (rc) return rc;
    // 3 waves per SIMD (162 VGPRs): 2 waves 2 % and 4 waves (spills) 5-15 % slower
    local2nd16_kernel<3><<<grid_for(D.n_lanes, 256), 256, 0, c.st>>>(D);
    HIPCHK(hipGetLastError());
    *todo = D.todo;
    return GASALX_OK;
}

// BANDED, two pairs per lane (banded16.hpp): *todo marks the pairs left to gen_banded_kernel
static int run_band16_prepass(Call &c, const GenArgs &A, const uint8_t **todo) {
    Workspace &ws = c.ws;
    const gasalx_params &p = c.p;
    const uint32_t n = c.n, q8 = pad8(c.shape.max_q);
    BandArgs D;
    std::memset(&D, 0, sizeof(D));
    D.qw = A.qw; D.tw = A.tw;
    D.qoff = c.b.q_offsets; D.toff = c.b.t_offsets; D.qlen = c.b.q_lens; D.tlen = c.b.t_lens;
    D.score = c.out.aln_score; D.qend = c.qend; D.tend = c.tend;
    D.n = n; D.n_lanes = (n + 1) / 2;
    D.a = p.match; D.b = p.mismatch; D.oe = p.gap_open + p.gap_extend; D.e = p.gap_extend;
    D.kbw = A.kbw; D.nval = A.nval; D.base = band16_base(p);
    HIPCHK(ws.misc.reserve(n));
    HIPCHK(hipMemsetAsync(ws.misc.p, 0, n, c.st));
    D.todo = ws.misc.as<uint8_t>();
    HIPCHK(ws.aux.reserve((size_t)q8 * D.n_lanes * 8 + 64));
    D.rows = ws.aux.as<uint2>();
    const int rc = geometry_perm(ws, c.b, c.shape, n, c.st, &D.perm);
    if (rc) return rc;
    band16_kernel<<<grid_for(D.n_lanes, 256), 256, 0, c.st>>>(D);
    HIPCHK(hipGetLastError());
    *todo = D.todo;
    return GASALX_OK;
}

// PLAN_GENERIC: a thread per pair over packed words, after the two-pairs-per-lane kernel of the
// plans that have one
static int run_generic(Call &c) {
    Workspace &ws = c.ws;
    const gasalx_params &p = c.p;
    const gasalx_batch &b = c.b;
    const uint32_t n = c.n;
    hipStream_t st = c.st;
    GenArgs A;
    std::memset(&A, 0, sizeof(A));
    A.qw = ws.packed_q.as<uint32_t>(); A.tw = ws.packed_t.as<uint32_t>();
    A.qoff = b.q_offsets; A.toff = b.t_offsets; A.qlen = b.q_lens; A.tlen = b.t_lens;
    A.seed = b.seed_scores;
    A.score = c.out.aln_score; A.qend = c.qend; A.tend = c.tend; A.qstart = c.out.q_start; A.tstart = c.out.t_start;
    A.score2 = c.out.aln_score2; A.qend2 = c.out.q_end2; A.tend2 = c.out.t_end2;
    A.tb = ws.tb.as<uint32_t>(); A.tb_pair_words = c.tb_words;
    const uint32_t q8 = pad8(c.shape.max_q), t8 = pad8(c.shape.max_t);
    uint32_t maxq = p.max_query_len > 0 ? (uint32_t)p.max_query_len : std::max(q8, t8);
    if (maxq < q8) { set_error("max_query_len smaller than a padded query"); return GASALX_ERANGE; }
    if (p.algo == 2 && p.start_pos == 1 && maxq < t8) {
        set_error("semi-global WITH_START needs max_query_len >= padded target length");
        return GASALX_ERANGE;
    }
    A.rows_cap = std::max(maxq, q8) + 8;
    A.maxq = (int32_t)maxq;
    A.rev_words = maxq / 8 + 1;
    A.n = n;
    fill_scoring(A, p);
    A.start_pos = p.start_pos; A.second = p.second_best; A.head = p.head; A.tail = p.tail;
    A.kbw = p.k_band >> 3;
    int rc = GASALX_OK;
    if (p.algo == 6) {
        if ((rc = run_ksw(c, A))) return rc;
    } else {
        const size_t rows_elems = (size_t)A.rows_cap * n;
        HIPCHK(ws.rows_h.reserve(rows_elems * 2));
        HIPCHK(ws.rows_e.reserve(rows_elems * 2));
        A.rowH = ws.rows_h.as<int16_t>(); A.rowE = ws.rows_e.as<int16_t>();
        if (p.algo == 3) {
            if (c.pl.local16 && (rc = run_local16_prepass(c, A, &A.todo))) return rc;
            gen_local_kernel<<<grid_for(n, 256), 256, 0, st>>>(A);
        } else if (p.algo == 2) {
            if (p.start_pos == 1) {
                HIPCHK(ws.rev.reserve((size_t)2 * A.rev_words * n * 4));
                A.rev = ws.rev.as<uint32_t>();
            }
            gen_semi_kernel<<<grid_for(n, 256), 256, 0, st>>>(A);
        } else if (p.algo == 5) {
            if (c.pl.band16 && (rc = run_band16_prepass(c, A, &A.todo))) return rc;
            gen_banded_kernel<<<grid_for(n, 256), 256, 0, st>>>(A);
        } else {
            gen_global_kernel<<<grid_for(n, 256), 256, 0, st>>>(A);
        }
    }
    HIPCHK(hipGetLastError());
    return GASALX_OK;
}

// The walk's arguments: every field's default in one place, then what the main launch decided.
// walk_qseq: align_device's copy of the query codes, or NULL.
static TbArgs make_tb_args(const Call &c, uint64_t cigar_cap, const uint8_t *walk_qseq) {
    const gasalx_params &p = c.p;
    const Plan &pl = c.pl;
    TbArgs T;
    std::memset(&T, 0, sizeof(T));
    T.tb = c.ws.tb.as<uint32_t>(); T.tb_pair_words = c.tb_words;
    T.qlen = c.b.q_lens; T.tlen = c.b.t_lens; T.qoff = c.b.q_offsets;
    T.score = c.out.aln_score; T.qend = c.qend; T.tend = c.tend;
    T.qstart = c.out.q_start; T.tstart = c.out.t_start;
    T.cigar = c.out.cigar; T.n_ops = c.out.n_cigar_ops; T.n = c.n;
    T.cigar_cap = cigar_cap ? cigar_cap : c.b.q_bytes;
    fill_scoring(T, p);
    T.is_local = pl.semi_tb ? kTbSemi : p.algo == 3;
    T.semi_head = pl.semi_tb ? p.head : 2;
    T.slot_of = c.slot_of;
    T.sc_nn = p.has_n_penalty ? -p.n_penalty : p.match;   // GLOBAL: N == N is a match unless N_PENALTY
    T.qseq = walk_qseq ? walk_qseq : c.qsrc; T.tseq = c.tsrc; T.toff = c.b.t_offsets; T.seq_packed = c.packed;
    // no packed launch, one shape, no band, no fallback list (pointers and offsets: zero)
    T.pk_ppb = 1; T.pk_R = 1; T.pk_G = 1;
    T.pk_p1 = 0xFFFFFFFFu; T.pk_ppb2 = 1;
    T.band_wd = 4; T.pk_ppw = 1;
    T.band_wd2 = 4; T.pk_R2 = 4; T.pk_G2 = 1; T.pk_ppw2 = 1;
    if (pl.kind == PLAN_WAVEFRONT && pl.packed16) {
        T.pk_flags = c.ws.misc.as<uint8_t>();
        T.pk_ppb = pairs_per_block(pl.G16);
        T.pk_R = pl.R16;
        T.pk_G = pl.G16;
        T.pk_rmagic = rmagic(pl.R16);
        T.pk_fix = c.ws.aux.as<int32_t>();
        T.pk_q8 = c.A.tb_q8;
        if (c.tail.fn) { T.pk_p1 = c.tail.p0; T.pk_b1 = c.tail.b0; T.pk_ppb2 = c.tail.ppb; }   // the launch's flag ranges
    }
    if (c.fb_count) {
        T.band = c.ws.band_fl.as<uint4>();
        T.band_w = pl.band_w; T.band_wd = pl.band_wd;
        T.pk_ppw = pairs_per_wave(pl.G16);
        if (c.tail.fn) {   // the second region of a mixed-shape launch
            T.band2 = c.A.bflags2;
            T.band_wd2 = c.A.band_wd2;
            T.pk_R2 = c.tail.R2; T.pk_G2 = c.tail.G2; T.pk_ppw2 = pairs_per_wave(c.tail.G2);
            T.pk_rmagic2 = rmagic(c.tail.R2);
        }
        T.fb_count = c.fb_count;
        T.fb_list = c.fb_count + 64;
    }
    return T;
}

// Band traceback, after the walk: pairs whose path left the band (or whose block the packed launch
// declined): the full-matrix packed traceback kernel over the list (slots = list positions; per-pair
// flag layout at slot positions of the capped buffer), its int32 kernel for any block it
// declines, and the walk again -- in chunks of n_tb list positions, each launch reading
// the device-side count less its chunk's offset (empty chunks exit at once)
static int run_band_fallback(Call &c, const TbArgs &T, const uint8_t *walk_qseq) {
    Plan fp = c.pl;
    fp.tb_band = false;
    for (uint32_t k0 = 0; k0 < c.n; k0 += c.n_tb) {
        const uint32_t cn = std::min(c.n_tb, c.n - k0);
        WfArgs F = c.A;
        // the band walk has written CIGAR prefixes over the query batch when that is the
        // CIGAR buffer (get_tb.h:94): the DP reads align_device's copy of the codes then
        if (walk_qseq) F.q = walk_qseq;
        F.perm = T.fb_list + k0;
        F.n = cn;
        F.n_dev = c.fb_count;
        F.n_dev_off = k0;
        F.tb_slot = 1;
        F.tb_q8 = 0;
        F.cp = nullptr; F.stm = nullptr; F.bflags = nullptr;
        int rc = launch_wavefront(c.ws, fp, c.p, F, TailShape(), c.st);
        if (rc) return rc;
        TbArgs T2 = T;
        T2.band = nullptr;
        T2.list = T.fb_list + k0;
        T2.n = cn;
        T2.n_dev = c.fb_count;
        T2.n_dev_off = k0;
        T2.tb_slot = 1;
        T2.slot_of = nullptr;
        T2.pk_q8 = 0;
        T2.pk_p1 = 0xFFFFFFFFu;   // the fallback launch is one shape (its n_dev excludes the tail)
        T2.fb_list = T2.fb_count = nullptr;
        tb_kernel<<<grid_for(cn, 256), 256, 0, c.st>>>(T2);
        HIPCHK(hipGetLastError());
    }
    return GASALX_OK;
}

// the traceback walk over every pair, then the band path's fallback
static int run_walk(Call &c, uint64_t cigar_cap, const uint8_t *walk_qseq) {
    const TbArgs T = make_tb_args(c, cigar_cap, walk_qseq);
    if (c.fb_count) HIPCHK(hipMemsetAsync(c.fb_count, 0, 4, c.st));
    tb_kernel<<<grid_for(c.n, 256), 256, 0, c.st>>>(T);
    HIPCHK(hipGetLastError());
    return c.fb_count ? run_band_fallback(c, T, walk_qseq) : GASALX_OK;
}

// Everything after align_device's prologue, over the pairs of b (a whole batch or one
// chunk of it): pack, size, launch, walk.  walk_qseq: the query codes the traceback walk
// reads when the CIGAR buffer overlays the query batch (copied once by the prologue), else NULL.
static int align_body(Workspace &ws, const gasalx_params &p, const Plan &pl, const gasalx_batch &b,
                      const gasalx_results &out, hipStream_t st, const BatchShape &shape, uint64_t cigar_cap,
                      const uint8_t *walk_qseq) {
    const uint32_t n = b.n_alns;
    if (pl.kind == PLAN_CONST) {
        semi_tail_none_kernel<<<grid_for(n, 256), 256, 0, st>>>(out.aln_score, out.q_end, out.t_end, b.q_lens,
                                                                      b.t_lens, n);
        HIPCHK(hipGetLastError());
        return GASALX_OK;
    }
    const bool runs_tb = p.start_pos == 2 && (p.algo == 1 || p.algo == 3) && pl.kind != PLAN_NONE;
    const bool wf_start = pl.kind == PLAN_WAVEFRONT && (p.algo == 3 || p.algo == 2) && p.start_pos == 1 &&
                          (out.q_start || out.t_start);
    Call c{ws, p, pl, b, out, st, shape, n, runs_tb, b.q_batch, b.t_batch, p.is_packed ? 1 : 0, out.q_end, out.t_end};
    int rc = pack_inputs(c);
    if (!rc) rc = size_traceback(c, wf_start);
    if (!rc) rc = pl.kind == PLAN_WAVEFRONT ? run_wavefront(c, wf_start) : run_generic(c);
    if (!rc && runs_tb && out.cigar && out.n_cigar_ops) rc = run_walk(c, cigar_cap, walk_qseq);
    return rc;
}

int align_device(Workspace &ws, const gasalx_params &p, const gasalx_batch &b, const gasalx_results &out,
                 hipStream_t st, const BatchShape &shape, uint64_t cigar_cap) {
    if (b.n_alns == 0 || b.q_bytes == 0 || b.t_bytes == 0) { set_error("empty batch"); return GASALX_EINVAL; }
    if ((b.q_bytes & 7) || (b.t_bytes & 7)) { set_error("batch bytes not a multiple of 8"); return GASALX_EINVAL; }
    if (!out.aln_score) { set_error("aln_score output required"); return GASALX_EINVAL; }
    if (p.algo == 6 && !b.seed_scores) { set_error("KSW needs seed_scores"); return GASALX_EINVAL; }
    if (shape.max_q == 0 || shape.max_t == 0) { set_error("zero-length sequence"); return GASALX_ERANGE; }
    const bool has_ops = b.q_ops && b.t_ops;
    // gasalx_packed_pairs reads the packed launch flags of this call only: a call that launches
    // no packed kernel (or reuses misc for other flags, the KSW / banded / local16 todo arrays)
    // must not leave the last call's count behind
    ws.pk_flags = 0;
    BatchShape sized = shape;
    sized.n = b.n_alns;
    Plan pl = make_plan(p, sized, has_ops);
    const uint32_t n = b.n_alns;
    const bool tb = p.start_pos == 2;

    // TB: the device cigar buffer starts as the unpacked query batch, as in the
    // reference where get_tb writes into unpacked_query_batch (get_tb.h:94,
    // gasal_align.cu:281); n_cigar_ops = query_batch_lens unless get_tb runs.
    if (tb && out.cigar && (const void *)out.cigar != (const void *)b.q_batch)
        HIPCHK(copy_d2d(out.cigar, b.q_batch, b.q_bytes, st));
    const bool runs_tb = tb && (p.algo == 1 || p.algo == 3) && pl.kind != PLAN_NONE;
    if (tb && out.n_cigar_ops && !runs_tb && (const void *)out.n_cigar_ops != (const void *)b.q_lens)
        HIPCHK(hipMemcpyAsync(out.n_cigar_ops, b.q_lens, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    if (pl.kind == PLAN_NONE) return GASALX_OK;   // UNKNOWN / MICROLOCAL: nothing launched

    // the walk writes CIGARs over the unpacked query batch when that is the cigar
    // buffer (get_tb.h:94) but the packed kernels' walk reads query codes from it:
    // give it a copy, taken before any walk runs
    const uint8_t *walk_qseq = nullptr;
    const bool cigar_on_query = out.cigar && (const uint8_t *)out.cigar < b.q_batch + b.q_bytes &&
                                b.q_batch < (const uint8_t *)out.cigar + (cigar_cap ? cigar_cap : b.q_bytes);
    if (runs_tb && out.cigar && out.n_cigar_ops && pl.kind == PLAN_WAVEFRONT && pl.packed16 && !pl.need_pack) {
        if (cigar_on_query) {
            HIPCHK(ws.packed_q.reserve(b.q_bytes));
            HIPCHK(hipMemcpyAsync(ws.packed_q.p, b.q_batch, b.q_bytes, hipMemcpyDeviceToDevice, st));
            walk_qseq = ws.packed_q.as<uint8_t>();
        }
    }

    // (one launch chain: the walk is latency-bound -- ~600 dependent steps whatever the batch size --
    // so splitting a call into halves whose walks overlap the next half's DP leaves the last walk
    // exposed and gained nothing; round 6 measured it, profiles/r06/)
    return align_body(ws, p, pl, b, out, st, sized, cigar_cap, walk_qseq);
}

// gasalx_semi_cigar_*: SEMI-GLOBAL with HEAD = TAIL = TARGET and the alignment itself.  Three steps on
// one stream: the score launch of align_device with WITHOUT_START (score, q_end, t_end: the same
// kernels, so the same numbers), the direction-flag launch over the same sequences (WF16_SEMI_TB, the
// int32 kernel for declined blocks), and the walk from (ql - 1, t_end) until the query is exhausted.
// gasalx_semi_cigar_head_* (heads): the same three steps under any HEAD -- the score launch is
// align_device's for that HEAD, the flag launch takes the boundary from the kernel argument
// (WF16_SEMI_TBH; HEAD = TARGET the instances above), the walk ends by that HEAD's rules.
int semi_cigar_device(Workspace &ws, const gasalx_params &p, const gasalx_batch &b, const gasalx_results &out,
                      hipStream_t st, const BatchShape &shape, bool sort_t, bool heads) {
    if (b.n_alns == 0 || b.q_bytes == 0 || b.t_bytes == 0) { set_error("empty batch"); return GASALX_EINVAL; }
    if ((b.q_bytes & 7) || (b.t_bytes & 7)) { set_error("batch bytes not a multiple of 8"); return GASALX_EINVAL; }
    if (shape.max_q == 0 || shape.max_t == 0) { set_error("zero-length sequence"); return GASALX_ERANGE; }
    const bool has_ops = b.q_ops && b.t_ops;
    const uint32_t n = b.n_alns;
    ws.pk_flags = 0;
    BatchShape sized = shape;
    sized.n = n;
    gasalx_params ps = p;
    ps.algo = 2; ps.start_pos = 0; ps.second_best = 0; ps.tail = 2;
    if (!heads) ps.head = 2;   // (gasalx_semi_cigar_head_*: the caller's HEAD through all three steps)
    int rc = GASALX_OK;
    std::string why;
    BatchShape tshape = sized;
    tshape.sort = sort_t;
    const Plan tpl = make_semi_cigar_plan(ps, tshape, has_ops, &rc, &why, heads);
    if (rc) { set_error(why); return rc; }
    const Plan spl = make_plan(ps, sized, has_ops);

    // the score launch: the walk needs t_end whether the caller asked for it or not
    gasalx_results so = {};
    so.aln_score = out.aln_score; so.q_end = out.q_end; so.t_end = out.t_end;
    if (!so.t_end) {
        HIPCHK(ws.ends_t.reserve((size_t)n * 4));
        so.t_end = ws.ends_t.as<int32_t>();
    }
    Call sc{ws, ps, spl, b, so, st, sized, n, false, b.q_batch, b.t_batch, ps.is_packed ? 1 : 0, so.q_end, so.t_end};
    rc = pack_inputs(sc);
    if (!rc) rc = size_traceback(sc, false);
    if (!rc) rc = spl.kind == PLAN_WAVEFRONT ? run_wavefront(sc, false) : run_generic(sc);
    if (rc) return rc;

    // the flags launch over the sequences the score launch read (the packed words after ops), the walk
    Call tc{ws, ps, tpl, b, out, st, tshape, n, true, sc.qsrc, sc.tsrc, sc.packed, so.q_end, so.t_end};
    rc = size_traceback(tc, false);
    if (!rc) rc = run_wavefront(tc, false);
    if (!rc) rc = run_walk(tc, b.q_bytes, nullptr);
    return rc;
}

// ----------------------------------------------------------------------------
constexpr int kHmmRows = 8;   // read rows per lane
using HmmFn = void (*)(HmmArgs);
template <bool QUALS, bool ABS>
static HmmFn hmm_lookup(int G) {
    switch (G) {
        case 4: return &pairhmm_kernel<4, kHmmRows, QUALS, ABS>;
        case 8: return &pairhmm_kernel<8, kHmmRows, QUALS, ABS>;
        case 16: return &pairhmm_kernel<16, kHmmRows, QUALS, ABS>;
        case 32: return &pairhmm_kernel<32, kHmmRows, QUALS, ABS>;
        case 64: return &pairhmm_kernel<64, kHmmRows, QUALS, ABS>;
        default: return nullptr;
    }
}

// lanes per pair for a read of max_r rows: `rows` read rows per lane, G in {4, ..., 64}
static int hmm_group(uint32_t max_r, int rows) {
    for (int g : {4, 8, 16, 32, 64})
        if ((uint32_t)g * rows >= max_r) return g;
    return 0;
}
int pairhmm_group(uint32_t max_r) { return hmm_group(max_r, kHmmRows); }

// One launch over slots [slot0, slot1) of A (A.perm maps slots to pairs, or NULL).
static int pairhmm_launch(HmmArgs A, bool quals, uint32_t max_r, uint32_t slot0, uint32_t slot1, uint32_t max_h,
                          hipStream_t st) {
    const int rows = kHmmRows;
    const int G = hmm_group(max_r, rows);
    if (slot1 <= slot0) return GASALX_OK;
    if (!G) { set_error("PairHMM read longer than 512"); return GASALX_ERANGE; }
    A.slot0 = slot0;
    A.n = slot1;
    A.lds_stride = (std::max<uint32_t>(max_h, 4) + 3) & ~3u;
    // reads shorter than the group's rows: the top lane's first row is virtual and
    // absorbs the boundary (pairhmm.hpp ABS)
    const bool absorb = (uint32_t)G * rows > max_r;
    // haplotype slots, then the per-lane prior tables (pairhmm.hpp): 4 waves x 4 codes x
    // rows x 64 lanes x 4 bytes
    const size_t lds = (((size_t)4 * (64 / G) * A.lds_stride + 15) & ~(size_t)15) + (size_t)4 * 4 * rows * 64 * 4;
    if (lds > 160 * 1024) { set_error("PairHMM haplotype too long"); return GASALX_ERANGE; }
    HmmFn fn = quals ? (absorb ? hmm_lookup<true, true>(G) : hmm_lookup<true, false>(G))
                     : (absorb ? hmm_lookup<false, true>(G) : hmm_lookup<false, false>(G));
    HIPCHK(launch_lds(fn, dim3(grid_for(slot1 - slot0, 4 * (64 / G))), dim3(256), lds, st, A));
    return GASALX_OK;
}

int pairhmm_device(Workspace &ws, const gasalx_hmm_batch &b, float *result, hipStream_t st, uint32_t max_r,
                   uint32_t max_h) {
    (void)ws;
    if (b.n_pairs == 0) return GASALX_OK;
    HmmArgs A;
    std::memset(&A, 0, sizeof(A));
    A.reads = b.reads; A.roff = b.read_offsets; A.rlen = b.read_lens;
    A.qm = b.qm; A.delta = b.delta; A.xiksi = b.xiksi; A.alpha = b.alpha;
    A.haps = b.haps; A.hoff = b.hap_offsets; A.hlen = b.hap_lens;
    A.result = result;
    return pairhmm_launch(A, false, max_r, 0, b.n_pairs, max_h, st);
}

int pairhmm_quals_device(Workspace &ws, const gasalx_hmm_qual_batch &b, float *result, hipStream_t st,
                         const float *ph2pr_dev, const uint32_t *perm, const HmmClass *classes, int n_classes,
                         uint32_t max_r, uint32_t max_h) {
    (void)ws;
    if (b.n_pairs == 0) return GASALX_OK;
    HmmArgs A;
    std::memset(&A, 0, sizeof(A));
    A.reads = b.reads; A.roff = b.read_offsets; A.rlen = b.read_lens;
    A.bq = b.base_quals; A.iq = b.ins_quals; A.dq = b.del_quals; A.ph2pr = ph2pr_dev;
    A.haps = b.haps; A.hoff = b.hap_offsets; A.hlen = b.hap_lens;
    A.result = result;
    A.perm = perm;
    if (!classes) return pairhmm_launch(A, true, max_r, 0, b.n_pairs, max_h, st);
    for (int c = 0; c < n_classes; c++) {
        int rc = pairhmm_launch(A, true, classes[c].max_r, classes[c].slot0, classes[c].slot1,
                                classes[c].max_h, st);
        if (rc) return rc;
    }
    return GASALX_OK;
}

}  // namespace gx
