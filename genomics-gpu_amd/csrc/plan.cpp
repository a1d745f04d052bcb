// plan.cpp — the planner: which kernel family, launch shape and value window a batch gets.  Host only.
// A wrong plan corrupts a neighbouring pair's half-word silently, so each rule stands here once.
#include "plan.hpp"

namespace gx {

// the planner's shape lists, smallest first (shapes.hpp)
struct Shape { int G, R; };
#define GX_SHAPE(g, r) {g, r},
static const Shape kShapes[] = {GX_SHAPES_R4(GX_SHAPE)};
static const Shape kShapes16[] = {GX_SHAPES_PK(GX_SHAPE)};
#undef GX_SHAPE

// every score a magnitude: match, mismatch, gap_open, gap_extend and the optional N penalty >= 0
static bool scores_nonneg(const gasalx_params &p) {
    return p.match >= 0 && p.mismatch >= 0 && p.gap_open >= 0 && p.gap_extend >= 0 &&
           !(p.has_n_penalty && p.n_penalty < 0);
}
static int64_t npen_of(const gasalx_params &p) { return p.has_n_penalty ? p.n_penalty : 0; }
// table offsets K (wavefront16.hpp pk16_params; a table byte is s + K): LOCAL's, GLOBAL's round-2 offset and
// its K >= 2e (drift e, step_global; the semi-CIGAR flags kernel shares it); LOCAL's stored value of 0
static int64_t local_k(const gasalx_params &p) { return std::max<int64_t>(p.mismatch, npen_of(p)); }
static int64_t global_k0(const gasalx_params &p) { return 2 * ((local_k(p) + 1) / 2); }
static int64_t global_k(const gasalx_params &p) { return std::max<int64_t>(global_k0(p), 2 * (int64_t)p.gap_extend); }
static int64_t local_base(const gasalx_params &p) { return 0x400 + (int64_t)p.gap_open + p.gap_extend + local_k(p) + 16; }

// A packed kernel is exact when every stored value stays inside [0x0400, 0x7BFF] (positive normal f16
// patterns) and the score tables fit bytes: one function per frame.  LOCAL's two first (vmin 0): round-2
// keys H*256 + (255 - column), H <= 255 (unpadded lengths), 512 columns (two key sets), 256 with traceback
static bool local_key16_ok(const gasalx_params &p, uint32_t mq, uint32_t mt) {
    const int64_t a = p.match, k = local_k(p);
    if (a * std::min(mq, mt) > 255 || pad8(mt) > (p.start_pos == 2 ? 256u : 512u)) return false;
    return local_base(p) + 255 + a + k + 64 <= 0x7BFF;
}
LocalDrift local_drift_frame(const gasalx_params &p, int64_t q8, int64_t y8, int G, int R) {
    const int64_t a = std::max(p.match, 0), e = p.gap_extend, k = local_k(p);
    LocalDrift d;
    d.hmax = a * std::min(q8, y8);
    d.kc = y8 + G;
    d.window = local_base(p) + d.hmax + e * packed_span(G, R, y8) + a + k + 64 <= 0x7BFF;
    d.floor = local_base(p) - 2 * e >= 0x400;
    d.f16 = (d.hmax + e * (R - 1) + 1) * d.kc <= 0x7800;
    return d;
}

// The frames that drift (GLOBAL, SEMI, the semi-CIGAR flags): stored "minus infinity" neg, the value
// of 0 at neg + v with v below every reachable value (*vmin, set on admission), table offset k, and
// `rise`, what the frame adds over the span.  Both halves of a register hold the same cell of two
// pairs of different lengths, so one pair's pad cells share 32-bit adds with the other's real cells:
// every computed cell (register rows up to G*R, steps past the longest sequence) must stay inside the
// window or a borrow corrupts the neighbour.
static bool drift_window(const gasalx_params &p, int64_t q8, int64_t t8, int64_t k, int64_t v, int64_t rise,
                         int32_t *vmin) {
    const int64_t a = p.match, e = p.gap_extend, oe = (int64_t)p.gap_open + e;
    if (!scores_nonneg(p) || a + k > 255) return false;   // table bytes
    const int64_t neg = 0x400 + 2 * e + 16;
    if (neg + v + a * std::min(q8, t8) + a + k + oe + 64 + rise > 0x7BFF) return false;
    *vmin = (int32_t)v;
    return true;
}
// GLOBAL: values fall by at most e per row or column along a gap, and rise by the drift
bool global_window(const gasalx_params &p, int64_t q8, int64_t t8, int64_t span, int32_t *vmin) {
    const int64_t e = p.gap_extend, oe = (int64_t)p.gap_open + e, k = global_k(p);
    return drift_window(p, q8, t8, k, 4 * oe + k + e * span + 2 * e + 64, e * span, vmin);
}
// SEMI's frame (+ e per anti-diagonal, wavefront16.hpp step_semi; no floor on E/F): E and F never
// decay, every F is at least its column's top boundary and every E its row's left one, so no value
// falls below B - 3*OE whatever the span; values rise by the frame, e per row + column (the tail
// keys add up to e*(span) more to put the last row or column in one frame)
static bool semi_window(const gasalx_params &p, int64_t q8, int64_t t8, int64_t span, int32_t *vmin) {
    const int64_t e = p.gap_extend, oe = (int64_t)p.gap_open + e, k = oe + e;   // table offset K = OE + e
    if (k < p.mismatch || k < npen_of(p)) return false;                        // bytes s + K >= 0
    return drift_window(p, q8, t8, k, 4 * oe + k + 64, e * (2 * span + 1), vmin);
}
// gasalx_semi_cigar_*: the packed flags kernel (wavefront16.hpp WF16_SEMI_TB).  GLOBAL's frame and
// table offset, but not GLOBAL's bound: with the free target head values no longer fall along the top
// row.  Every cell has H >= F >= -(OE + e*r) (the insertion run from H(-1, c) = 0), stored + e*(r + c)
// >= B - OE, and the gap candidates tmp - OE >= -(2*OE + K + e*r) likewise stay within 2*OE + K + 2e
// of B whatever the span; values rise by at most a per diagonal step and by the frame, e per row + column.
// The other heads (gasalx_semi_cigar_head_*), boundary by boundary, H for the true value and B + H + e*(r + c)
// stored:
//   top, HEAD NONE / QUERY: the value above (0, c) is -(o + e*c), which falls by e per column as GLOBAL's
//     top row does -- but the frame adds e per column, so stored it is the constant B - o, the diagonal
//     into (0, c) B - 2e - o and F(0, c) B - 2o - e.  Every cell has H >= F >= -(o + e*c) - (OE + e*r), the
//     insertion run from above, stored >= B - (OE + o): no cell falls below B - 2*OE whatever the span, one
//     OE lower than under the free target head.  Gap candidates H - OE and tmp - OE stay above B - 3*OE - K.
//   left, HEAD QUERY / BOTH: H(r, -1) = 0 and E(r, c) >= -e*(c + 1), stored >= B + e*(r - 1) >= B - e;
//     stored H(r, -1) = B + e*(r - 1) rises with the row, by less than e*span over the rows a shape
//     computes (pad and register rows up to G*R included), which `rise` already holds.
//   above: H <= a * min(r + 1, c + 1) under every head (no boundary value is positive).
// So one bound serves the four heads: v = 4*OE + K + 2e + 64 lies below B - 3*OE - K - 2e.
static bool semi_cigar_window(const gasalx_params &p, int64_t q8, int64_t t8, int64_t span, int32_t *vmin) {
    const int64_t e = p.gap_extend, oe = (int64_t)p.gap_open + e, k = global_k(p);
    return drift_window(p, q8, t8, k, 4 * oe + k + 2 * e + 64, e * span, vmin);
}
// Every plan checks its window twice: over this span before the shape is known, over the chosen
// shape's packed_span after.  Neither implies the other: a shape of a forced GASALX_GMIN=64 computes
// more cells than this (G*R past the padded register axis), most shapes fewer; dropping either check
// changes plans.
static int64_t conservative_span(int64_t q8, int64_t t8) { return q8 + t8 + 2 * 64 + 8; }

// Largest |value| the DP can reach, to decide whether int32 arithmetic without
// the reference's int16 row-buffer truncation is exact.
static bool int16_safe(const gasalx_params &p, uint32_t mq, uint32_t mt) {
    const int64_t L = (int64_t)pad8(mq) + pad8(mt) + 16;
    const int64_t step = (int64_t)std::max({std::abs(p.match), std::abs(p.mismatch),
                                            p.has_n_penalty ? std::abs(p.n_penalty) : 0}) +
                         std::abs(p.gap_open) + std::abs(p.gap_extend);
    return std::abs((int64_t)p.gap_open) + L * step < 30000;
}

// Packed banded kernel (banded16.hpp): stored values B + [0, Hmax] and keys
// H*8 + 7 + 0x400 inside [0x0400, 0x7BFF]; pads score -b, which needs an N score
// <= 0.  GASALX_BAND16=0 keeps every pair on the int32 kernel (A/B runs).
static bool band16_ok(const gasalx_params &p, uint32_t q8, uint32_t t8) {
    if (!env_flag("GASALX_BAND16", true) || !scores_nonneg(p)) return false;
    if (p.match + p.mismatch > 255 || p.gap_open + p.gap_extend > 4096) return false;
    if (q8 > 65535) return false;   // the first-maximum row is tracked in 16 bits
    const int64_t hmax = (int64_t)p.match * std::min(q8, t8);
    return hmax + band16_base(p) <= 0x7BFF && hmax * 8 + 7 + 0x400 <= 0x7BFF;
}
// Packed LOCAL second-best kernel (local16.hpp): table bytes s + K in [0, 255]
// (K = max(0, b, N_PENALTY)), stored values B + [0, Hmax] and keys H*8 + 7 +
// 0x400 inside [0x0400, 0x7BFF].  GASALX_LOCAL16=0 keeps every pair on the int32
// kernel (A/B runs).
static bool local16_ok(const gasalx_params &p, uint32_t q8, uint32_t t8) {
    if (!env_flag("GASALX_LOCAL16", true)) return false;
    // (not scores_nonneg: a negative mismatch and a negative N penalty are admitted, K covers them)
    if (p.match < 0 || p.gap_open < 0 || p.gap_extend < 0 || p.gap_open + p.gap_extend > 4096) return false;
    const int64_t k = local16_k(p), sn = local16_sn(p);
    if (p.match + k > 255 || k - p.mismatch > 255 || sn + k > 255) return false;
    if (q8 > 65535 || t8 / 8 > 65535) return false;   // rows and strips are tracked in 16 bits
    // largest gain of one cell: match, a negative mismatch or a negative N penalty
    const int64_t step = std::max<int64_t>({(int64_t)p.match, -(int64_t)p.mismatch, sn});
    const int64_t hmax = step * std::min(q8, t8);
    return hmax + local16_base(p) <= 0x7BFF && hmax * 8 + 7 + 0x400 <= 0x7BFF;
}
// Packed KSW kernel (ksw16.hpp): every table byte s + K in [0, 255] (*kofs = K), queries of up to 254
// rows.  GASALX_KSW16=0: the 8-bit / 16-bit / int2 levels only.
bool ksw16_ok(const gasalx_params &p, uint32_t max_q, int32_t *kofs) {
    const int32_t nsc = local16_sn(p), k = std::max({0, p.mismatch, -nsc, -p.match});
    *kofs = k;
    // (not scores_nonneg: match, mismatch and the N penalty may have either sign, K covers them)
    return env_flag("GASALX_KSW16", true) && p.gap_open >= 0 && p.gap_extend >= 0 &&
           p.gap_open + p.gap_extend <= 0x300 && p.match + k <= 255 && -p.mismatch + k <= 255 &&
           nsc + k <= 255 && max_q <= 254;
}

// The int32 kernel's shape for q8 query rows into the plan, with its LDS per pair slot and per block
// for t8 target columns; or why there is none (a shape over the LDS limit is still written).
enum Int32Why { INT32_OK, QUERY_TOO_LONG, TARGET_TOO_LONG };
static Int32Why pick_int32_shape(Plan &pl, uint32_t q8, uint32_t t8) {
    for (const Shape &sh : kShapes)
        if ((uint32_t)(sh.G * sh.R) >= q8) {
            pl.G = sh.G; pl.R = sh.R;
            pl.lds_stride = std::max<uint32_t>(t8, 8);
            pl.lds_bytes = (size_t)kWavesPerBlock * (64 / pl.G) * pl.lds_stride;
            return pl.lds_bytes > 160 * 1024 ? TARGET_TOO_LONG : INT32_OK;
        }
    return QUERY_TOO_LONG;
}
// The packed kernels' smallest G.  Small batches: enough lanes per pair that the launch still holds
// about two waves per SIMD (128/G pairs per wave, 1024 SIMDs); traceback keeps G = 8 up.
// GASALX_GMIN: fixed minimum G (A/B runs, parity sweeps); read per call so a test process can sweep it
static uint32_t packed_gmin(uint32_t n, bool tb) {
    const int gforce = env_int("GASALX_GMIN", 0);
    if (gforce > 0) return (uint32_t)gforce;
    uint32_t gmin = 8;
    if (n && !tb)
        while (gmin < 64 && (uint64_t)n * gmin < 2048ull * 128) gmin *= 2;
    return gmin;
}
// The first packed shape with G >= gmin over x8 register-axis positions, {0, 0} when there is none.
// tb_only: the traceback kernels store flags in groups of 4 rows and keep >= 16 rows per lane above
// G = 8 (their instances, dispatch.hip wf16_pick_r4): the other shapes are never taken, forced or not
static Shape pick_packed_shape(uint32_t x8, uint32_t gmin, bool tb_only) {
    for (const Shape &sh : kShapes16)
        if ((uint32_t)sh.G >= gmin && (uint32_t)(sh.G * sh.R) >= x8 &&
            !(tb_only && (sh.R % 4 || (sh.G > 8 && sh.R < 16))))
            return sh;
    return {0, 0};
}
// the plan's packed shape and its LDS over y8 step-axis positions; false: no shape, or too much LDS
static bool set_packed_shape(Plan &pl, const Shape &sh, uint32_t y8) {
    pl.G16 = sh.G; pl.R16 = sh.R;
    pl.lds16_stride = packed_lds_stride(y8, pl.G16);
    pl.lds16_bytes = packed_lds_bytes(y8, pl.G16);
    return pl.G16 != 0 && pl.lds16_bytes <= 160 * 1024;
}
static std::string shape_name(int G, int R) { return "_G" + std::to_string(G) + "R" + std::to_string(R); }

// make_plan's steps.  The wavefront family of a request, -1 for none
static int pick_family(const gasalx_params &p) {
    // WITH_START: start.hpp (LOCAL's reversed query drops pad rows, exact unless N cells score > 0)
    if (p.algo == 3 /*LOCAL*/ && !p.second_best && !(p.start_pos == 1 && p.has_n_penalty && p.n_penalty < 0))
        return WF_LOCAL;
    if (p.algo == 1 /*GLOBAL*/) return WF_GLOBAL;
    if (p.algo == 2 /*SEMI*/ && !p.second_best && (p.start_pos != 1 || p.tail == 2)) return WF_SEMI;
    return -1;
}

// Policy, not arithmetic: the requests a packed wavefront kernel exists for.
static bool packed_family_ok(const gasalx_params &p, int wf_algo, uint32_t q8, uint32_t t8) {
    // GASALX_PACKED16=0: every block on the int32 kernel (A/B runs, the int32 probe of
    // bench.py --force-int32); read per call
    if (!env_flag("GASALX_PACKED16", true) || p.second_best) return false;
    if (wf_algo == WF_GLOBAL) {
        if (p.start_pos == 1) return false;
        // GLOBAL+TB reads the first pad query row, scored -K = -max(b, npen) there: exact for N-vs-base
        // cells only if that equals the reference's -npen, and only with the round-2 offset (K >= 2e
        // must not have raised it)
        if (p.start_pos == 2 && p.has_n_penalty && p.n_penalty < p.mismatch) return false;
        if (p.start_pos == 2 && global_k(p) != global_k0(p)) return false;
    }
    if (wf_algo == WF_SEMI) {
        if (p.start_pos == 2) return false;     // no traceback for SEMI (reference)
        // TAIL=TARGET (last query row); TAIL=QUERY/BOTH score-only through the class launches
        // (the last padded column, Q11): targets up to 256 (R <= 32), rows keyed in 16 bits
        const bool tq = p.start_pos == 0 && (p.tail == 1 || p.tail == 3);
        if (p.tail != 2 && !tq) return false;
        if (tq && (t8 > 256 || q8 > 65535)) return false;
    }
    return true;
}

// The key form of a packed LOCAL launch of shape G16 x R16.  Round-2 keys (kf16 = 0; key2: the second
// key set past 256 columns) unless the e-drift frame (wavefront16.hpp step_local_dr) holds: keys
// H*C + (C-1-c) with C = the padded target length, as f16 patterns 0x0400 + key while (Hmax + 1) * C
// <= 0x7800, as u16 integers (WF16_LOCAL_U16, one more instruction per two cells) up to 65536 --
// either covers targets past 256 columns without the second key set.  GASALX_KF16=0 keeps the
// round-2 kernel (the tests' cross-check of both key forms).  LOCAL + traceback takes the e-drift
// kernel with f16 keys (WF16_LOCAL_TBD) when they fit.  Sets pl.kf16, ku16, kseg_shift and key2.
static void local_key_form(Plan &pl, const gasalx_params &p, uint32_t q8, uint32_t y8) {
    pl.key2 = y8 > 256;
    if (!env_flag("GASALX_KF16", true)) return;
    const LocalDrift d = local_drift_frame(p, q8, y8, pl.G16, pl.R16);
    const bool frame = d.window && d.floor;
    // past both, f16 keys by step segments of M = 2^m columns (WF16_LOCAL_SEG): (Hmax +
    // 1) * M <= 0x7800 for any target length.  GASALX_KSEG=0: never, 2: before u16 keys
    const int kseg_mode = env_int("GASALX_KSEG", 1);
    uint32_t mseg = 0;
    while ((d.hmax + 1) * (int64_t)(2u << mseg) <= 0x7800 && mseg < 12) ++mseg;   // M = 2^mseg
    const bool seg_ok = frame && kseg_mode > 0 && mseg >= 2 && y8 <= 0xFFFF;
    if (frame && d.f16) {
        pl.kf16 = y8;
    } else if (pl.tb) {
        // (the traceback kernel has f16 keys only)
    } else if (seg_ok && kseg_mode == 2) {
        pl.kf16 = y8; pl.kseg_shift = mseg;
    } else if (frame && (d.hmax + 1) * d.kc <= 0x10000 && y8 <= 0xFFFF) {
        pl.kf16 = y8; pl.ku16 = true;
    } else if (seg_ok) {
        pl.kf16 = y8; pl.kseg_shift = mseg;
    }
    if (pl.kf16) pl.key2 = false;
}

// The packed half of a wavefront plan: the window before the shape is known, the shape, its LDS, the
// window again over the shape's span, LOCAL's key form.  pl.packed16 only where all of them admit.
static void plan_packed(Plan &pl, const gasalx_params &p, const BatchShape &s) {
    const uint32_t q8 = pad8(s.max_q), t8 = pad8(s.max_t);
    const bool local = pl.wf_algo == WF_LOCAL, semi = pl.wf_algo == WF_SEMI;
    const uint32_t x8 = semi ? t8 : q8, y8 = semi ? q8 : t8;   // register axis, step axis
    const auto window = [&](int64_t span) {
        return semi ? semi_window(p, q8, t8, span, &pl.vmin) : global_window(p, q8, t8, span, &pl.vmin);
    };
    // LOCAL has no window before the shape: its table bytes, and one of its two key frames can hold
    if (local ? !(scores_nonneg(p) && p.match + local_k(p) <= 255 &&
                  (local_key16_ok(p, s.max_q, s.max_t) || env_flag("GASALX_KF16", true)))
              : !window(conservative_span(q8, t8)))
        return;
    // SEMI TAIL=QUERY/BOTH: G = 8 and R = padded target / 8 per class launch (the last padded
    // column at register R - 1 of lane 7); the plan names the largest
    pl.semi_tq = semi && p.tail != 2;
    const Shape sh = pl.semi_tq ? Shape{8, (int)(x8 / 8)} : pick_packed_shape(x8, packed_gmin(s.n, pl.tb), pl.tb);
    pl.packed16 = set_packed_shape(pl, sh, y8) && (local || window(packed_span(pl.G16, pl.R16, y8)));
    if (local) {
        // (worked out whether or not the shape held: a plan that is not packed carries the fields unread)
        local_key_form(pl, p, q8, y8);
        // outside the e-drift frame the round-2 keys must hold
        if (!pl.kf16 && !local_key16_ok(p, s.max_q, s.max_t)) pl.packed16 = false;
    }
    pl.semi_tq = pl.semi_tq && pl.packed16;
}

// GLOBAL + traceback: the score sweep stores band checkpoints, a second pass recomputes each lane's
// band window with flags, the walk leaves the band only through the full-matrix fallback
// (wavefront16.hpp WF16_GLOBAL_CP / _BAND).  GASALX_TB_BAND=0: the full-matrix flags kernel (A/B);
// GASALX_TB_BAND_W: the band's half width w (window of lane lg: columns [max(lg*R - w, 0), + R + 2w))
static void plan_band(Plan &pl) {
    if (!(pl.packed16 && pl.tb && pl.wf_algo == WF_GLOBAL && pl.R16 % 4 == 0 && env_flag("GASALX_TB_BAND", true))) return;
    // w = 22: config 3's paths stray up to 20 cells from the diagonal, and any pair
    // that leaves its band costs the chain a full-matrix sweep and a second walk,
    // latency floors however few pairs they hold; w = 10 -> 22 took config 3 from
    // 2,953 to 3,647 GCUPS on one engine and 4,240 to 4,450-4,560 on three, though
    // the band pass grows by 60 % (profiles/r05/n_band_width.md)
    pl.tb_band = true;
    pl.band_w = (uint32_t)std::max(0, env_int("GASALX_TB_BAND_W", 22));
    pl.band_wd = band_window(pl.R16, pl.band_w);
}

static std::string wavefront_name(const Plan &pl, const gasalx_params &p) {
    const bool local = pl.wf_algo == WF_LOCAL;
    const std::string an = local ? (p.start_pos == 1 ? "local_start" : "local")
                         : pl.wf_algo == WF_GLOBAL ? "global"
                         : pl.semi_tq ? "semi_tq" : (p.start_pos == 1 ? "semi_start" : "semi");
    if (!pl.packed16)
        return "wavefront_" + an + (pl.tb ? "_tb" : "") + (pl.keys ? "_keys" : "") + shape_name(pl.G, pl.R);
    // (_nodrift: a LOCAL score plan outside the e-drift frame's window, the round-2 kernel)
    return "wavefront16_" + an + (pl.tb ? (pl.tb_band ? "_tbband" : "_tb") : "") + (pl.key2 ? "_k2" : "") +
           (local && !pl.tb && !pl.key2 && !pl.kf16 ? "_nodrift" : "") + (local && pl.tb && pl.kf16 ? "_dr" : "") +
           (pl.ku16 ? "_u16" : "") + (pl.kseg_shift ? "_seg" + std::to_string(1u << pl.kseg_shift) : "") +
           shape_name(pl.G16, pl.R16);
}

// the generic kernels, with their 16-bit prepass where it is exact; PLAN_NONE for any other algo
static void plan_generic(Plan &pl, const gasalx_params &p, uint32_t q8, uint32_t t8) {
    pl.name = "none";
    if (!(p.algo == 1 || p.algo == 2 || p.algo == 3 || p.algo == 5 || p.algo == 6)) return;
    pl.kind = PLAN_GENERIC; pl.need_pack = true;
    static const char *names[] = {"?", "global", "semi", "local", "?", "banded", "ksw"};
    pl.name = std::string("generic_") + names[p.algo];
    if (p.algo == 5 && band16_ok(p, q8, t8)) { pl.band16 = true; pl.name = "banded16_local"; }
    if (p.algo == 3 && p.second_best && p.start_pos == 0 && local16_ok(p, q8, t8)) {
        pl.local16 = true; pl.name = "local16_second";
    }
}

Plan make_plan(const gasalx_params &p, const BatchShape &s, bool has_ops) {
    Plan pl;
    pl.max_q = s.max_q; pl.max_t = s.max_t;
    const uint32_t q8 = pad8(s.max_q), t8 = pad8(s.max_t);
    const int wf_algo = pick_family(p);
    // SEMI TAIL=NONE, score-only: the reference keeps maxHH = MINUS_INF and the initial ends
    // (semiglobal_kernel_template.h:49-51,63-64,206-218; neither tail block runs)
    if (p.algo == 2 && p.tail == 0 && p.start_pos == 0 && !p.second_best) {
        pl.kind = PLAN_CONST; pl.name = "semi_tail_none";
        return pl;
    }
    bool ok = wf_algo >= 0 && int16_safe(p, s.max_q, s.max_t) && t8 < 32000 && p.gap_extend >= 0;
    if (wf_algo == WF_SEMI && p.start_pos == 1 && t8 > 8192) ok = false;   // stop key: strips < 1024
    if (!ok || pick_int32_shape(pl, q8, t8) != INT32_OK) {
        plan_generic(pl, p, q8, t8);
        return pl;
    }
    pl.kind = PLAN_WAVEFRONT; pl.wf_algo = wf_algo;
    pl.keys = wf_algo == WF_LOCAL || (wf_algo == WF_SEMI && (p.tail == 2 || p.tail == 3));
    pl.tb = p.start_pos == 2 && wf_algo != WF_SEMI; pl.need_pack = has_ops;
    if (packed_family_ok(p, wf_algo, q8, t8)) {
        plan_packed(pl, p, s);
        plan_band(pl);
    }
    pl.name = wavefront_name(pl, p);
    return pl;
}

Plan make_semi_cigar_plan(const gasalx_params &p, const BatchShape &s, bool has_ops, int *rc, std::string *why,
                          bool heads) {
    Plan pl;
    const std::string call = heads ? "semi_cigar_head: " : "semi_cigar: ";
    pl.max_q = s.max_q; pl.max_t = s.max_t;
    pl.name = "none";
    *rc = GASALX_OK;
    const uint32_t q8 = pad8(s.max_q), t8 = pad8(s.max_t);
    const auto refuse = [&](int code, const std::string &text) { *rc = code; *why = text; return pl; };
    // (an extension dearer than an opening, or a gap that scores: the walk's "extended" bit could then
    // name a source the maximum did not take)
    if (p.gap_open < 0 || p.gap_extend < 0)
        return refuse(GASALX_EUNSUPPORTED, call + "negative gap_open or gap_extend is not supported");
    if (!int16_safe(p, s.max_q, s.max_t) || t8 >= 32000)
        return refuse(GASALX_ERANGE, call + "lengths x scores leave the int16 range the semi-global kernels keep");
    const Int32Why i32 = pick_int32_shape(pl, q8, t8);
    const Shape &last = kShapes[sizeof(kShapes) / sizeof(kShapes[0]) - 1];
    if (i32 == QUERY_TOO_LONG)
        return refuse(GASALX_ERANGE, call + "padded query of " + std::to_string(q8) +
                                     " over the largest wavefront shape (" + std::to_string(last.G * last.R) + " rows)");
    if (i32 == TARGET_TOO_LONG)
        return refuse(GASALX_ERANGE, call + "padded target of " + std::to_string(t8) + " needs more than 160 KB of LDS");
    pl.kind = PLAN_WAVEFRONT;
    pl.wf_algo = WF_GLOBAL;   // query rows in registers, target on the step axis
    pl.semi_tb = true; pl.tb = true; pl.need_pack = has_ops;
    pl.semi_heads = heads && p.head != 2;   // HEAD = TARGET: gasalx_semi_cigar_*'s instances
    if (env_flag("GASALX_PACKED16", true) && semi_cigar_window(p, q8, t8, conservative_span(q8, t8), &pl.vmin))
        // the traceback shapes; n does not widen G (traceback keeps G = 8 up)
        pl.packed16 = set_packed_shape(pl, pick_packed_shape(q8, packed_gmin(0, true), true), t8) &&
                      semi_cigar_window(p, q8, t8, packed_span(pl.G16, pl.R16, t8), &pl.vmin);
    pl.name = pl.packed16 ? "wavefront16_semi_tb" + shape_name(pl.G16, pl.R16)
                          : "wavefront_semi_tb" + shape_name(pl.G, pl.R);
    if (heads) pl.name += std::string("_h") + "nqtb"[p.head & 3];
    return pl;
}

}  // namespace gx
