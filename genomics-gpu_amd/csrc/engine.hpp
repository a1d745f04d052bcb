// engine.hpp — host-side dispatcher of the MI355X engine.
//
// Replaces gasal_kernel_launcher + the KERNEL_SWITCH macro tree
// (Non-CDP/GASAL2/src/gasal_align.cu:10-25, gasal_align.h:7-107) and the CDP
// launch wrappers (CDP/GASAL2/src/gasal_align.cu:27-52) by one flat planner:
// (algo, start, head, tail, secondBest, lengths) -> one kernel family + launch
// shape, all launched from the host on one hipStream_t.  No device-side enqueue.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "gasalx.h"

namespace gx {

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t need);   // grow-only
    void release();
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

struct Workspace {
    int device = 0;
    DevBuf packed_q, packed_t;      // packed words (RC / generic paths)
    DevBuf tb;                      // traceback direction words
    DevBuf rows_h, rows_e, rev;     // generic kernels' row buffers
    DevBuf ends_q, ends_t;          // LOCAL WITH_TB ends when the caller did not ask for them
    DevBuf misc;                    // packed kernels: per-block "aligned here" flags
    DevBuf aux;                     // packed GLOBAL+TB: H' of the traceback start cell per pair
    DevBuf rev_meta;                // WITH_START: reversed lengths, slot order, reverse-pass results
    DevBuf sort_meta;               // length sort of the forward pass: perm, inverse, histogram
    DevBuf band_cp, band_stm, band_fl;   // GLOBAL+TB band recomputation: checkpoints, hand-offs, flags
    DevBuf band_fb;                 // its fallback: count, then the list of pairs, then the launch's flags
    DevBuf kseg;                    // packed LOCAL keys by segments: the finished segments' keys per wave
    // the last packed launch's "aligned here" flags in misc (gasalx_packed_pairs): flag count, pairs
    // per flag, pairs of the launch (0 flags: no packed launch yet)
    uint32_t pk_flags = 0, pk_ppb = 0, pk_pairs = 0;
    // a mixed-shape launch (wavefront16.hpp wf16_mix_kernel): flags from pk_b1 on cover pk_ppb2 pairs
    // each, from pair pk_p1 on (pk_p1 = 0xFFFFFFFF: one block size)
    uint32_t pk_p1 = 0xFFFFFFFFu, pk_b1 = 0, pk_ppb2 = 1;
    int cus = 0;                    // CU count of `device`, asked on first use (0: not yet)
    void release_all();
};

// a length padded to whole 8-base words
inline uint32_t pad8(uint32_t x) { return (x + 7u) & ~7u; }

template <class T> struct LaunchArg { using type = T; };
// Launch kernel fn(args...) with `lds` bytes of dynamic LDS, raising the kernel's limit first when
// that is past the 64 KB default; the error of either step, or of the launch.
template <class... P>
hipError_t launch_lds(void (*fn)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st,
                      const typename LaunchArg<P>::type &...args) {
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    void *argv[] = {const_cast<void *>(static_cast<const void *>(&args))...};
    hipError_t e = hipLaunchKernel((const void *)fn, grid, block, argv, lds, st);
    return e != hipSuccess ? e : hipGetLastError();
}

// PLAN_CONST: outputs that do not depend on the DP (SEMI TAIL=NONE, score-only)
enum PlanKind { PLAN_NONE = 0, PLAN_WAVEFRONT, PLAN_GENERIC, PLAN_CONST };

struct Plan {
    PlanKind kind = PLAN_NONE;
    int wf_algo = 0;        // WfAlgo
    bool keys = false, tb = false;
    bool packed16 = false;  // two pairs per lane in 16-bit halves (wavefront16.hpp), int32 fallback
    bool key2 = false;      // packed LOCAL over 257..512 target columns (second key set)
    int G16 = 0, R16 = 0;   // packed kernel shape
    uint32_t lds16_stride = 0;
    size_t lds16_bytes = 0;
    int32_t vmin = 0;       // packed GLOBAL/SEMI value-range bound
    uint32_t kf16 = 0;      // packed LOCAL: f16-pattern key columns (wavefront16.hpp step_local KU), 0 = 16-bit keys
    bool ku16 = false;      // packed LOCAL in the e-drift frame with u16 keys (WF16_LOCAL_U16)
    uint32_t kseg_shift = 0; // packed LOCAL with f16 keys by step segments of 2^kseg_shift (WF16_LOCAL_SEG), 0 = off
    int G = 0, R = 0;
    uint32_t lds_stride = 0;
    size_t lds_bytes = 0;
    bool need_pack = false; // generic kernels / reverse-complement need packed words
    bool band16 = false;    // banded: two pairs per lane in 16-bit halves (banded16.hpp), int32 fallback
    bool local16 = false;   // LOCAL second best: two pairs per lane in 16-bit halves (local16.hpp), int32 fallback
    bool semi_tq = false;   // SEMI TAIL=QUERY/BOTH: packed class launches (one per padded target length), int32 fallback
    bool tb_band = false;   // packed GLOBAL+TB by band recomputation (wavefront16.hpp WF16_GLOBAL_CP / _BAND)
    uint32_t band_w = 0, band_wd = 0;
    bool semi_tb = false;   // the direction-flag launch of gasalx_semi_cigar_* (make_semi_cigar_plan): GLOBAL's
                            // traceback kernels under the semi-global boundary (WF16_SEMI_TB / SEMITB)
    bool semi_heads = false;   // semi_tb under the boundary of params.head (gasalx_semi_cigar_head_* with HEAD
                               // NONE, QUERY or BOTH: WF16_SEMI_TBH / SEMITB = 2); HEAD = TARGET keeps semi_tb's
    uint32_t max_q = 0, max_t = 0;   // the batch shape the plan was made for
    std::string name;
};

// Host-visible summary of a batch needed for planning.
struct BatchShape {
    uint32_t max_q = 0, max_t = 0;
    bool sort = false;   // lengths are uneven: run the wavefront kernels over pairs sorted by step-axis length
    uint32_t n = 0;      // pairs in the launch (0 = unknown: shapes for large batches)
    bool tb_split = true; // traceback: chunks on two streams so a chunk's walk overlaps the next DP
    bool one_t8 = false;  // host-side lengths: every padded target length is the same (SEMI TAIL=QUERY/BOTH
                          // then launches its one class without reading the class histogram back)
};

// The planner (plan.cpp, host only; what the launch code shares with it: plan.hpp).  has_ops: the
// batch carries reverse / complement ops.
Plan make_plan(const gasalx_params &p, const BatchShape &shape, bool has_ops);

// The direction-flag launch of gasalx_semi_cigar_* (SEMI-GLOBAL, HEAD = TAIL = TARGET, with CIGARs):
// PLAN_WAVEFRONT, or PLAN_NONE with *why and a GASALX_E* code in *rc when the scores or the lengths
// have no wavefront form.  The score launch that runs before it is make_plan's, unchanged.
// heads: gasalx_semi_cigar_head_* -- p.head is any of the four (TAIL = TARGET), the name carries the head
// (_hn, _hq, _ht, _hb) and refusals the prefix "semi_cigar_head:"; HEAD = TARGET is the same plan otherwise.
Plan make_semi_cigar_plan(const gasalx_params &p, const BatchShape &shape, bool has_ops, int *rc, std::string *why,
                          bool heads = false);

// Host-side check for BatchShape::sort: the padded lengths of the step axis
// (targets; queries for SEMI-GLOBAL, whose kernel runs transposed) spread over
// at least two 8-base words.
inline bool uneven_lengths(const gasalx_params &p, const uint32_t *q_lens, const uint32_t *t_lens, uint32_t n) {
    const uint32_t *l = p.algo == 2 ? q_lens : t_lens;
    if (!l || n == 0) return false;
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t w = (l[i] + 7) >> 3;
        lo = w < lo ? w : lo;
        hi = w > hi ? w : hi;
    }
    return hi >= lo + 2;
}

// Host-side check for BatchShape::one_t8: one padded target length in the batch, and it is the
// padded max_t the plan is sized for (a caller's max_t_len is only an upper bound, and a chunk of
// the host pipeline may hold only shorter targets: the class launch then covers no pair, so the
// histogram decides)
inline bool one_pad8(const uint32_t *t_lens, uint32_t n, uint32_t max_t) {
    if (!t_lens || n == 0) return false;
    const uint32_t w = (t_lens[0] + 7) >> 3;
    if (w != (max_t + 7) >> 3) return false;
    for (uint32_t i = 1; i < n; i++)
        if (((t_lens[i] + 7) >> 3) != w) return false;
    return true;
}

// Launch the full path for a device-resident batch on `stream`.
// Returns GASALX_OK or an error code; sets the thread's last error message.
// cigar_cap: bytes writable at out.cigar (0 = b.q_bytes)
int align_device(Workspace &ws, const gasalx_params &p, const gasalx_batch &b, const gasalx_results &out,
                 hipStream_t stream, const BatchShape &shape, uint64_t cigar_cap = 0);

// SEMI-GLOBAL with HEAD = TAIL = TARGET and the alignment itself: the score launch of align_device
// (score, ends), the direction-flag launch, the walk (CIGAR bytes, op counts, starts).  sort_t: the
// target lengths are uneven (the flag launch runs its slots in target-length order).
// heads: gasalx_semi_cigar_head_* (p.head kept: any HEAD, and q_start written); false forces HEAD = TARGET.
int semi_cigar_device(Workspace &ws, const gasalx_params &p, const gasalx_batch &b, const gasalx_results &out,
                      hipStream_t stream, const BatchShape &shape, bool sort_t, bool heads = false);

int pairhmm_device(Workspace &ws, const gasalx_hmm_batch &b, float *result, hipStream_t stream, uint32_t max_r,
                   uint32_t max_h);

// PairHMM from Phred qualities.  ph2pr_dev: the 128-entry table in device memory.
// With perm/classes (host path): slots sorted by (read, haplotype) length, one launch
// per class of slots sharing a lane-group size; otherwise one launch over all pairs.
struct HmmClass { uint32_t slot0, slot1, max_r, max_h; };
int pairhmm_group(uint32_t max_r);
int pairhmm_quals_device(Workspace &ws, const gasalx_hmm_qual_batch &b, float *result, hipStream_t stream,
                         const float *ph2pr_dev, const uint32_t *perm, const HmmClass *classes, int n_classes,
                         uint32_t max_r, uint32_t max_h);

// PairHMM in float64 (pairhmm64.hip, pairhmm64.hpp).  The pairs come in either input form:
// quals (with ph2pr, the 128-entry device table) when set, otherwise params.
struct Hmm64Src {
    const gasalx_hmm_batch *params;
    const gasalx_hmm_qual_batch *quals;
    const float *ph2pr;
};
// lanes per pair and read rows per lane for reads of up to max_r rows (0: longer than 512)
int pairhmm64_shape(uint32_t max_r, int *rows);
// the raw forward value of every pair, initial constant 2^1020
int pairhmm64_device(const Hmm64Src &src, uint32_t n, double *result, hipStream_t stream, uint32_t max_r,
                     uint32_t max_h);
// log10 likelihoods from the fp32 results r32: accepted pairs (r >= min_accepted, <= 0: 1e-28f,
// and finite) directly, the others recomputed in float64.  count (one word) and list (n words)
// are device scratch; count holds the number of rescued pairs afterwards.  No host round trip.
int pairhmm_log10_device(const Hmm64Src &src, uint32_t n, const float *r32, float min_accepted, double *out,
                         uint8_t *used, uint32_t *count, uint32_t *list, hipStream_t stream, uint32_t max_r,
                         uint32_t max_h);

// nvbio-style batched scoring (batched.hip, nvbio.hpp)
int nv_score_device(const gasalx_nv_aligner &al, uint32_t n, const gasalx_nv_strings &pat,
                    const gasalx_nv_strings &txt, int32_t *scores, int16_t *scores16, uint32_t max_p, uint32_t max_t,
                    hipStream_t stream);
// the same with the BestSink position (nvbio_sink.hpp): sinks[2k] = x (text), sinks[2k + 1] = y
// (pattern), one-based; scores or sinks may be NULL
int nv_score_sinks_device(const gasalx_nv_aligner &al, uint32_t n, const gasalx_nv_strings &pat,
                          const gasalx_nv_strings &txt, int32_t *scores, uint32_t *sinks, uint32_t max_p,
                          uint32_t max_t, hipStream_t stream);
std::string nv_sinks_plan_name(const gasalx_nv_aligner &al, uint32_t max_p, uint32_t max_t, bool per_pair_text,
                               uint32_t text_bits);
// GotohAligner over a substitution matrix (nvmatrix.hpp): S = mat.scores[t + p * n] from a host table
// read during the call, symbols >= n clamped to n - 1; al.match / al.mismatch are not read.  sinks as
// nv_score_sinks_device (NULL: the score-only kernel); scores or sinks may be NULL
int nv_matrix_score_device(const gasalx_nv_aligner &al, const gasalx_nv_matrix &mat, uint32_t n,
                           const gasalx_nv_strings &pat, const gasalx_nv_strings &txt, int32_t *scores, uint32_t *sinks,
                           uint32_t max_p, uint32_t max_t, hipStream_t stream);
// its kernel's name ("nvbio_matrix_gotoh_local_G8R16_sink", or "none"), or the code the call would return
int nv_matrix_plan_name(const gasalx_nv_aligner &al, uint32_t matrix_n, uint32_t max_p, uint32_t max_t,
                        bool per_pair_text, bool sinks, std::string &name);
// nvbio BatchedBandedAlignmentScore<band> (batched.hip / nvbanded.hpp): BestSink score per pair
// max_p: the longest pattern (0: unknown; the packed kernel needs it for its value window)
int nv_banded_score_device(const gasalx_nv_aligner &al, uint32_t band, uint32_t n, const gasalx_nv_strings &pat,
                           const gasalx_nv_strings &txt, int32_t *scores, hipStream_t st, uint32_t max_p);
// the same with the BestSink position (nvbanded_sink.hpp; sinks as nv_score_sinks_device); scores or
// sinks may be NULL
int nv_banded_score_sinks_device(const gasalx_nv_aligner &al, uint32_t band, uint32_t n, const gasalx_nv_strings &pat,
                                 const gasalx_nv_strings &txt, int32_t *scores, uint32_t *sinks, hipStream_t st,
                                 uint32_t max_p);
// its kernel's name ("nvbio_banded16_gotoh_local_b16_sink"), or the code the call would return
int nv_banded_sinks_plan_name(const gasalx_nv_aligner &al, uint32_t band, uint32_t max_p, uint32_t text_bits,
                              std::string &name);
// EditDistanceAligner<TYPE, MyersTag<alphabet>> under the same banded scorer (nvmyers.hpp): BestSink
// score and position per pair (sinks as nv_score_sinks_device); scores or sinks may be NULL
int nv_banded_myers_device(int32_t type, uint32_t alphabet, uint32_t band, uint32_t n, const gasalx_nv_strings &pat,
                           const gasalx_nv_strings &txt, int32_t *scores, uint32_t *sinks, hipStream_t st);
// its kernel's name ("nvbio_myers_semi_a5"), or the code the call would return
int nv_myers_plan_name(int32_t type, uint32_t alphabet, uint32_t band, std::string &name);
int nv_traceback_device(const gasalx_nv_aligner &al, uint32_t n, const gasalx_nv_strings &pat,
                        const gasalx_nv_strings &txt, uint32_t max_p, uint32_t max_t, uint8_t *dir, int32_t *row,
                        int32_t *score, uint32_t *src, uint32_t *snk, uint8_t *ops, uint32_t ops_stride,
                        uint32_t *n_ops, hipStream_t st);
// the full-DP traceback of GotohAligner over a substitution matrix (nvmatrix_trace.hpp): workspace and
// outputs as nv_traceback_device, the table as nv_matrix_score_device.  The check runs what needs no
// lengths (aligner and table size, the table, symbol bits) and gives the largest |entry|.
int nv_matrix_traceback_check(const gasalx_nv_aligner &al, const gasalx_nv_matrix &mat, const gasalx_nv_strings &pat,
                              const gasalx_nv_strings &txt, int32_t *entry_mag);
int nv_matrix_traceback_device(const gasalx_nv_aligner &al, const gasalx_nv_matrix &mat, uint32_t n,
                               const gasalx_nv_strings &pat, const gasalx_nv_strings &txt, uint32_t max_p,
                               uint32_t max_t, uint8_t *dir, int32_t *row, int32_t *score, uint32_t *src,
                               uint32_t *snk, uint8_t *ops, uint32_t ops_stride, uint32_t *n_ops, hipStream_t st);
int nv_banded_traceback_device(const gasalx_nv_aligner &al, uint32_t band, uint32_t n, const gasalx_nv_strings &pat,
                               const gasalx_nv_strings &txt, uint32_t max_p, uint32_t *dir, int32_t *score,
                               uint32_t *src, uint32_t *snk, uint8_t *ops, uint32_t ops_stride, uint32_t *n_ops,
                               hipStream_t st);
std::string nv_plan_name(const gasalx_nv_aligner &al, uint32_t max_p, uint32_t max_t, bool per_pair_text,
                         uint32_t text_bits);
// The banded Gotoh scorer (with sinks) and the banded traceback under a quality-aware scheme
// (nvbanded_qual.hpp): q->quals a device array indexed by the pattern offsets, the two tables host
// arrays read during the call; al.match / al.mismatch are not read.  Outputs and workspace as
// nv_banded_score_sinks_device and nv_banded_traceback_device.  The check runs what needs no lengths,
// in the entry points' order (bytes: the call reads q->quals), and gives the largest |entry|.
int nv_banded_qual_check(const gasalx_nv_aligner &al, const gasalx_nv_quals *q, bool bytes, uint32_t band,
                         const gasalx_nv_strings &pat, const gasalx_nv_strings &txt, int32_t *entry_mag);
int nv_banded_qual_score_device(const gasalx_nv_aligner &al, const gasalx_nv_quals *q, uint32_t band, uint32_t n,
                                const gasalx_nv_strings &pat, const gasalx_nv_strings &txt, int32_t *scores,
                                uint32_t *sinks, hipStream_t st, uint32_t max_p);
int nv_banded_qual_traceback_device(const gasalx_nv_aligner &al, const gasalx_nv_quals *q, uint32_t band, uint32_t n,
                                    const gasalx_nv_strings &pat, const gasalx_nv_strings &txt, uint32_t max_p,
                                    uint32_t *dir, int32_t *score, uint32_t *src, uint32_t *snk, uint8_t *ops,
                                    uint32_t ops_stride, uint32_t *n_ops, hipStream_t st);
// the kernel's name ("nvbio_banded16_qual_gotoh_local_b16_sink"), or the code the call would return
int nv_banded_qual_plan_name(const gasalx_nv_aligner &al, const gasalx_nv_quals *q, uint32_t band, uint32_t max_p,
                             uint32_t text_bits, bool traceback, std::string &name);

// The engine's own stream (capi.cpp; gasalx_engine is opaque elsewhere).
hipStream_t engine_stream(gasalx_engine *e);

void set_error(const std::string &msg);
const char *last_error();

// An environment switch (A/B runs, the tests' cross-checks): the variable read as an integer, or
// `dflt` when unset.  Read at every call, so one process can sweep a switch.
inline int env_int(const char *name, int dflt) {
    const char *e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}
inline bool env_flag(const char *name, bool dflt) { return env_int(name, dflt ? 1 : 0) != 0; }

}  // namespace gx
