// Host-only check of include/nvbio_batched.h's quality-aware Gotoh scheme: no GPU and no libgasal.
// The flat C API entry points are stubs that record their arguments.  The three cost functions and
// QualityGotohScheme must give the values worked by hand from nvBowtie's lines (scoring.h:97-101,
// :286-291, quality_coeffs.h:44-54); a GotohAligner over the scheme must reach
// gasalx_nv_banded_qual_score_device through BatchedBandedAlignmentScore::enact and
// batch_banded_alignment_score, and gasalx_nv_banded_qual_traceback_device through
// BatchedBandedAlignmentTraceback::enact, with the scheme's tables, levels and gap scores and the
// stream's qualities.  The compile-time refusals, one macro each (the file must then fail to compile):
//   -DCHECK_SW_OVER_QUALS_REFUSED          SmithWatermanAligner over QualityGotohScheme
//   -DCHECK_FULL_SCORE_OVER_QUALS_REFUSED  BatchedAlignmentScore with the quality aligner
//   -DCHECK_FREE_SCORE_OVER_QUALS_REFUSED  batch_alignment_score with it
//   -DCHECK_FULL_TRACEBACK_OVER_QUALS_REFUSED  BatchedAlignmentTraceback with it
#include <stdio.h>
#include <string.h>

#include "nvbio_batched.h"

namespace {
struct Call {
    int which = 0;   // 1 the scorer, 2 the traceback
    gasalx_nv_aligner al;
    gasalx_nv_quals q;
    uint32_t band, n, max_p;
    const void *scores, *sinks, *sources, *ops;
    uint32_t ops_stride;
};
Call last;
int failures = 0;
gasalx_engine *const kEngine = reinterpret_cast<gasalx_engine *>(0x10);
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) { printf("line %d: %s\n", __LINE__, #c); failures++; } \
    } while (0)
}  // namespace

extern "C" {
int gasalx_engine_create(int, gasalx_engine **out) { *out = kEngine; return GASALX_OK; }
const char *gasalx_last_error(void) { return "stub"; }
uint64_t gasalx_nv_banded_traceback_workspace(uint32_t, uint32_t, uint32_t) { return 0; }
uint64_t gasalx_nv_traceback_workspace(uint32_t, uint32_t, uint32_t) { return 0; }
int gasalx_nv_banded_qual_score_device(gasalx_engine *, const gasalx_nv_aligner *al, const gasalx_nv_quals *q, uint32_t band,
                                       uint32_t n, const gasalx_nv_strings *, const gasalx_nv_strings *, int32_t *scores,
                                       uint32_t *sinks, uint32_t max_p, void *) {
    last = Call{1, *al, *q, band, n, max_p, scores, sinks, nullptr, nullptr, 0};
    return GASALX_OK;
}
int gasalx_nv_banded_qual_traceback_device(gasalx_engine *, const gasalx_nv_aligner *al, const gasalx_nv_quals *q,
                                           uint32_t band, uint32_t n, const gasalx_nv_strings *, const gasalx_nv_strings *,
                                           uint32_t max_p, int32_t *scores, uint32_t *sources, uint32_t *sinks, uint8_t *ops,
                                           uint32_t ops_stride, uint32_t *, void *) {
    last = Call{2, *al, *q, band, n, max_p, scores, sinks, sources, ops, ops_stride};
    return GASALX_OK;
}
}

using namespace nvbio;
using namespace nvbio::aln;

int main() {
    // QualCost(2, 6): 2 + int(min(q, 40) / 40.0f * 4): q = 9 -> int(0.9) = 0, 10 -> 1, 39 -> int(3.9) = 3, 40 and up -> 4
    const QualCost mmp(2, 6);
    EXPECT(mmp(0) == 2 && mmp(9) == 2 && mmp(10) == 3 && mmp(39) == 5 && mmp(40) == 6 && mmp(41) == 6 && mmp(255) == 6);
    EXPECT(ConstantCost(7)(0) == 7 && ConstantCost(7)(200) == 7);
    const RoundedQualCost rq;
    EXPECT(rq(0) == 0 && rq(4) == 0 && rq(5) == 10 && rq(14) == 10 && rq(15) == 20 && rq(24) == 20 && rq(25) == 30 && rq(255) == 30);

    const QualityGotohScheme def = QualityGotohScheme::nvbowtie_default();
    EXPECT(def.m_levels == 256 && def.match(30) == 0 && def.mismatch(0) == -2 && def.mismatch(20) == -4 &&
           def.mismatch(255) == -6);
    EXPECT(def.pattern_gap_open() == -8 && def.pattern_gap_extension() == -3);
    EXPECT(def.substitution(0, 0, 1, 1, 40) == 0 && def.substitution(0, 0, 1, 2, 40) == -6 && def.substitution(0, 0, 255, 2, 3) == -2);
    const QualityGotohScheme shrt(ConstantCost(1), QualCost(2, 6), -5, -2, 11);   // a quality >= levels reads the last entry
    EXPECT(shrt.m_levels == 11 && shrt.mismatch(10) == -3 && shrt.mismatch(200) == -3 && shrt.match(200) == 1);

    typedef GotohAligner<SEMI_GLOBAL, QualityGotohScheme> aligner_type;
    const aligner_type aligner = make_gotoh_aligner<SEMI_GLOBAL>(def);
    const gasalx_nv_aligner ca = aligner.c_aligner();
    EXPECT(ca.aligner == GASALX_NV_GOTOH && ca.type == 2 && ca.gap_open == -8 && ca.gap_ext == -3);
    uint32 words[4] = {}, offs[3] = {0, 3, 7}, sinks[4];
    int32 scores[2];
    uint8 quals[8] = {}, ops[64];
    uint32 src[4], nops[2];

    AlignmentStream<aligner_type> s(aligner, 2, offs, words, 4, 7, words, 0, NULL);
    s.m_text_offsets = offs; s.m_scores32 = scores; s.m_sinks = sinks;
    s.set_quals(quals);
    BatchedBandedAlignmentScore<15, AlignmentStream<aligner_type> > scorer;
    scorer.enact(s);
    EXPECT(last.which == 1 && last.band == 15 && last.n == 2 && last.max_p == 4 && last.q.quals == quals &&
           last.q.levels == 256 && last.q.mismatch[40] == -6 && last.q.match[0] == 0 && last.scores == scores &&
           last.sinks == sinks);

    last = Call();
    const PackedStringSet set(2, words, offs, 4, 1), tset(2, words, offs, 2, 0);
    const BestSinks best = {scores, NULL};
    batch_banded_alignment_score<7>(aligner, set, tset, best, DeviceThreadScheduler(), 4, 10, quals);
    EXPECT(last.which == 1 && last.band == 7 && last.q.quals == quals && last.sinks == NULL && last.scores == scores);

    last = Call();
    TracebackStream<aligner_type> t(aligner, 2, offs, words, 4, 7, words, 0, scores, src, sinks, ops, 23, nops);
    t.m_text_offsets = offs;
    t.set_quals(quals);
    BatchedBandedAlignmentTraceback<15, 32, TracebackStream<aligner_type> > tb;
    tb.enact(t);
    EXPECT(last.which == 2 && last.band == 15 && last.q.quals == quals && last.q.levels == 256 && last.sources == src &&
           last.ops == ops && last.ops_stride == 23 && last.al.gap_open == -8);

#if defined(CHECK_SW_OVER_QUALS_REFUSED)
    SmithWatermanAligner<LOCAL, QualityGotohScheme> sw;
    (void)sw;
#endif
#if defined(CHECK_FULL_SCORE_OVER_QUALS_REFUSED)
    BatchedAlignmentScore<AlignmentStream<aligner_type>, DeviceThreadScheduler> full;
    full.enact(s);
#endif
#if defined(CHECK_FREE_SCORE_OVER_QUALS_REFUSED)
    batch_alignment_score(aligner, set, tset, best, DeviceThreadScheduler());
#endif
#if defined(CHECK_FULL_TRACEBACK_OVER_QUALS_REFUSED)
    BatchedAlignmentTraceback<32, TracebackStream<aligner_type> > ftb;
    ftb.enact(t);
#endif
    printf(failures ? "%d failures\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
