// Host-only check of include/nvbio_batched.h's sink plumbing: no GPU and no libgasal.  The
// flat C API entry points BatchedAlignmentScore::enact calls are stubs here that record their
// arguments: a TextBlockingTag stream with sinks set must reach gasalx_nv_score_sinks_device
// with the stream's pointers, the same enact without sinks must make the score-only call with
// the arguments it always made, and a PatternBlockingTag stream must still score.
// (AlignmentStream::set_sinks on a PatternBlockingTag aligner is a static_assert: compile this
// file with -DCHECK_PATTERN_TAG_REFUSED to see it fire.)
#include <stdio.h>
#include <string.h>

#include "nvbio_batched.h"

namespace {
struct Call {
    int which = 0;   // 1 score, 2 score + sinks
    gasalx_nv_aligner al;
    uint32_t n, max_p, max_t;
    gasalx_nv_strings p, t;
    const void *scores, *scores16, *sinks, *stream;
};
Call last;
int n_calls = 0, failures = 0;
gasalx_engine *const kEngine = reinterpret_cast<gasalx_engine *>(0x10);
}  // namespace

extern "C" {
int gasalx_engine_create(int, gasalx_engine **out) { *out = kEngine; return GASALX_OK; }
const char *gasalx_last_error(void) { return "stub"; }
int gasalx_nv_score_device(gasalx_engine *eng, const gasalx_nv_aligner *al, uint32_t n, const gasalx_nv_strings *p,
                           const gasalx_nv_strings *t, int32_t *scores, int16_t *scores16, uint32_t max_p,
                           uint32_t max_t, void *stream) {
    if (eng != kEngine) return GASALX_EINVAL;
    last = Call{1, *al, n, max_p, max_t, *p, *t, scores, scores16, nullptr, stream};
    n_calls++;
    return GASALX_OK;
}
int gasalx_nv_score_sinks_device(gasalx_engine *eng, const gasalx_nv_aligner *al, uint32_t n,
                                 const gasalx_nv_strings *p, const gasalx_nv_strings *t, int32_t *scores,
                                 uint32_t *sinks, uint32_t max_p, uint32_t max_t, void *stream) {
    if (eng != kEngine) return GASALX_EINVAL;
    last = Call{2, *al, n, max_p, max_t, *p, *t, scores, nullptr, sinks, stream};
    n_calls++;
    return GASALX_OK;
}
}

#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

int main() {
    using namespace nvbio;
    using namespace nvbio::aln;
    static uint32 offsets[3] = {0, 5, 9}, patterns[2], text[2], text_offsets[3] = {0, 7, 20}, sinks[4];
    static int32 scores32[2];
    static int16 scores16[2];
    int marker = 0;
    const SimpleGotohScheme scheme(2, -1, -2, -1);

    auto text_al = make_gotoh_aligner<LOCAL, TextBlockingTag>(scheme);
    typedef AlignmentStream<decltype(text_al)> text_stream;
    auto check_strings = [&](const Call &c, bool per_pair) {
        EXPECT(c.n == 2 && c.max_p == 5 && c.max_t == 13);
        EXPECT(c.al.aligner == GASALX_NV_GOTOH && c.al.type == GASALX_NV_LOCAL && c.al.match == 2 && c.al.mismatch == -1 &&
               c.al.gap_open == -2 && c.al.gap_ext == -1);
        EXPECT(c.p.words == patterns && c.p.offsets == offsets && c.p.bits == 4 && c.p.big_endian == 1);
        EXPECT(c.t.words == text && c.t.offsets == (per_pair ? text_offsets : nullptr) && c.t.length == 13 &&
               c.t.bits == 2 && c.t.big_endian == 0);
        EXPECT(c.stream == &marker);
    };

    {   // sinks set: the sinks entry point, with the stream's own pointers
        text_stream s(text_al, 2, offsets, patterns, 5, 9, text, 13, nullptr);
        s.m_scores32 = scores32;
        s.m_text_offsets = text_offsets;
        s.set_sinks(sinks);
        BatchedAlignmentScore<text_stream, DeviceThreadScheduler> batch;
        batch.enact(s, 0, nullptr, &marker);
        EXPECT(n_calls == 1 && last.which == 2 && last.sinks == sinks && last.scores == scores32);
        check_strings(last, true);
        // sinks alone
        s.m_scores32 = nullptr;
        batch.enact(s, 0, nullptr, &marker);
        EXPECT(n_calls == 2 && last.which == 2 && last.sinks == sinks && last.scores == nullptr);
    }
    {   // sinks unset: today's score-only call, int16 and int32 scores as before
        text_stream s(text_al, 2, offsets, patterns, 5, 9, text, 13, scores16);
        s.m_scores32 = scores32;
        BatchedAlignmentScore<text_stream, DeviceThreadScheduler> batch;
        batch.enact(s, 0, nullptr, &marker);
        EXPECT(n_calls == 3 && last.which == 1 && last.sinks == nullptr && last.scores == scores32 &&
               last.scores16 == scores16);
        check_strings(last, false);
    }
    {   // PatternBlockingTag (the default tag): score-only calls are accepted as ever
        auto pat_al = make_gotoh_aligner<LOCAL>(scheme);
        typedef AlignmentStream<decltype(pat_al)> pat_stream;
        pat_stream s(pat_al, 2, offsets, patterns, 5, 9, text, 13, scores16);
#ifdef CHECK_PATTERN_TAG_REFUSED
        s.set_sinks(sinks);   // static_assert: sinks are provided for TextBlockingTag aligners only
#endif
        BatchedAlignmentScore<pat_stream, DeviceThreadScheduler> batch;
        batch.enact(s, 0, nullptr, &marker);
        EXPECT(n_calls == 4 && last.which == 1 && last.scores16 == scores16 && last.scores == nullptr);
        check_strings(last, false);
    }
    if (failures) { fprintf(stderr, "nvbio_sinks_header_check: %d failure(s)\n", failures); return 1; }
    printf("nvbio_sinks_header_check ok\n");
    return 0;
}
