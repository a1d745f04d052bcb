// Host-only check of include/nvbio_batched.h's substitution-matrix routing: no GPU and no libgasal.
// The flat C API entry points are stubs that record their arguments.  A GotohAligner over
// SubstitutionMatrixScheme must reach gasalx_nv_matrix_score_device with the scheme's table and gap
// scores, through BatchedAlignmentScore::enact and through batch_alignment_score over 8-bit
// ConcatenatedStringSets; a Simple scheme through the same free function must make the calls it always
// made.  BatchedAlignmentTraceback::enact over a TracebackStream of the matrix aligner must reach
// gasalx_nv_matrix_traceback_device with the table, n, the gap scores and every output pointer, and a
// Simple-scheme stream must still reach gasalx_nv_traceback_device.  The compile-time refusals, one
// macro each (the file must then fail to compile):
//   -DCHECK_SW_OVER_MATRIX_REFUSED       SmithWatermanAligner over SubstitutionMatrixScheme
//   -DCHECK_BANDED_OVER_MATRIX_REFUSED   BatchedBandedAlignmentScore with the matrix aligner
//   -DCHECK_BANDED_TRACEBACK_OVER_MATRIX_REFUSED  BatchedBandedAlignmentTraceback with it
#include <stdio.h>
#include <string.h>

#include "nvbio_batched.h"

namespace {
struct Call {
    int which = 0;   // 1 score, 2 score + sinks, 3 matrix, 4 traceback, 5 matrix traceback
    gasalx_nv_aligner al;
    gasalx_nv_matrix mat;
    uint32_t n, max_p, max_t;
    gasalx_nv_strings p, t;
    const void *scores, *sinks;
    const void *sources = nullptr, *ops = nullptr, *n_ops = nullptr, *stream = nullptr;   // the tracebacks
    uint32_t ops_stride = 0;
};
Call last;
int n_calls = 0, failures = 0;
gasalx_engine *const kEngine = reinterpret_cast<gasalx_engine *>(0x10);
}  // namespace

extern "C" {
int gasalx_engine_create(int, gasalx_engine **out) { *out = kEngine; return GASALX_OK; }
const char *gasalx_last_error(void) { return "stub"; }
int gasalx_nv_score_device(gasalx_engine *, const gasalx_nv_aligner *al, uint32_t n, const gasalx_nv_strings *p,
                           const gasalx_nv_strings *t, int32_t *scores, int16_t *, uint32_t max_p, uint32_t max_t, void *) {
    last = Call{1, *al, {nullptr, 0}, n, max_p, max_t, *p, *t, scores, nullptr};
    n_calls++;
    return GASALX_OK;
}
int gasalx_nv_score_sinks_device(gasalx_engine *, const gasalx_nv_aligner *al, uint32_t n, const gasalx_nv_strings *p,
                                 const gasalx_nv_strings *t, int32_t *scores, uint32_t *sinks, uint32_t max_p,
                                 uint32_t max_t, void *) {
    last = Call{2, *al, {nullptr, 0}, n, max_p, max_t, *p, *t, scores, sinks};
    n_calls++;
    return GASALX_OK;
}
int gasalx_nv_matrix_score_device(gasalx_engine *eng, const gasalx_nv_aligner *al, const gasalx_nv_matrix *mat, uint32_t n,
                                  const gasalx_nv_strings *p, const gasalx_nv_strings *t, int32_t *scores,
                                  uint32_t *sinks, uint32_t max_p, uint32_t max_t, void *) {
    if (eng != kEngine) return GASALX_EINVAL;
    last = Call{3, *al, *mat, n, max_p, max_t, *p, *t, scores, sinks};
    n_calls++;
    return GASALX_OK;
}
uint64_t gasalx_nv_traceback_workspace(uint32_t, uint32_t, uint32_t) { return 0; }
int gasalx_nv_traceback_device(gasalx_engine *, const gasalx_nv_aligner *al, uint32_t n, const gasalx_nv_strings *p,
                               const gasalx_nv_strings *t, uint32_t max_p, uint32_t max_t, int32_t *scores,
                               uint32_t *sources, uint32_t *sinks, uint8_t *ops, uint32_t ops_stride, uint32_t *n_ops,
                               void *stream) {
    last = Call{4, *al, {nullptr, 0}, n, max_p, max_t, *p, *t, scores, sinks, sources, ops, n_ops, stream, ops_stride};
    n_calls++;
    return GASALX_OK;
}
int gasalx_nv_matrix_traceback_device(gasalx_engine *eng, const gasalx_nv_aligner *al, const gasalx_nv_matrix *mat,
                                      uint32_t n, const gasalx_nv_strings *p, const gasalx_nv_strings *t, uint32_t max_p,
                                      uint32_t max_t, int32_t *scores, uint32_t *sources, uint32_t *sinks, uint8_t *ops,
                                      uint32_t ops_stride, uint32_t *n_ops, void *stream) {
    if (eng != kEngine) return GASALX_EINVAL;
    last = Call{5, *al, *mat, n, max_p, max_t, *p, *t, scores, sinks, sources, ops, n_ops, stream, ops_stride};
    n_calls++;
    return GASALX_OK;
}
#if defined(CHECK_BANDED_OVER_MATRIX_REFUSED)
int gasalx_nv_banded_score_device(gasalx_engine *, const gasalx_nv_aligner *, uint32_t, uint32_t, const gasalx_nv_strings *,
                                  const gasalx_nv_strings *, int32_t *, uint32_t, void *) { return GASALX_OK; }
#endif
#if defined(CHECK_BANDED_TRACEBACK_OVER_MATRIX_REFUSED)
uint64_t gasalx_nv_banded_traceback_workspace(uint32_t, uint32_t, uint32_t) { return 0; }
int gasalx_nv_banded_traceback_device(gasalx_engine *, const gasalx_nv_aligner *, uint32_t, uint32_t,
                                      const gasalx_nv_strings *, const gasalx_nv_strings *, uint32_t, int32_t *, uint32_t *,
                                      uint32_t *, uint8_t *, uint32_t, uint32_t *, void *) { return GASALX_OK; }
#endif
}

#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

int main() {
    using namespace nvbio;
    using namespace nvbio::aln;
    static int8_t table[24 * 24];
    for (int i = 0; i < 24 * 24; ++i) table[i] = (int8_t)(i % 13 - 4);
    static uint8 pat_symbols[16], txt_symbols[64];
    static uint32 pat_offsets[3] = {0, 5, 9}, txt_offsets[3] = {0, 7, 20}, sinks[4];
    static int32 scores32[2];
    const SubstitutionMatrixScheme scheme(table, 24, -5, -3);

    // the scheme concept: substitution(r_i, q_j, r, q, qq) = table[r + q * n], r the text symbol
    EXPECT(scheme.substitution(0, 0, 3, 7) == table[3 + 7 * 24] && scheme.substitution(9, 9, 7, 3, 40) == table[7 + 3 * 24]);
    EXPECT(scheme.match() == 8 && scheme.pattern_gap_open() == -5 && scheme.text_gap_extension() == -3);
    static_assert(uses_matrix_scheme<GotohAligner<LOCAL, SubstitutionMatrixScheme, TextBlockingTag> >::value, "");
    static_assert(!uses_matrix_scheme<GotohAligner<LOCAL, SimpleGotohScheme> >::value, "");
    static_assert(!uses_matrix_scheme<EditDistanceAligner<LOCAL> >::value, "");

    auto check_matrix_call = [&](const void *want_sinks) {
        EXPECT(last.which == 3 && last.mat.scores == table && last.mat.n == 24);
        EXPECT(last.al.aligner == GASALX_NV_GOTOH && last.al.type == GASALX_NV_LOCAL && last.al.gap_open == -5 &&
               last.al.gap_ext == -3);
        EXPECT(last.n == 2 && last.max_p == 5 && last.max_t == 13 && last.scores == scores32 && last.sinks == want_sinks);
        EXPECT(last.p.words == (const uint32_t *)pat_symbols && last.p.offsets == pat_offsets && last.p.bits == 8 &&
               last.p.big_endian == 0);
        EXPECT(last.t.words == (const uint32_t *)txt_symbols && last.t.offsets == txt_offsets && last.t.bits == 8 &&
               last.t.big_endian == 0);
    };
    const ConcatenatedStringSet P = make_concatenated_string_set(2, pat_symbols, pat_offsets);
    const ConcatenatedStringSet T = make_concatenated_string_set(2, txt_symbols, txt_offsets);
    {   // the free function, TextBlockingTag: scores and sinks
        const BestSinks out = {scores32, sinks};
        batch_alignment_score(make_gotoh_aligner<LOCAL, TextBlockingTag>(scheme), P, T, out, DeviceThreadScheduler(), 5, 13);
        EXPECT(n_calls == 1);
        check_matrix_call(sinks);
    }
    {   // PatternBlockingTag: scores only
        const BestSinks out = {scores32, nullptr};
        batch_alignment_score(make_gotoh_aligner<LOCAL, PatternBlockingTag>(scheme), P, T, out,
                              DeviceThreadBlockScheduler<128, 1>(), 5, 13);
        EXPECT(n_calls == 2);
        check_matrix_call(nullptr);
    }
    {   // enact over a stream of the matrix aligner
        auto al = make_gotoh_aligner<LOCAL, TextBlockingTag>(scheme);
        typedef AlignmentStream<decltype(al)> stream_type;
        stream_type s(al, 2, pat_offsets, (const uint32 *)pat_symbols, 5, 9, (const uint32 *)txt_symbols, 13, nullptr);
        s.m_text_offsets = txt_offsets;
        s.m_pattern_bits = 8; s.m_pattern_big_endian = 0; s.m_text_bits = 8; s.m_text_big_endian = 0;
        s.m_scores32 = scores32;
        s.set_sinks(sinks);
        BatchedAlignmentScore<stream_type, DeviceThreadScheduler> batch;
        batch.enact(s);
        EXPECT(n_calls == 3);
        check_matrix_call(sinks);
    }
    {   // a Simple scheme through the free function: the calls BatchedAlignmentScore always made
        const SimpleGotohScheme simple(1, -1, -5, -3);
        const BestSinks both = {scores32, sinks}, only_scores = {scores32, nullptr};
        batch_alignment_score(make_gotoh_aligner<LOCAL, TextBlockingTag>(simple), P, T, both, DeviceThreadScheduler(), 5, 13);
        EXPECT(n_calls == 4 && last.which == 2 && last.al.match == 1 && last.al.mismatch == -1 && last.sinks == sinks &&
               last.p.bits == 8 && last.t.offsets == txt_offsets && last.max_t == 13);
        batch_alignment_score(make_gotoh_aligner<LOCAL, PatternBlockingTag>(simple), P, T, only_scores,
                              DeviceThreadScheduler(), 5, 13);
        EXPECT(n_calls == 5 && last.which == 1 && last.scores == scores32);
        // a packed set on one side
        static uint32 words[4];
        const PackedStringSet P4(2, words, pat_offsets, 4, 1);
        batch_alignment_score(make_edit_distance_aligner<SEMI_GLOBAL, TextBlockingTag>(), P4, T, both, DeviceThreadScheduler());
        EXPECT(n_calls == 6 && last.which == 2 && last.al.aligner == GASALX_NV_ED && last.p.words == words &&
               last.p.bits == 4 && last.p.big_endian == 1 && last.max_p == 1000 && last.max_t == 1000);
    }
#ifdef CHECK_SW_OVER_MATRIX_REFUSED
    { auto sw = make_smith_waterman_aligner<LOCAL>(scheme); (void)sw; }   // static_assert: a Gotoh scheme
#endif
#ifdef CHECK_BANDED_OVER_MATRIX_REFUSED
    {   // static_assert: no banded matrix kernels
        const BestSinks out = {scores32, nullptr};
        batch_banded_alignment_score<15>(make_gotoh_aligner<LOCAL, TextBlockingTag>(scheme), PackedStringSet(2, nullptr, pat_offsets, 8, 0),
                                         PackedStringSet(2, nullptr, txt_offsets, 8, 0), out, DeviceThreadScheduler(), 5, 13);
    }
#endif
    {   // the full-DP traceback: the matrix aligner reaches the matrix entry point, a Simple scheme its own
        static uint32 sources[4], n_ops[2];
        static uint8 ops[2 * 18];
        void *const hip_stream = reinterpret_cast<void *>(0x20);
        auto fill = [&](auto &s) {
            s.m_text_offsets = txt_offsets; s.m_max_text_len = 13;
            s.m_pattern_bits = 8; s.m_pattern_big_endian = 0; s.m_text_bits = 8; s.m_text_big_endian = 0;
        };
        auto check_outputs = [&] {
            EXPECT(last.n == 2 && last.max_p == 5 && last.max_t == 13 && last.scores == scores32 && last.sources == sources &&
                   last.sinks == sinks && last.ops == ops && last.ops_stride == 18 && last.n_ops == n_ops &&
                   last.stream == hip_stream);
            EXPECT(last.p.words == (const uint32_t *)pat_symbols && last.p.offsets == pat_offsets && last.p.bits == 8 &&
                   last.t.words == (const uint32_t *)txt_symbols && last.t.offsets == txt_offsets && last.t.bits == 8);
        };
        typedef GotohAligner<LOCAL, SubstitutionMatrixScheme> matrix_aligner;
        typedef TracebackStream<matrix_aligner> matrix_stream;
        matrix_stream ms(matrix_aligner(scheme), 2, pat_offsets, (const uint32 *)pat_symbols, 5, 9,
                         (const uint32 *)txt_symbols, 0, scores32, sources, sinks, ops, 18, n_ops);
        fill(ms);
        BatchedAlignmentTraceback<0, matrix_stream> mbatch;
        mbatch.enact(ms, 0u, NULL, hip_stream);
        EXPECT(n_calls == 7 && last.which == 5 && last.mat.scores == table && last.mat.n == 24);
        EXPECT(last.al.aligner == GASALX_NV_GOTOH && last.al.type == GASALX_NV_LOCAL && last.al.gap_open == -5 &&
               last.al.gap_ext == -3);
        check_outputs();
        typedef GotohAligner<LOCAL, SimpleGotohScheme> simple_aligner;
        typedef TracebackStream<simple_aligner> simple_stream;
        simple_stream ss(simple_aligner(SimpleGotohScheme(1, -1, -5, -3)), 2, pat_offsets, (const uint32 *)pat_symbols, 5, 9,
                         (const uint32 *)txt_symbols, 0, scores32, sources, sinks, ops, 18, n_ops);
        fill(ss);
        BatchedAlignmentTraceback<0, simple_stream> sbatch;
        sbatch.enact(ss, 0u, NULL, hip_stream);
        EXPECT(n_calls == 8 && last.which == 4 && last.al.match == 1 && last.al.mismatch == -1 && last.al.gap_open == -5 &&
               last.al.gap_ext == -3 && last.mat.scores == nullptr);
        check_outputs();
    }
#ifdef CHECK_BANDED_TRACEBACK_OVER_MATRIX_REFUSED
    {   // static_assert: no banded matrix traceback
        auto al = make_gotoh_aligner<LOCAL, TextBlockingTag>(scheme);
        typedef TracebackStream<decltype(al)> stream_type;
        stream_type s(al, 2, pat_offsets, nullptr, 5, 9, nullptr, 13, scores32, nullptr, nullptr, nullptr, 18, nullptr);
        BatchedBandedAlignmentTraceback<15, 0, stream_type> batch;
        batch.enact(s);
    }
#endif
    if (failures) { fprintf(stderr, "nvbio_matrix_header_check: %d failure(s)\n", failures); return 1; }
    printf("nvbio_matrix_header_check ok\n");
    return 0;
}
