/*
 * nvbio_batched.h — nvbio-shaped batched alignment scoring over libgasal (second
 * front-end).
 *
 * Replaces, for the scoring path sw-benchmark drives:
 *   nvbio::aln::BatchedAlignmentScore<stream, scheduler>   NvB/nvbio/alignment/batched.h:313-352
 *   the scheduler tags                                      batched.h:44-87
 *   SimpleSmithWatermanScheme / SimpleGotohScheme           alignment/utils.h:92-135
 *   make_{edit_distance,smith_waterman,gotoh}_aligner       alignment/alignment_base.h:180-330
 *   nvbio::aln::BatchedBandedAlignmentScore<BAND_LEN, stream, scheduler>
 *                                                           batched.h:337-352, batched_banded_inl.h:44-75
 *   nvbio::aln::BatchedAlignmentTraceback<CHECKPOINTS, stream, scheduler>
 *                                                           batched.h:436-449, batched_inl.h:612-664
 *   nvbio::aln::BatchedBandedAlignmentTraceback<BAND_LEN, CHECKPOINTS, stream, scheduler>
 *                                                           batched.h:464-478, batched_banded_inl.h:248-297
 *   sw-benchmark's AlignmentStream (reads 4-bit DNA_N big-endian, reference 2-bit,
 *   int16 scores)                                           NvB/sw-benchmark/sw-benchmark.cu:100-215
 * Every scheduler maps to the same MI355X kernel (nvbio.hpp: lane groups per pattern,
 * text in LDS; banded: nvbanded.hpp, one pair per thread with the band in registers);
 * the scoring classes take no temporary storage, so their max_temp_storage() is 0.  The
 * traceback classes report the engine's own workspace there (gasalx_nv_*traceback_workspace:
 * the flags of every cell, in chunks of at most 4 GiB); enact() does not use the caller's
 * temp buffer.  The TextBlockingTag /
 * PatternBlockingTag score semantics are provided (both give the same scores), full and
 * banded.  The banded scorer (BatchedBandedAlignmentScore, batch_banded_alignment_score) reports
 * the BestSink position beside the score for the ED, SW and Gotoh aligners when the stream carries a
 * sinks array (nvbanded_sink.hpp: the banded score pass has one report order, so either blocking
 * tag is taken), what nvBowtie places its banded traceback by.  The full-DP scorer also reports where the best score ends: AlignmentStream::set_sinks
 * asks for nvbio's BestSink position (x = text, y = pattern) of every pair, exact to the
 * TextBlockingTag report order on ties (nvbio_sink.hpp); PatternBlockingTag aligners, whose
 * tied sinks differ, are refused at compile time.  Traceback: BatchedAlignmentTraceback<CHECKPOINTS, stream_type> (full DP) and
 * BatchedBandedAlignmentTraceback<BAND_LEN, CHECKPOINTS, stream_type> for the edit-distance,
 * Smith-Waterman and Gotoh aligners over a TracebackStream (nvtrace.hpp: one pair per thread,
 * as the reference's DeviceThreadScheduler runs it); the warp variants are not provided.
 * EditDistanceAligner<TYPE, MyersTag<N>> (nvbio's Myers bit-vector edit distance,
 * myers/myers_banded_inl.h) runs under BatchedBandedAlignmentScore and the free function
 * batch_banded_alignment_score<BAND_LEN>, qmap's and fmmap's call, with scores and BestSink
 * positions (nvmyers.hpp); the full-DP scorer and the tracebacks refuse it at compile time.
 * Substitution matrices: a GotohAligner over SubstitutionMatrixScheme (a host table of n x n signed
 * bytes, n <= 32, read as table[r + q*n] with r the text and q the pattern symbol: the proteinsw
 * example's BlosumScheme, examples/proteinsw/proteinsw.cu:76-100, with the table made a member) is
 * routed by BatchedAlignmentScore::enact to gasalx_nv_matrix_score_* (nvmatrix.hpp: int32 scores,
 * BestSink positions for TextBlockingTag aligners; symbols >= n read as n - 1), and by
 * BatchedAlignmentTraceback::enact to gasalx_nv_matrix_traceback_* (nvmatrix_trace.hpp: the full-DP
 * traceback with the same outputs and workspace as the Simple schemes').  No table is
 * shipped: the caller supplies BLOSUM62 or whatever it scores with.  Smith-Waterman never reads a
 * substitution score from its scheme, and the banded scorer and the banded traceback have no matrix
 * kernels: all three refuse the scheme at compile time.  ConcatenatedStringSet /
 * make_concatenated_string_set (8-bit symbols) and the free function batch_alignment_score
 * (batched.h:137-150), proteinsw's call, take any aligner the full scorer takes.
 * Base qualities: a GotohAligner over QualityGotohScheme (two host tables match[l] / mismatch[l] over
 * quality levels, nvBowtie's SmithWatermanScoringScheme<QualCost, ConstantCost> as its Gotoh aligners
 * read it, nvBowtie/bowtie2/cuda/scoring.h:286-291; the tables are built on the host by QualCost,
 * ConstantCost and RoundedQualCost with the reference's arithmetic) is routed by
 * BatchedBandedAlignmentScore::enact, batch_banded_alignment_score and
 * BatchedBandedAlignmentTraceback::enact to gasalx_nv_banded_qual_score_* and
 * gasalx_nv_banded_qual_traceback_* (nvbanded_qual.hpp), with the qualities the stream carries
 * (AlignmentStream::set_quals: one byte per pattern symbol at the patterns' offsets; a stream without
 * them is an error at enact).  What nvBowtie calls at score_best_inl.h:179-197, score_all_inl.h:199-217,
 * score_paired_inl.h:217-235 and traceback_inl.h:239-257, :495-513.  The full-DP BatchedAlignmentScore,
 * batch_alignment_score and BatchedAlignmentTraceback have no quality kernels and refuse the scheme at
 * compile time (nvBowtie's score_opposite_inl.h:266 and traceback_inl.h:292 call sites are not covered),
 * as does SmithWatermanAligner, which nothing in the tree drives with qualities.
 *
 * Header-only C++ over the flat C-ABI (gasalx.h); link with -lgasal.
 */
#ifndef NVBIO_BATCHED_H
#define NVBIO_BATCHED_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>
#include <utility>

#include "gasalx.h"

namespace nvbio {

typedef uint8_t uint8;
typedef int16_t int16;
typedef int32_t int32;
typedef uint32_t uint32;
typedef uint64_t uint64;

// A set of 8-bit strings stored back to back (strings/string_set.h ConcatenatedStringSet over a
// uint8 iterator, as proteinsw builds it): string k is symbols[offsets[k] .. offsets[k + 1]).  Both
// are device pointers; symbols must be 4-byte aligned (the kernels read whole words, symbol s in
// bits 8 * (s % 4) of word s / 4).
struct ConcatenatedStringSet {
    ConcatenatedStringSet(const uint32 count, const uint8 *symbols, const uint32 *offsets)
        : m_count(count), m_symbols(symbols), m_offsets(offsets) {}
    uint32 size() const { return m_count; }
    uint32 m_count;
    const uint8 *m_symbols;
    const uint32 *m_offsets;
};
inline ConcatenatedStringSet make_concatenated_string_set(const uint32 count, const uint8 *symbols,
                                                          const uint32 *offsets) {
    return ConcatenatedStringSet(count, symbols, offsets);
}

namespace aln {

enum AlignmentType { GLOBAL, LOCAL, SEMI_GLOBAL };   // alignment_base.h:54

struct PatternBlockingTag {};
struct TextBlockingTag {};
// the Myers bit-vector algorithm over an alphabet of N symbols (alignment_base.h:64-65): edit
// distance only, banded scoring only (myers/myers_banded_inl.h is the one function this tree has)
template <uint32 N>
struct MyersTag { static const uint32 ALPHABET_SIZE = N; };
template <typename T> struct is_myers_tag : std::false_type {};
template <uint32 N> struct is_myers_tag<MyersTag<N> > : std::true_type {};

// batch schedulers (batched.h:44-87): tags only; all run the same device kernel
struct HostThreadScheduler {};
template <uint32 BLOCKDIM_T, uint32 MINBLOCKS_T>
struct DeviceThreadBlockScheduler {
    static const uint32 BLOCKDIM = BLOCKDIM_T;
    static const uint32 MINBLOCKS = MINBLOCKS_T;
};
typedef DeviceThreadBlockScheduler<128, 1> DeviceThreadScheduler;
struct DeviceStagedThreadScheduler {};
struct DeviceWarpScheduler {};

struct SimpleSmithWatermanScheme {   // utils.h:92-110
    SimpleSmithWatermanScheme() {}
    SimpleSmithWatermanScheme(int32 match, int32 mm, int32 del, int32 ins)
        : m_match(match), m_mismatch(mm), m_deletion(del), m_insertion(ins) {}
    int32 match(uint8 = 0) const { return m_match; }
    int32 mismatch(uint8 = 0) const { return m_mismatch; }
    int32 deletion() const { return m_deletion; }
    int32 insertion() const { return m_insertion; }
    int32 m_match = 0, m_mismatch = 0, m_deletion = 0, m_insertion = 0;
};

struct SimpleGotohScheme {   // utils.h:114-135
    SimpleGotohScheme() {}
    SimpleGotohScheme(int32 match, int32 mm, int32 gap_open, int32 gap_ext)
        : m_match(match), m_mismatch(mm), m_gap_open(gap_open), m_gap_ext(gap_ext) {}
    int32 match(uint8 = 0) const { return m_match; }
    int32 mismatch(uint8 = 0) const { return m_mismatch; }
    int32 pattern_gap_open() const { return m_gap_open; }
    int32 pattern_gap_extension() const { return m_gap_ext; }
    int32 text_gap_open() const { return m_gap_open; }
    int32 text_gap_extension() const { return m_gap_ext; }
    int32 m_match = 0, m_mismatch = 0, m_gap_open = 0, m_gap_ext = 0;
};

// A Gotoh scheme whose substitution score comes from a table: nvbio's scheme concept as
// GotohAligner reads it (gotoh_inl.h:534, :1042 call substitution(r_i, q_j, r, q, qq)), the
// proteinsw example's BlosumScheme with the table's size a member.  table: a HOST array of n * n
// signed bytes, n in 2..32, table[r + q*n] the score of text (reference) symbol r against pattern
// (query) symbol q; it is read at every enact() and must live until that call returns.
struct SubstitutionMatrixScheme {
    SubstitutionMatrixScheme() {}
    SubstitutionMatrixScheme(const int8_t *table, uint32 n, int32 gap_open, int32 gap_ext)
        : m_table(table), m_n(n), m_gap_open(gap_open), m_gap_ext(gap_ext) {}
    // the maximum match bonus: the table's largest entry
    int32 match(uint8 = 0) const {
        int32 best = m_table[0];
        for (uint32 i = 1; i < m_n * m_n; ++i) best = m_table[i] > best ? m_table[i] : best;
        return best;
    }
    int32 substitution(uint32 /*r_i*/, uint32 /*q_j*/, uint8 r, uint8 q, uint8 /*qq*/ = 0) const {
        return m_table[r + q * m_n];
    }
    int32 pattern_gap_open() const { return m_gap_open; }
    int32 pattern_gap_extension() const { return m_gap_ext; }
    int32 text_gap_open() const { return m_gap_open; }
    int32 text_gap_extension() const { return m_gap_ext; }
    gasalx_nv_matrix c_matrix() const {
        gasalx_nv_matrix m = {m_table, m_n};
        return m;
    }
    const int8_t *m_table = nullptr;
    uint32 m_n = 0;
    int32 m_gap_open = 0, m_gap_ext = 0;
};
template <typename T> struct is_matrix_scheme : std::false_type {};
template <> struct is_matrix_scheme<SubstitutionMatrixScheme> : std::true_type {};
// an aligner whose scheme is a SubstitutionMatrixScheme (EditDistanceAligner has no scheme)
template <typename A, typename = void> struct uses_matrix_scheme : std::false_type {};
template <typename A>
struct uses_matrix_scheme<A, std::void_t<decltype(std::declval<const A &>().scheme)> >
    : is_matrix_scheme<typename std::decay<decltype(std::declval<const A &>().scheme)>::type> {};

// The three cost functions nvBowtie builds its schemes from, evaluated on the host (float arithmetic
// included, so no rounding question reaches the device): cost(q) at quality q.
struct QualCost {        // scoring.h:86-105: min + int(min(q, 40) / 40.0f * (max - min))
    QualCost(int32 min_val, int32 max_val) : m_min_val(min_val), m_max_val(max_val) {}
    int32 operator()(const int q) const {
        const float frac = (float)((q < 40 ? q : 40) / 40.0f);
        return m_min_val + int32(frac * (m_max_val - m_min_val));
    }
    int32 m_min_val, m_max_val;
};
struct ConstantCost {    // scoring.h:111-125
    explicit ConstantCost(int32 v) : m_val(v) {}
    int32 operator()(const int) const { return m_val; }
    int32 m_val;
};
struct RoundedQualCost { // scoring.h:68-80: phred_to_maq(q), quality_coeffs.h:44-54
    int32 operator()(const int q) const { return q < 5 ? 0 : q < 15 ? 10 : q < 25 ? 20 : 30; }
};

// A Gotoh scheme whose substitution score depends on the base quality of the pattern symbol, as
// nvBowtie's SmithWatermanScoringScheme answers its Gotoh aligners (scoring.h:286-291): two host
// tables over `levels` quality levels (1..256; a quality >= levels reads the last entry), signed
// scores, and the pattern gap scores.  Built from a match cost and a mismatch penalty function:
// match[l] = match_cost(l), mismatch[l] = -mismatch_penalty(l).
struct QualityGotohScheme {
    static const uint32 MAX_LEVELS = 256;
    QualityGotohScheme() {}
    template <typename MatchCost, typename MismatchCost>
    QualityGotohScheme(const MatchCost &match_cost, const MismatchCost &mismatch_penalty, int32 gap_open, int32 gap_ext,
                       uint32 levels = MAX_LEVELS)
        : m_levels(levels < 1 ? 1 : levels > MAX_LEVELS ? MAX_LEVELS : levels), m_gap_open(gap_open), m_gap_ext(gap_ext) {
        for (uint32 l = 0; l < m_levels; ++l) {
            m_match[l] = (int16)match_cost((int)l);
            m_mismatch[l] = (int16)-mismatch_penalty((int)l);
        }
    }
    // nvBowtie's default scheme (scoring_inl.h:108-122): match 0, mismatch penalty QualCost(2, 6)
    // (bowtie2's --mp 6,2), read gaps 5 + 3 to open and 3 to extend, i.e. -(const + coeff) and -coeff
    static QualityGotohScheme nvbowtie_default() {
        return QualityGotohScheme(ConstantCost(0), QualCost(2, 6), -(5 + 3), -3);
    }
    uint32 level(uint8 q) const { return q < m_levels ? q : m_levels - 1; }
    int32 match(uint8 q = 0) const { return m_match[level(q)]; }
    int32 mismatch(uint8 q = 0) const { return m_mismatch[level(q)]; }
    int32 substitution(uint32 /*r_i*/, uint32 /*q_j*/, uint8 r, uint8 q, uint8 qq = 0) const {
        return r == q ? match(qq) : mismatch(qq);
    }
    int32 pattern_gap_open() const { return m_gap_open; }
    int32 pattern_gap_extension() const { return m_gap_ext; }
    int32 text_gap_open() const { return m_gap_open; }
    int32 text_gap_extension() const { return m_gap_ext; }
    // the tables with a batch's qualities (a device array for the device entry points); the struct
    // points into this scheme, which must live until the call returns
    gasalx_nv_quals c_quals(const uint8 *quals = NULL) const {
        gasalx_nv_quals q = {quals, m_match, m_mismatch, m_levels};
        return q;
    }
    int16 m_match[MAX_LEVELS] = {}, m_mismatch[MAX_LEVELS] = {};
    uint32 m_levels = 1;
    int32 m_gap_open = 0, m_gap_ext = 0;
};
template <typename T> struct is_quality_scheme : std::false_type {};
template <> struct is_quality_scheme<QualityGotohScheme> : std::true_type {};
template <typename A, typename = void> struct uses_quality_scheme : std::false_type {};
template <typename A>
struct uses_quality_scheme<A, std::void_t<decltype(std::declval<const A &>().scheme)> >
    : is_quality_scheme<typename std::decay<decltype(std::declval<const A &>().scheme)>::type> {};

template <AlignmentType T_TYPE, typename AlgorithmType = PatternBlockingTag>
struct EditDistanceAligner {
    static const AlignmentType TYPE = T_TYPE;
    typedef AlgorithmType algorithm_tag;
    gasalx_nv_aligner c_aligner() const {
        gasalx_nv_aligner a = {GASALX_NV_ED, (int32)TYPE, 0, -1, 0, 0, -1, -1};
        return a;
    }
};

template <AlignmentType T_TYPE, typename scoring_scheme_type, typename AlgorithmType = PatternBlockingTag>
struct SmithWatermanAligner {
    static_assert(!is_matrix_scheme<scoring_scheme_type>::value,
                  "SubstitutionMatrixScheme is a Gotoh scheme: nvbio's Smith-Waterman (sw/sw_inl.h) reads match() and "
                  "mismatch() only and never calls substitution(); use make_gotoh_aligner");
    static_assert(!is_quality_scheme<scoring_scheme_type>::value,
                  "QualityGotohScheme is a Gotoh scheme: nothing in the tree drives Smith-Waterman with qualities, "
                  "and only the banded Gotoh kernels are built for it; use make_gotoh_aligner");
    static const AlignmentType TYPE = T_TYPE;
    typedef AlgorithmType algorithm_tag;
    SmithWatermanAligner() {}
    explicit SmithWatermanAligner(const scoring_scheme_type s) : scheme(s) {}
    gasalx_nv_aligner c_aligner() const {
        gasalx_nv_aligner a = {GASALX_NV_SW, (int32)TYPE, scheme.match(), scheme.mismatch(), 0, 0,
                               scheme.deletion(), scheme.insertion()};
        return a;
    }
    scoring_scheme_type scheme;
};

template <AlignmentType T_TYPE, typename scoring_scheme_type, typename AlgorithmType = PatternBlockingTag>
struct GotohAligner {
    static const AlignmentType TYPE = T_TYPE;
    typedef AlgorithmType algorithm_tag;
    GotohAligner() {}
    explicit GotohAligner(const scoring_scheme_type s) : scheme(s) {}
    gasalx_nv_aligner c_aligner() const {
        if constexpr (is_matrix_scheme<scoring_scheme_type>::value || is_quality_scheme<scoring_scheme_type>::value) {
            // match / mismatch are not read by the matrix and the quality entry points
            gasalx_nv_aligner a = {GASALX_NV_GOTOH, (int32)TYPE, 0, 0, scheme.pattern_gap_open(),
                                   scheme.pattern_gap_extension(), 0, 0};
            return a;
        } else {
            gasalx_nv_aligner a = {GASALX_NV_GOTOH, (int32)TYPE, scheme.match(), scheme.mismatch(),
                                   scheme.pattern_gap_open(), scheme.pattern_gap_extension(), 0, 0};
            return a;
        }
    }
    scoring_scheme_type scheme;
};

template <AlignmentType TYPE>
EditDistanceAligner<TYPE> make_edit_distance_aligner() { return EditDistanceAligner<TYPE>(); }
template <AlignmentType TYPE, typename algorithm_tag>
EditDistanceAligner<TYPE, algorithm_tag> make_edit_distance_aligner() { return EditDistanceAligner<TYPE, algorithm_tag>(); }
template <AlignmentType TYPE, typename scheme_type>
SmithWatermanAligner<TYPE, scheme_type> make_smith_waterman_aligner(const scheme_type &s) {
    return SmithWatermanAligner<TYPE, scheme_type>(s);
}
template <AlignmentType TYPE, typename algorithm_tag, typename scheme_type>
SmithWatermanAligner<TYPE, scheme_type, algorithm_tag> make_smith_waterman_aligner(const scheme_type &s) {
    return SmithWatermanAligner<TYPE, scheme_type, algorithm_tag>(s);
}
template <AlignmentType TYPE, typename scheme_type>
GotohAligner<TYPE, scheme_type> make_gotoh_aligner(const scheme_type &s) { return GotohAligner<TYPE, scheme_type>(s); }
template <AlignmentType TYPE, typename algorithm_tag, typename scheme_type>
GotohAligner<TYPE, scheme_type, algorithm_tag> make_gotoh_aligner(const scheme_type &s) {
    return GotohAligner<TYPE, scheme_type, algorithm_tag>(s);
}

// The device string sets and score sink of one batch: sw-benchmark's AlignmentStream
// (sw-benchmark.cu:100-215) with its packing made explicit.  All pointers are device
// pointers.  Patterns: n_tasks + 1 symbol offsets; text: one string shared by every
// pattern (text_offsets NULL) or n_tasks + 1 offsets.
template <typename aligner_type_T>
struct AlignmentStream {
    typedef aligner_type_T aligner_type;
    AlignmentStream(const aligner_type aligner, const uint32 count, const uint32 *offsets, const uint32 *patterns,
                    const uint32 max_pattern_len, const uint32 total_pattern_len, const uint32 *text,
                    const uint32 text_len, int16 *scores)
        : m_aligner(aligner), m_count(count), m_max_pattern_len(max_pattern_len),
          m_total_pattern_len(total_pattern_len), m_text_len(text_len), m_offsets(offsets), m_patterns(patterns),
          m_text(text), m_scores(scores) {}

    const aligner_type &aligner() const { return m_aligner; }
    uint32 max_pattern_length() const { return m_max_pattern_len; }
    uint32 max_text_length() const { return m_text_len; }
    uint32 size() const { return m_count; }
    uint64 cells() const { return uint64(m_total_pattern_len) * uint64(m_text_len); }

    // Ask for the BestSink position of every pair beside its score (what nvbio's
    // alignment_score(aligner, pattern, text, min_score, sink) leaves in the sink): a device
    // array of 2 x count entries, sinks[2k] = x (text), sinks[2k + 1] = y (pattern), one-based.
    // On ties BestSink keeps the last maximum in the aligner's report order, and the kernels
    // follow the TextBlockingTag order (text stripes of the aligner's BAND_LEN columns: 8 for Gotoh, 16 for Smith-Waterman and edit distance).
    void set_sinks(uint32 *sinks) {
        static_assert(std::is_same<typename aligner_type::algorithm_tag, TextBlockingTag>::value ||
                          is_myers_tag<typename aligner_type::algorithm_tag>::value,
                      "sinks are provided for TextBlockingTag aligners only: PatternBlockingTag reports cells in "
                      "another order (pattern stripes), so its tied sinks differ; make the aligner with "
                      "make_*_aligner<TYPE, TextBlockingTag>(...) or score without sinks");
        m_sinks = sinks;
    }
    // The base qualities of the patterns, for an aligner over QualityGotohScheme: a device array of
    // one byte per pattern symbol at the patterns' own offsets (quals[offsets[k] + i] is symbol i of
    // pattern k), what nvbio's banded_alignment_score(aligner, pattern, quals, text, ...) takes.
    void set_quals(const uint8 *quals) { m_quals = quals; }

    aligner_type m_aligner;
    uint32 m_count, m_max_pattern_len, m_total_pattern_len, m_text_len;
    const uint32 *m_offsets, *m_patterns, *m_text;
    int16 *m_scores;
    int32 *m_scores32 = nullptr;            // optional int32 scores
    uint32 *m_sinks = nullptr;              // optional BestSink positions, 2 x count: set_sinks()
    const uint8 *m_quals = nullptr;         // base qualities, one per pattern symbol: set_quals()
    const uint32 *m_text_offsets = nullptr; // per-pattern texts instead of the shared one
    uint32 m_pattern_bits = 4, m_pattern_big_endian = 1;   // io::SequenceDataTraits<DNA_N>
    uint32 m_text_bits = 2, m_text_big_endian = 0;         // REF_BITS / REF_BIG_ENDIAN
};

// One engine per thread for the current device (set_device, default 0).
inline int &current_device() {
    static thread_local int d = 0;
    return d;
}
inline void set_device(int d) { current_device() = d; }
inline gasalx_engine *engine() {
    static thread_local gasalx_engine *eng[64] = {};
    const int d = current_device();
    if (d < 0 || d >= 64) { fprintf(stderr, "nvbio_batched: bad device %d\n", d); exit(EXIT_FAILURE); }
    if (!eng[d] && gasalx_engine_create(d, &eng[d]) != GASALX_OK) {
        fprintf(stderr, "nvbio_batched: %s\n", gasalx_last_error());
        exit(EXIT_FAILURE);
    }
    return eng[d];
}

template <typename stream_type, typename scheduler_type>
struct BatchedAlignmentScore {
    typedef stream_type input_stream_type;
    typedef typename stream_type::aligner_type aligner_type;

    // no temporary storage: the DP state stays in registers and LDS
    static uint64 max_temp_storage(const uint32, const uint32, const uint32) { return 0; }

    // enact the batch on the engine's stream (nvbio's enact is asynchronous too; the
    // benchmark synchronises the device afterwards).  Errors exit, as nvbio's do.
    void enact(stream_type stream, uint64 temp_size = 0u, uint8 *temp = NULL, void *hip_stream = NULL) {
        static_assert(!is_myers_tag<typename aligner_type::algorithm_tag>::value,
                      "MyersTag aligners run under BatchedBandedAlignmentScore only: nvbio has the banded Myers "
                      "scorer (myers/myers_banded_inl.h) and no full-DP or traceback form of it");
        static_assert(!uses_quality_scheme<aligner_type>::value,
                      "QualityGotohScheme runs under BatchedBandedAlignmentScore / batch_banded_alignment_score and "
                      "BatchedBandedAlignmentTraceback only: the full-DP scorer and traceback have no quality kernels");
        (void)temp_size; (void)temp;
        const gasalx_nv_aligner a = stream.aligner().c_aligner();
        gasalx_nv_strings p = {stream.m_patterns, stream.m_offsets, 0, stream.m_pattern_bits,
                               stream.m_pattern_big_endian};
        gasalx_nv_strings t = {stream.m_text, stream.m_text_offsets, stream.m_text_len, stream.m_text_bits,
                               stream.m_text_big_endian};
        int rc;
        if (stream.m_sinks) {
            // set_sinks() refuses PatternBlockingTag at compile time; a pointer stored around it
            // must not get TextBlockingTag sinks silently
            if (!std::is_same<typename aligner_type::algorithm_tag, TextBlockingTag>::value) {
                fprintf(stderr, "BatchedAlignmentScore::enact: sinks need a TextBlockingTag aligner\n");
                exit(EXIT_FAILURE);
            }
            if (stream.m_scores) {
                fprintf(stderr, "BatchedAlignmentScore::enact: with sinks the scores are int32, set m_scores32\n");
                exit(EXIT_FAILURE);
            }
        }
        if constexpr (uses_matrix_scheme<aligner_type>::value) {
            // GotohAligner over SubstitutionMatrixScheme: the matrix kernels (int32 scores, sinks optional)
            if (stream.m_scores) {
                fprintf(stderr, "BatchedAlignmentScore::enact: matrix scores are int32, set m_scores32\n");
                exit(EXIT_FAILURE);
            }
            const gasalx_nv_matrix m = stream.aligner().scheme.c_matrix();
            rc = gasalx_nv_matrix_score_device(engine(), &a, &m, stream.size(), &p, &t, stream.m_scores32,
                                               stream.m_sinks, stream.max_pattern_length(),
                                               stream.max_text_length(), hip_stream);
        } else if (stream.m_sinks) {
            rc = gasalx_nv_score_sinks_device(engine(), &a, stream.size(), &p, &t, stream.m_scores32, stream.m_sinks,
                                              stream.max_pattern_length(), stream.max_text_length(), hip_stream);
        } else {
            rc = gasalx_nv_score_device(engine(), &a, stream.size(), &p, &t, stream.m_scores32,
                                        stream.m_scores, stream.max_pattern_length(),
                                        stream.max_text_length(), hip_stream);
        }
        if (rc != GASALX_OK) {
            fprintf(stderr, "BatchedAlignmentScore::enact: %s\n", gasalx_last_error());
            exit(EXIT_FAILURE);
        }
    }
};

// Banded scoring (batched_banded_inl.h:44-75): every pattern against the first
// pattern_length + BAND_LEN - 1 symbols of its text, cells (i, i + j) with j < BAND_LEN
// (2..32).  Scores are int32 (stream.m_scores32); a text shorter than its pattern is
// skipped and scores INT32_MIN, as nvbio's BestSink leaves it.
template <uint32 BAND_LEN, typename stream_type, typename scheduler_type = DeviceThreadScheduler>
struct BatchedBandedAlignmentScore {
    typedef stream_type input_stream_type;
    typedef typename stream_type::aligner_type aligner_type;

    static uint64 min_temp_storage(const uint32, const uint32, const uint32) { return 0; }
    static uint64 max_temp_storage(const uint32, const uint32, const uint32) { return 0; }

    void enact(stream_type stream, uint64 temp_size = 0u, uint8 *temp = NULL, void *hip_stream = NULL) {
        static_assert(!uses_matrix_scheme<aligner_type>::value,
                      "SubstitutionMatrixScheme runs under BatchedAlignmentScore / batch_alignment_score and "
                      "BatchedAlignmentTraceback only: the banded scorer and the banded traceback have no matrix kernels");
        (void)temp_size; (void)temp;
        const gasalx_nv_aligner a = stream.aligner().c_aligner();
        gasalx_nv_strings p = {stream.m_patterns, stream.m_offsets, 0, stream.m_pattern_bits,
                               stream.m_pattern_big_endian};
        gasalx_nv_strings t = {stream.m_text, stream.m_text_offsets, stream.m_text_len, stream.m_text_bits,
                               stream.m_text_big_endian};
        if constexpr (is_myers_tag<typename aligner_type::algorithm_tag>::value) {
            // EditDistanceAligner<TYPE, MyersTag<N>>: nvbio's banded_myers, with the BestSink
            // positions when the stream carries them (scores or sinks, not neither)
            const int rc = gasalx_nv_banded_myers_device(engine(), a.type, aligner_type::algorithm_tag::ALPHABET_SIZE,
                                                         BAND_LEN, stream.size(), &p, &t, stream.m_scores32,
                                                         stream.m_sinks, stream.max_pattern_length(), hip_stream);
            if (rc != GASALX_OK) {
                fprintf(stderr, "BatchedBandedAlignmentScore::enact: %s\n", gasalx_last_error());
                exit(EXIT_FAILURE);
            }
            return;
        }
        int rc;
        if constexpr (uses_quality_scheme<aligner_type>::value) {
            // GotohAligner over QualityGotohScheme: scores and / or sinks, the stream's qualities
            if (stream.m_quals == NULL) {
                fprintf(stderr, "BatchedBandedAlignmentScore::enact: a QualityGotohScheme aligner needs the patterns' "
                                "qualities, call set_quals() on the stream\n");
                exit(EXIT_FAILURE);
            }
            const gasalx_nv_quals q = stream.aligner().scheme.c_quals(stream.m_quals);
            rc = gasalx_nv_banded_qual_score_device(engine(), &a, &q, BAND_LEN, stream.size(), &p, &t, stream.m_scores32,
                                                    stream.m_sinks, stream.max_pattern_length(), hip_stream);
        } else if (stream.m_sinks) {
            // ED, SW and Gotoh with the BestSink positions (scores optional)
            rc = gasalx_nv_banded_score_sinks_device(engine(), &a, BAND_LEN, stream.size(), &p, &t, stream.m_scores32,
                                                     stream.m_sinks, stream.max_pattern_length(), hip_stream);
        } else {
            if (stream.m_scores32 == NULL) {
                fprintf(stderr, "BatchedBandedAlignmentScore::enact: banded scores are int32, set m_scores32\n");
                exit(EXIT_FAILURE);
            }
            rc = gasalx_nv_banded_score_device(engine(), &a, BAND_LEN, stream.size(), &p, &t, stream.m_scores32,
                                               stream.max_pattern_length(), hip_stream);
        }
        if (rc != GASALX_OK) {
            fprintf(stderr, "BatchedBandedAlignmentScore::enact: %s\n", gasalx_last_error());
            exit(EXIT_FAILURE);
        }
    }
};

// A packed string set and the sinks of a batch as the free function below takes them: what qmap
// passes as read_infix_set / genome_infix_set and sinks.begin() (examples/qmap/qmap.cu:285-293),
// with the packing made explicit.  All pointers are device pointers; offsets: count + 1 symbol
// offsets into words.  BestSinks is a vector of BestSink<int32> as two arrays: scores[k], and
// sinks[2k] = x (text), sinks[2k + 1] = y (pattern); either may be NULL.
struct PackedStringSet {
    PackedStringSet(const uint32 count, const uint32 *words, const uint32 *offsets, const uint32 bits,
                    const uint32 big_endian)
        : m_count(count), m_words(words), m_offsets(offsets), m_bits(bits), m_big_endian(big_endian) {}
    uint32 size() const { return m_count; }
    uint32 m_count;
    const uint32 *m_words, *m_offsets;
    uint32 m_bits, m_big_endian;
};
struct BestSinks {
    int32 *scores;
    uint32 *sinks;
};

// batch_banded_alignment_score<BAND_LEN>(aligner, patterns, texts, sinks, scheduler, max_pattern_length,
// max_text_length) (batched.h:216-231), the form qmap and fmmap call: patterns[k] against texts[k]
// on the engine's stream (asynchronous, as nvbio's).  Every aligner takes scores and sinks: a
// MyersTag aligner through gasalx_nv_banded_myers_*, the ED, SW and Gotoh aligners through
// gasalx_nv_banded_score_sinks_* (gasalx_nv_banded_score_* when no sinks array is given), a Gotoh
// aligner over QualityGotohScheme through gasalx_nv_banded_qual_score_* with `quals` (a device array,
// one byte per pattern symbol at the patterns' offsets; needed by that scheme alone).
template <uint32 BAND_LEN, typename aligner_type, typename scheduler_type>
void batch_banded_alignment_score(const aligner_type aligner, const PackedStringSet patterns,
                                  const PackedStringSet texts, BestSinks sinks, const scheduler_type,
                                  const uint32 max_pattern_length, const uint32 max_text_length,
                                  const uint8 *quals = NULL) {
    (void)max_text_length;
    AlignmentStream<aligner_type> stream(aligner, patterns.size(), patterns.m_offsets, patterns.m_words,
                                         max_pattern_length, 0, texts.m_words, 0, NULL);
    stream.m_text_offsets = texts.m_offsets;
    stream.m_pattern_bits = patterns.m_bits; stream.m_pattern_big_endian = patterns.m_big_endian;
    stream.m_text_bits = texts.m_bits; stream.m_text_big_endian = texts.m_big_endian;
    stream.m_scores32 = sinks.scores;
    stream.m_sinks = sinks.sinks;
    stream.m_quals = quals;
    BatchedBandedAlignmentScore<BAND_LEN, AlignmentStream<aligner_type>, scheduler_type> batch;
    batch.enact(stream);
}

// batch_alignment_score(aligner, patterns, texts, sinks, scheduler, max_pattern_length, max_text_length)
// (batched.h:137-150), the form proteinsw calls: patterns[k] against texts[k], full DP, on the engine's
// stream (asynchronous, as nvbio's).  Every aligner BatchedAlignmentScore takes, the Simple schemes and
// SubstitutionMatrixScheme, over PackedStringSet or ConcatenatedStringSet.  Scores are int32.
// TextBlockingTag aligners fill sinks.scores and sinks.sinks (either may be NULL); PatternBlockingTag
// aligners give scores only, and a non-NULL sinks.sinks with one is refused as enact() refuses it.
inline PackedStringSet as_packed_string_set(const PackedStringSet &s) { return s; }
inline PackedStringSet as_packed_string_set(const ConcatenatedStringSet &s) {
    return PackedStringSet(s.m_count, reinterpret_cast<const uint32 *>(s.m_symbols), s.m_offsets, 8, 0);
}
template <typename aligner_type, typename pattern_set_type, typename text_set_type, typename scheduler_type>
void batch_alignment_score(const aligner_type aligner, const pattern_set_type patterns, const text_set_type texts,
                           BestSinks sinks, const scheduler_type, const uint32 max_pattern_length = 1000,
                           const uint32 max_text_length = 1000) {
    const PackedStringSet p = as_packed_string_set(patterns), t = as_packed_string_set(texts);
    AlignmentStream<aligner_type> stream(aligner, p.size(), p.m_offsets, p.m_words, max_pattern_length, 0, t.m_words,
                                         max_text_length, NULL);
    stream.m_text_offsets = t.m_offsets;
    stream.m_pattern_bits = p.m_bits; stream.m_pattern_big_endian = p.m_big_endian;
    stream.m_text_bits = t.m_bits; stream.m_text_big_endian = t.m_big_endian;
    stream.m_scores32 = sinks.scores;
    stream.m_sinks = sinks.sinks;
    BatchedAlignmentScore<AlignmentStream<aligner_type>, scheduler_type> batch;
    batch.enact(stream);
}

// The outputs of a traceback batch (batched_inl.h:612-664's stream.output(): the Alignment
// and the backtracer of each job), as device arrays: per pair the BestSink score, the
// Alignment's source and sink as (x = text, y = pattern) pairs, and the backtracker's pushes
// in push order (end of the alignment first; 0 SUBSTITUTION, 1 INSERTION, 2 DELETION) at
// ops + k * ops_stride, n_ops[k] of them (ops_stride >= max pattern + max text length).
enum { SUBSTITUTION = 0, INSERTION = 1, DELETION = 2 };   // alignment_base.h:139-147

template <typename aligner_type_T>
struct TracebackStream : AlignmentStream<aligner_type_T> {
    typedef aligner_type_T aligner_type;
    TracebackStream(const aligner_type aligner, const uint32 count, const uint32 *offsets, const uint32 *patterns,
                    const uint32 max_pattern_len, const uint32 total_pattern_len, const uint32 *text,
                    const uint32 text_len, int32 *scores, uint32 *sources, uint32 *sinks, uint8 *ops,
                    const uint32 ops_stride, uint32 *n_ops)
        : AlignmentStream<aligner_type_T>(aligner, count, offsets, patterns, max_pattern_len, total_pattern_len,
                                          text, text_len, nullptr),
          m_sources(sources), m_sinks(sinks), m_ops(ops), m_ops_stride(ops_stride), m_n_ops(n_ops) {
        this->m_scores32 = scores;
    }
    uint32 *m_sources, *m_sinks;
    uint8 *m_ops;
    uint32 m_ops_stride;
    uint32 *m_n_ops;
    uint32 m_max_text_len = 0;   // per-pair texts: the longest (0 = read back)
};

// Feed one job's result (host copies of the stream's outputs) to an nvbio Backtracer (push(op),
// clip(len)) in the order alignment_traceback calls it (alignment_inl.h:413-462): the end clip,
// the pushes, the start clip.
template <typename backtracer_type>
void replay(backtracer_type &bt, const uint32 pattern_len, const uint32 source_y, const uint32 sink_y,
            const uint8 *ops, const uint32 n_ops) {
    bt.clip(pattern_len - sink_y);
    for (uint32 i = 0; i < n_ops; ++i) bt.push(ops[i]);
    bt.clip(source_y);
}

template <uint32 CHECKPOINTS, typename stream_type, typename scheduler_type = DeviceThreadScheduler>
struct BatchedAlignmentTraceback {
    typedef stream_type input_stream_type;
    typedef typename stream_type::aligner_type aligner_type;

    // the workspace (flags of every cell, one DP row per pair) is the engine's, not the caller's:
    // these report what enact() reserves in it (batches past 4 GB of it run in chunks), so a
    // caller sizing its batches from them sees the device memory a call takes.
    // enact() calls sharing one engine() must be serialised: they share that workspace.
    static uint64 min_temp_storage(const uint32 max_pattern_len, const uint32 max_text_len, const uint32) {
        return gasalx_nv_traceback_workspace(max_pattern_len, max_text_len, 1);
    }
    static uint64 max_temp_storage(const uint32 max_pattern_len, const uint32 max_text_len, const uint32 n) {
        return gasalx_nv_traceback_workspace(max_pattern_len, max_text_len, n);
    }

    void enact(stream_type stream, uint64 temp_size = 0u, uint8 *temp = NULL, void *hip_stream = NULL) {
        static_assert(!is_myers_tag<typename aligner_type::algorithm_tag>::value,
                      "MyersTag aligners run under BatchedBandedAlignmentScore only: nvbio has the banded Myers "
                      "scorer (myers/myers_banded_inl.h) and no full-DP or traceback form of it");
        static_assert(!uses_quality_scheme<aligner_type>::value,
                      "QualityGotohScheme runs under BatchedBandedAlignmentScore / batch_banded_alignment_score and "
                      "BatchedBandedAlignmentTraceback only: the full-DP scorer and traceback have no quality kernels");
        (void)temp_size; (void)temp;
        const gasalx_nv_aligner a = stream.aligner().c_aligner();
        gasalx_nv_strings p = {stream.m_patterns, stream.m_offsets, 0, stream.m_pattern_bits,
                               stream.m_pattern_big_endian};
        gasalx_nv_strings t = {stream.m_text, stream.m_text_offsets, stream.m_text_len, stream.m_text_bits,
                               stream.m_text_big_endian};
        const uint32 max_text_len = stream.m_text_offsets ? stream.m_max_text_len : stream.m_text_len;
        int rc;
        if constexpr (uses_matrix_scheme<aligner_type>::value) {
            // GotohAligner over SubstitutionMatrixScheme: the matrix traceback, the same workspace and outputs
            const gasalx_nv_matrix m = stream.aligner().scheme.c_matrix();
            rc = gasalx_nv_matrix_traceback_device(engine(), &a, &m, stream.size(), &p, &t, stream.max_pattern_length(),
                                                   max_text_len, stream.m_scores32, stream.m_sources, stream.m_sinks,
                                                   stream.m_ops, stream.m_ops_stride, stream.m_n_ops, hip_stream);
        } else {
            rc = gasalx_nv_traceback_device(engine(), &a, stream.size(), &p, &t, stream.max_pattern_length(),
                                            max_text_len, stream.m_scores32, stream.m_sources, stream.m_sinks,
                                            stream.m_ops, stream.m_ops_stride, stream.m_n_ops, hip_stream);
        }
        if (rc != GASALX_OK) {
            fprintf(stderr, "BatchedAlignmentTraceback::enact: %s\n", gasalx_last_error());
            exit(EXIT_FAILURE);
        }
    }
};

// Banded traceback (banded_inl.h:352-427): the band's cells (i, i + j), j < BAND_LEN (2..32);
// ops_stride >= 2 x max pattern length + BAND_LEN.  nvBowtie runs BAND_LEN 3 / 7 / 15 / 31
// (nvBowtie/bowtie2/cuda/traceback_inl.h:239-257).  CHECKPOINTS only sizes the reference's
// storage; the flags of every cell live in the engine's workspace here.
template <uint32 BAND_LEN, uint32 CHECKPOINTS, typename stream_type, typename scheduler_type = DeviceThreadScheduler>
struct BatchedBandedAlignmentTraceback {
    typedef stream_type input_stream_type;
    typedef typename stream_type::aligner_type aligner_type;

    // the engine's workspace a call reserves (see BatchedAlignmentTraceback)
    static uint64 min_temp_storage(const uint32 max_pattern_len, const uint32, const uint32) {
        return gasalx_nv_banded_traceback_workspace(max_pattern_len, BAND_LEN, 1);
    }
    static uint64 max_temp_storage(const uint32 max_pattern_len, const uint32, const uint32 n) {
        return gasalx_nv_banded_traceback_workspace(max_pattern_len, BAND_LEN, n);
    }

    void enact(stream_type stream, uint64 temp_size = 0u, uint8 *temp = NULL, void *hip_stream = NULL) {
        static_assert(!is_myers_tag<typename aligner_type::algorithm_tag>::value,
                      "MyersTag aligners run under BatchedBandedAlignmentScore only: nvbio has the banded Myers "
                      "scorer (myers/myers_banded_inl.h) and no full-DP or traceback form of it");
        static_assert(!uses_matrix_scheme<aligner_type>::value,
                      "SubstitutionMatrixScheme runs under BatchedAlignmentScore / batch_alignment_score and "
                      "BatchedAlignmentTraceback only: the banded scorer and the banded traceback have no matrix kernels");
        (void)temp_size; (void)temp;
        const gasalx_nv_aligner a = stream.aligner().c_aligner();
        gasalx_nv_strings p = {stream.m_patterns, stream.m_offsets, 0, stream.m_pattern_bits,
                               stream.m_pattern_big_endian};
        gasalx_nv_strings t = {stream.m_text, stream.m_text_offsets, stream.m_text_len, stream.m_text_bits,
                               stream.m_text_big_endian};
        int rc;
        if constexpr (uses_quality_scheme<aligner_type>::value) {
            if (stream.m_quals == NULL) {
                fprintf(stderr, "BatchedBandedAlignmentTraceback::enact: a QualityGotohScheme aligner needs the "
                                "patterns' qualities, call set_quals() on the stream\n");
                exit(EXIT_FAILURE);
            }
            const gasalx_nv_quals q = stream.aligner().scheme.c_quals(stream.m_quals);
            rc = gasalx_nv_banded_qual_traceback_device(engine(), &a, &q, BAND_LEN, stream.size(), &p, &t,
                                                        stream.max_pattern_length(), stream.m_scores32,
                                                        stream.m_sources, stream.m_sinks, stream.m_ops,
                                                        stream.m_ops_stride, stream.m_n_ops, hip_stream);
        } else {
            rc = gasalx_nv_banded_traceback_device(engine(), &a, BAND_LEN, stream.size(), &p, &t,
                                                   stream.max_pattern_length(), stream.m_scores32, stream.m_sources,
                                                   stream.m_sinks, stream.m_ops, stream.m_ops_stride, stream.m_n_ops,
                                                   hip_stream);
        }
        if (rc != GASALX_OK) {
            fprintf(stderr, "BatchedBandedAlignmentTraceback::enact: %s\n", gasalx_last_error());
            exit(EXIT_FAILURE);
        }
    }
};

}  // namespace aln
}  // namespace nvbio

#endif
