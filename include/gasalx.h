/*
 * gasalx.h — flat C-ABI of the MI355X GASAL2-compatible engine (FFI boundary).
 *
 * Plain pointers and sizes only; no HIP or torch types in the signatures
 * (streams are passed as void*, i.e. a hipStream_t).  The entry points are the
 * ones a ctypes / cgo / JNI binding of the reference's path would bind:
 *
 *   gasalx_align_host    <- gasal_aln(...)   (Non-CDP/GASAL2/src/__deprecated.cpp:5,
 *                                             the flat batch call, commented out in
 *                                             the reference; same argument meaning,
 *                                             plus the Parameters fields it needs)
 *   gasalx_align_device  <- gasal_aln_async(...) (gasal_align.cu:29) without the host
 *                           staging: inputs already resident in device memory
 *   gasalx_pairhmm_*     <- pairHMM<<<>>> launch (Non-CDP/PairHMM/inter_task/
 *                           Synthetic_data/tile_1/tile_1.cu:44,507-524)
 *
 * The reference's C++ API (gasal_header.h: gasal_init_streams, gasal_host_batch_fill,
 * gasal_aln_async, gasal_is_aln_async_done, ...) is provided by the same library
 * with C++ linkage.  Every call here returns 0 on success and a negative
 * GASALX_E* code on failure (the reference exits instead, gasal.h:15-22);
 * gasalx_last_error() gives the message of the calling thread's last failure.
 */
#ifndef GASALX_H
#define GASALX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GASALX_ABI_VERSION 1

enum {
    GASALX_OK = 0,
    GASALX_EINVAL = -1,      /* bad argument (sizes, alignment, enum value)          */
    GASALX_ERANGE = -2,      /* sequence length / score range the engine rejects     */
    GASALX_EDEVICE = -3,     /* HIP runtime error                                    */
    GASALX_ENOMEM = -4,      /* device or host allocation failed                     */
    GASALX_EUNSUPPORTED = -5 /* configuration not implemented                        */
};

/* Mirrors the Parameters fields the reference's boundary reads
 * plus the compile-time knobs that become run-time values here. */
typedef struct gasalx_params {
    int32_t match;          /* gasal_subst_scores.match                              */
    int32_t mismatch;       /* gasal_subst_scores.mismatch (penalty, positive)       */
    int32_t gap_open;       /* gasal_subst_scores.gap_open                           */
    int32_t gap_extend;     /* gasal_subst_scores.gap_extend                         */
    int32_t algo;           /* enum algo_type                                        */
    int32_t start_pos;      /* enum comp_start                                       */
    int32_t second_best;    /* enum Bool                                             */
    int32_t head;           /* enum data_source, semi-global skipped head            */
    int32_t tail;           /* enum data_source, semi-global skipped tail            */
    int32_t k_band;         /* BANDED band width in bases (kernel uses k_band >> 3)  */
    int32_t is_packed;      /* inputs are already 4-bit packed words                 */
    int32_t n_code;         /* reference N_CODE (0x4E for ASCII input)               */
    int32_t has_n_penalty;  /* reference N_PENALTY defined?                          */
    int32_t n_penalty;
    int32_t max_query_len;  /* reference MAX_QUERY_LEN (0 = large enough for the batch) */
} gasalx_params;

/* Batch description; the pointers are device pointers for gasalx_align_device and
 * host pointers for gasalx_align_host.  Layout as the reference's host batch:
 * sequences concatenated, each padded with N_CODE to a multiple of 8, offsets in
 * bytes including the pads, lengths without them (GASAL2 README.md:145). */
typedef struct gasalx_batch {
    const uint8_t *q_batch;
    const uint32_t *q_offsets;
    const uint32_t *q_lens;
    const uint8_t *t_batch;
    const uint32_t *t_offsets;
    const uint32_t *t_lens;
    uint32_t q_bytes;             /* multiple of 8 */
    uint32_t t_bytes;             /* multiple of 8 */
    uint32_t n_alns;
    const uint8_t *q_ops;         /* enum operation_on_seq per pair, or NULL */
    const uint8_t *t_ops;
    const uint32_t *seed_scores;  /* KSW h0 per pair, or NULL */
    uint32_t max_q_len;           /* upper bound of q_lens (0 = unknown: the engine reads   */
    uint32_t max_t_len;           /* the lengths back, which synchronises the stream).      */
                                  /* SEMI_GLOBAL with TAIL = QUERY/BOTH, score only, reads  */
                                  /* back the histogram of padded target lengths (one sync */
                                  /* of the stream) even when both are given; the host     */
                                  /* entry points skip it when every target has the same   */
                                  /* padded length                                         */
} gasalx_batch;

/* Output arrays (n_alns entries; cigar has q_bytes entries).  NULL = not wanted.
 * Fields the reference would not write for the configuration are untouched. */
typedef struct gasalx_results {
    int32_t *aln_score;
    int32_t *q_end;
    int32_t *t_end;
    int32_t *q_start;
    int32_t *t_start;
    int32_t *aln_score2;
    int32_t *q_end2;
    int32_t *t_end2;
    uint8_t *cigar;          /* reversed RLE bytes at each pair's query offset     */
    uint32_t *n_cigar_ops;
} gasalx_results;

typedef struct gasalx_engine gasalx_engine;   /* device workspace, one per thread */

int gasalx_abi_version(void);
const char *gasalx_last_error(void);

int gasalx_device_count(int *count);
int gasalx_engine_create(int device, gasalx_engine **out);
int gasalx_engine_destroy(gasalx_engine *eng);

/* Asynchronous on `stream` (a hipStream_t; NULL = the engine's own stream). */
int gasalx_align_device(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *dev_batch,
                        const gasalx_results *dev_out, void *stream);

/* Synchronous host-to-host call (H2D, kernels, D2H). */
int gasalx_align_host(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *host_batch,
                      const gasalx_results *host_out);

/* Page-locked host memory from the HIP runtime libgasal itself uses (hipHostMalloc),
 * for caller-owned input / result buffers (the reference's host pages and host_res
 * are pinned: host_batch.cpp:79-153, res.cpp:8-70).  Freed with gasalx_host_free. */
int gasalx_host_alloc(uint64_t bytes, void **out);
int gasalx_host_free(void *ptr);

/* Which kernel family the dispatcher selects for a batch (for tests/profiling):
 * writes a short NUL-terminated name into buf. */
int gasalx_describe_plan(const gasalx_params *params, uint32_t max_q_len, uint32_t max_t_len, char *buf,
                         uint32_t buf_len);

/* SEMI_GLOBAL with HEAD = TARGET and TAIL = TARGET, with the alignment itself -- what a read mapper
 * asks for and what the reference's semi-global kernel cannot give (it has no traceback branch;
 * gasalx_align_* with WITH_TB keeps the reference's behaviour there).  params->algo must be
 * SEMI_GLOBAL, second_best FALSE; any other HEAD / TAIL is GASALX_EUNSUPPORTED; start_pos is ignored.
 *   aln_score, q_end, t_end   what gasalx_align_* returns with WITHOUT_START, bit for bit
 *   cigar, n_cigar_ops        reversed RLE bytes count << 2 | op (0 M, 1 X, 2 D, 3 I) at each pair's
 *                             query offset; a pair's ops consume its whole query and the target
 *                             bases t_start .. t_end.  cigar must be a buffer of its own, q_bytes
 *                             long (GASALX_EINVAL when it overlaps q_batch); bytes past a pair's
 *                             ops are not written by the device form and are 0 from the host form
 *   t_start                   the first target base the path consumes (t_end + 1 when it consumes
 *                             none); q_start = 0
 * Required outputs: aln_score, cigar, n_cigar_ops; the second-best fields must be NULL.  q_ops /
 * t_ops and is_packed as in gasalx_align_*.  A gap run ends in the cell it was opened from (the
 * semi-global matrix opens gaps from H), so an I run may stand next to a D run.  A negative
 * gap_open or gap_extend is GASALX_EUNSUPPORTED; lengths with no wavefront shape (a padded query
 * over 1,280, LDS over 160 KB, or lengths x scores past the int16 range the semi-global kernels
 * keep) are GASALX_ERANGE.  The device form is asynchronous on `stream`
 * when max_q_len / max_t_len are given.  gasalx_describe_semi_cigar_plan names the kernel family of
 * the direction-flag launch ("wavefront16_semi_tb_G..R..", or "wavefront_semi_tb_G..R.." when
 * every block takes the int32 kernel), or returns the error the call would. */
int gasalx_semi_cigar_device(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *dev_batch,
                             const gasalx_results *dev_out, void *stream);
int gasalx_semi_cigar_host(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *host_batch,
                           const gasalx_results *host_out);
int gasalx_describe_semi_cigar_plan(const gasalx_params *params, uint32_t max_q_len, uint32_t max_t_len, char *buf,
                                    uint32_t buf_len);

/* The same call for every HEAD: params->head is NONE, QUERY, TARGET or BOTH, params->tail must be TARGET
 * (anything else is GASALX_EUNSUPPORTED).  Structs, required outputs, the overlay check, the capacity
 * rule, q_ops / t_ops / is_packed and the order of the errors are those of gasalx_semi_cigar_*; messages
 * start "semi_cigar_head:".  With HEAD = TARGET every output is byte-identical to gasalx_semi_cigar_*.
 *   aln_score, q_end, t_end   what gasalx_align_* returns for that HEAD with WITHOUT_START, bit for bit
 *   HEAD NONE    anchored at (0, 0): the ops consume the whole query and target bases 0 .. t_end; t_start
 *                = 0, q_start = 0.  Target bases left of the path's first cell are a leading D run
 *   HEAD QUERY   the query's prefix is free: the ops consume query bases q_start .. and target bases
 *                0 .. t_end; t_start = 0
 *   HEAD BOTH    either prefix is free: query bases q_start .., target bases t_start .. t_end
 *   q_start      written when the pointer is given (0 under HEAD NONE / TARGET)
 * Boundary prices a caller who re-scores a path must know (they are the reference kernel's, Q3 of the
 * survey): a deletion run that starts at a free query head (HEAD QUERY / BOTH, q_start > 0, the path's
 * first op) costs e per base, not o + e -- E(r, -1) = 0 there; under HEAD NONE / QUERY the value above
 * cell (0, c) is -(o + e*c), so a leading D run of k bases followed by M / X costs o + e*k, followed by
 * an insertion o + e*(k - 1): c + 1 target bases stand above column c for the price of c, one base for
 * o.  Under HEAD NONE / TARGET a leading I run of k bases at t_start = 0 costs o + e*(k - 1), one base
 * nothing, as in gasalx_semi_cigar_*.
 * gasalx_describe_semi_cigar_head_plan: the names of gasalx_describe_semi_cigar_plan with the head
 * appended (_hn, _hq, _ht, _hb). */
int gasalx_semi_cigar_head_device(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *dev_batch,
                                  const gasalx_results *dev_out, void *stream);
int gasalx_semi_cigar_head_host(gasalx_engine *eng, const gasalx_params *params, const gasalx_batch *host_batch,
                                const gasalx_results *host_out);
int gasalx_describe_semi_cigar_head_plan(const gasalx_params *params, uint32_t max_q_len, uint32_t max_t_len,
                                         char *buf, uint32_t buf_len);

/* Diagnostics: pairs of the engine's last packed (two-pairs-per-lane) launches that the packed
 * kernel aligned itself (*handled) out of the pairs those launches covered (*total); the rest went
 * to the int32 kernel.  The engine's own workspace and its two host-pipeline stages each count
 * their last packed launch (a WITH_START call: the reverse pass) and forgets it once read.
 * Synchronises the engine's streams; 0 / 0 when no packed launch ran since the last read. */
int gasalx_packed_pairs(gasalx_engine *engine, uint64_t *handled, uint64_t *total);

/* PairHMM forward.  Per read base: read byte and the four per-base parameters
 * (qm = ph2pr[bq], delta = ph2pr[iq], xiksi = ph2pr[dq], alpha = 1 - ph2pr[(iq+dq)&127],
 * tile_1.cu:415-419) at the read's offset; haplotype bytes at hap offsets. */
typedef struct gasalx_hmm_batch {
    const uint8_t *reads;
    const uint32_t *read_offsets;
    const uint32_t *read_lens;
    const float *qm;
    const float *delta;
    const float *xiksi;
    const float *alpha;
    const uint8_t *haps;
    const uint32_t *hap_offsets;
    const uint32_t *hap_lens;
    uint32_t read_bytes;
    uint32_t hap_bytes;
    uint32_t n_pairs;
    uint32_t max_read_len;        /* upper bounds (0 = unknown, read back from the device) */
    uint32_t max_hap_len;
} gasalx_hmm_batch;

int gasalx_pairhmm_device(gasalx_engine *eng, const gasalx_hmm_batch *dev_batch, float *dev_result, void *stream);
int gasalx_pairhmm_host(gasalx_engine *eng, const gasalx_hmm_batch *host_batch, float *host_result);

/* Host-side helper: per-base PairHMM parameters from Phred qualities
 * (tile_1.cu:216-220 ph2pr table, :415-419). */
int gasalx_pairhmm_params(const uint8_t *bq, const uint8_t *iq, const uint8_t *dq, uint32_t n, float *qm,
                          float *delta, float *xiksi, float *alpha);

/* PairHMM from Phred qualities: the reference's input format (tile_1.cu:246-290,
 * Intra-task/real_data/improved_warp_based/improved_warp_based.cu:240-279).  base /
 * insertion / deletion quality bytes sit at the read offsets; the four per-base
 * parameters are formed on the device from the same ph2pr table the reference's host
 * builds (powf(10, -q/10), tile_1.cu:216-220; mapping :415-419), so the kernel's
 * input is 4 bytes per read base instead of 17. */
typedef struct gasalx_hmm_qual_batch {
    const uint8_t *reads;
    const uint32_t *read_offsets;
    const uint32_t *read_lens;
    const uint8_t *base_quals;
    const uint8_t *ins_quals;
    const uint8_t *del_quals;
    const uint8_t *haps;
    const uint32_t *hap_offsets;
    const uint32_t *hap_lens;
    uint64_t read_bytes;          /* bytes of reads (and of each quality array) */
    uint64_t hap_bytes;
    uint32_t n_pairs;
    uint32_t max_read_len;        /* upper bounds (0 = unknown) */
    uint32_t max_hap_len;
} gasalx_hmm_qual_batch;

/* Device-resident batch: one launch, lane groups sized by the longest read. */
int gasalx_pairhmm_quals_device(gasalx_engine *eng, const gasalx_hmm_qual_batch *dev_batch, float *dev_result,
                                void *stream);
/* Host arrays in, results out in input order.  Pairs run sorted by (read length,
 * haplotype length) as the reference's host sorts them (tile_1.cu:180-195,325), in
 * classes of reads that share a lane-group size (one launch each) instead of the
 * reference's 32-pair interleaved chunks (tile_1.cu:346-500). */
int gasalx_pairhmm_quals_host(gasalx_engine *eng, const gasalx_hmm_qual_batch *host_batch, float *host_result);

/* PairHMM in float64.  The fp32 entry points above start from the constant 2^120 and return 0
 * for a read that fits its haplotype badly (the value underflows the fp32 range).  These run the
 * same recurrence on the same fp32 inputs, widened, in double from the constant 2^1020.
 *
 * raw float64 forward value of every pair, initial constant 2^1020 */
int gasalx_pairhmm64_device(gasalx_engine *eng, const gasalx_hmm_batch *dev_batch, double *dev_result, void *stream);
int gasalx_pairhmm64_host(gasalx_engine *eng, const gasalx_hmm_batch *host_batch, double *host_result);
int gasalx_pairhmm64_quals_device(gasalx_engine *eng, const gasalx_hmm_qual_batch *dev_batch, double *dev_result,
                                  void *stream);
int gasalx_pairhmm64_quals_host(gasalx_engine *eng, const gasalx_hmm_qual_batch *host_batch, double *host_result);

/* log10 likelihoods: fp32 pass, pairs below min_accepted (<= 0: 1e-28f) rescued in float64.
 * Output i is log10(value) - log10(initial constant) of pair i: log10(r) - 120 log10(2) from
 * an accepted fp32 result, log10(r64) - 1020 log10(2) from a rescued pair.
 * An fp32 result that is 0, denormal, infinite or NaN is rescued whatever min_accepted is.
 * used_double (may be NULL): 1 per rescued pair.  n_rescued (may be NULL, host form only).
 * The device forms stay asynchronous on the stream when max_read_len / max_hap_len are set:
 * the rescue list and its length stay on the device. */
int gasalx_pairhmm_log10_device(gasalx_engine *eng, const gasalx_hmm_batch *dev_batch, float min_accepted,
                                double *dev_log10, uint8_t *dev_used_double, void *stream);
int gasalx_pairhmm_log10_host(gasalx_engine *eng, const gasalx_hmm_batch *host_batch, float min_accepted,
                              double *host_log10, uint8_t *host_used_double, uint32_t *n_rescued);
int gasalx_pairhmm_quals_log10_device(gasalx_engine *eng, const gasalx_hmm_qual_batch *dev_batch, float min_accepted,
                                      double *dev_log10, uint8_t *dev_used_double, void *stream);
int gasalx_pairhmm_quals_log10_host(gasalx_engine *eng, const gasalx_hmm_qual_batch *host_batch, float min_accepted,
                                    double *host_log10, uint8_t *host_used_double, uint32_t *n_rescued);

/* Reader of the reference's PairHMM input files: groups of `size` pairs, each pair
 * = read length, read bases, then read-length base / insertion / deletion / gcp
 * qualities, haplotype length, haplotype bases (whitespace-separated, fscanf
 * semantics of tile_1.cu:246-290; qualities stored as (char) values).  Arrays are
 * owned by the returned object (gasalx_hmm_file_free). */
typedef struct gasalx_hmm_file {
    uint32_t n_pairs;
    uint32_t n_groups;
    uint32_t *group_sizes;        /* pairs per group, in file order */
    uint8_t *reads;
    uint32_t *read_offsets;
    uint32_t *read_lens;
    uint8_t *base_quals, *ins_quals, *del_quals, *gcp_quals;
    uint8_t *haps;
    uint32_t *hap_offsets;
    uint32_t *hap_lens;
    uint64_t read_bytes;
    uint64_t hap_bytes;
} gasalx_hmm_file;

int gasalx_hmm_file_read(const char *path, gasalx_hmm_file **out);
int gasalx_hmm_file_free(gasalx_hmm_file *f);

/* Second front-end: nvbio-style batched alignment scoring (NvB/nvbio/alignment/
 * batched.h:44-87, the BatchedAlignmentScore<stream, scheduler> idiom of
 * sw-benchmark.cu:355-443; C++ wrapper in include/nvbio_batched.h).  nvbio's textbook
 * recurrences, not GASAL2's: Gotoh (gotoh/gotoh_inl.h), Smith-Waterman with linear
 * gaps (sw/sw_inl.h), edit distance (ed/ed_utils.h:45-52), each GLOBAL / LOCAL /
 * SEMI_GLOBAL (pattern fully aligned, text ends free); the output is the BestSink
 * score per pair. */
enum { GASALX_NV_ED = 0, GASALX_NV_SW = 1, GASALX_NV_GOTOH = 2 };
enum { GASALX_NV_GLOBAL = 0, GASALX_NV_LOCAL = 1, GASALX_NV_SEMI_GLOBAL = 2 };   /* nvbio AlignmentType */

typedef struct gasalx_nv_aligner {
    int32_t aligner;      /* GASALX_NV_ED / _SW / _GOTOH */
    int32_t type;         /* GASALX_NV_GLOBAL / _LOCAL / _SEMI_GLOBAL */
    int32_t match;        /* signed scores as in SimpleGotohScheme / SimpleSmithWatermanScheme */
    int32_t mismatch;     /*   (utils.h:92-135): penalties are negative                        */
    int32_t gap_open;     /* Gotoh: a gap of k symbols scores gap_open + (k-1) * gap_ext         */
    int32_t gap_ext;
    int32_t deletion;     /* Smith-Waterman: per text symbol skipped                            */
    int32_t insertion;    /* Smith-Waterman: per pattern symbol skipped                         */
} gasalx_nv_aligner;

/* A packed string set (nvbio PackedStream): symbol s of the set is field s % (32/bits)
 * of word s / (32/bits), counted from the top of the word when big_endian (nvbio reads,
 * SequenceDataTraits SEQUENCE_BIG_ENDIAN) or from bit 0 otherwise (sw-benchmark's
 * 2-bit reference, REF_BIG_ENDIAN = false). */
typedef struct gasalx_nv_strings {
    const uint32_t *words;
    const uint32_t *offsets;  /* n + 1 symbol offsets; texts: NULL = one text of `length` symbols for every pair */
    uint32_t length;
    uint32_t bits;            /* 2, 4 or 8 */
    uint32_t big_endian;
} gasalx_nv_strings;

/* scores (int32) and/or scores16 (int16, sw-benchmark's score vector) per pair.
 * Patterns up to 1024 symbols; max lengths are upper bounds (0 = read back). */
int gasalx_nv_score_device(gasalx_engine *eng, const gasalx_nv_aligner *aligner, uint32_t n_pairs,
                           const gasalx_nv_strings *dev_patterns, const gasalx_nv_strings *dev_texts,
                           int32_t *dev_scores, int16_t *dev_scores16, uint32_t max_pattern_len,
                           uint32_t max_text_len, void *stream);
/* The kernel a gasalx_nv_score_* call with these bounds runs (e.g.
 * "nvbio16_gotoh_semi_shared_G8R19": the packed kernel, two pairs per lane group;
 * "nvbio_..." the int32 one); per_pair_texts = 0 for one shared text. */
int gasalx_nv_describe_plan(const gasalx_nv_aligner *aligner, uint32_t max_pattern_len, uint32_t max_text_len,
                            int per_pair_texts, uint32_t text_bits, char *buf, uint32_t buf_len);
/* Host arrays in and out (words: the number of words of each set). */
int gasalx_nv_score_host(gasalx_engine *eng, const gasalx_nv_aligner *aligner, uint32_t n_pairs,
                         const gasalx_nv_strings *patterns, uint64_t pattern_words, const gasalx_nv_strings *texts,
                         uint64_t text_words, int32_t *scores, int16_t *scores16);

/* Score and sink: what nvbio's alignment_score(aligner, pattern, text, min_score, sink) leaves
 * in a BestSink (sink_inl.h:59-68) under a TextBlockingTag aligner: the score and the cell where
 * it was reached, sinks[2k] = x (text column) and sinks[2k + 1] = y (pattern row), one-based:
 * the coordinates and layout of gasalx_nv_traceback_*'s sinks.  BestSink keeps the last maximum
 * in report order: LOCAL reports every cell, text stripes of 8 columns (Gotoh) or 16 (Smith-Waterman,
 * edit distance: nvbio's BAND_LEN of the aligner) left to right, inside a
 * stripe the pattern rows top to bottom, inside a row the columns left to right; SEMI_GLOBAL the
 * last pattern row left to right (the rightmost maximum); GLOBAL the cell (N, M).  A pair that
 * reports no cell (an empty text; LOCAL: an empty pattern) gets INT32_MIN and (0xFFFFFFFF,
 * 0xFFFFFFFF).  PatternBlockingTag reports in another order: its tied sinks are not provided.
 * scores (int32) or sinks may be NULL, not both.  Limits, checks and error codes as
 * gasalx_nv_score_*.  The full DP only (not banded). */
int gasalx_nv_score_sinks_device(gasalx_engine *eng, const gasalx_nv_aligner *aligner, uint32_t n_pairs,
                                 const gasalx_nv_strings *dev_patterns, const gasalx_nv_strings *dev_texts,
                                 int32_t *dev_scores, uint32_t *dev_sinks, uint32_t max_pattern_len,
                                 uint32_t max_text_len, void *stream);
int gasalx_nv_score_sinks_host(gasalx_engine *eng, const gasalx_nv_aligner *aligner, uint32_t n_pairs,
                               const gasalx_nv_strings *patterns, uint64_t pattern_words,
                               const gasalx_nv_strings *texts, uint64_t text_words, int32_t *scores,
                               uint32_t *sinks);
/* The kernel a gasalx_nv_score_sinks_* call with these bounds runs (e.g.
 * "nvbio16_gotoh_local_shared_G8R19_sink"): the score-only plan's name with "_sink" appended,
 * the packed or the int32 kernel by the same rule; arguments as gasalx_nv_describe_plan. */
int gasalx_nv_describe_sinks_plan(const gasalx_nv_aligner *aligner, uint32_t max_pattern_len, uint32_t max_text_len,
                                  int per_pair_texts, uint32_t text_bits, char *buf, uint32_t buf_len);

/* Gotoh scoring with a substitution matrix: what nvbio's GotohAligner computes when its scheme
 * answers substitution(r_i, q_j, r, q, qq) from a table (gotoh/gotoh_inl.h:534, :1042; the
 * proteinsw example's BlosumScheme, examples/proteinsw/proteinsw.cu:76-100): in the Gotoh cell
 * update S(p, t) = scores[t + p * n].  Proteins, codons, IUPAC codes: the caller supplies the
 * table, none is shipped. */
typedef struct gasalx_nv_matrix {
    const int8_t *scores;   /* HOST pointer: n*n entries, scores[t + p*n] (t = text symbol, p = pattern symbol) */
    uint32_t n;             /* 2..32 */
} gasalx_nv_matrix;

/* aligner: GASALX_NV_GOTOH (Smith-Waterman and edit distance never read a substitution score
 * from the scheme, sw_inl.h: GASALX_EUNSUPPORTED); match and mismatch are ignored, gap_open and
 * gap_ext used as given.  The table is read during the call (it travels to the kernel by value):
 * the caller may free or change it on return, and calls on different streams share nothing.
 * A symbol >= n is read as n - 1 (the reference indexes past its table there).  dev_scores
 * (int32) and dev_sinks (2 x n_pairs) have the layout and semantics of gasalx_nv_score_sinks_*:
 * one-based (x, y), the last maximum in the TextBlockingTag report order, INT32_MIN and
 * (0xFFFFFFFF, 0xFFFFFFFF) for a pair that reports no cell; either may be NULL, not both
 * (GASALX_EINVAL); without sinks the score-only kernel runs.  int32, the full DP only.
 * GASALX_EINVAL: n outside 2..32, a NULL table, symbol bits other than 2 / 4 / 8.  GASALX_ERANGE:
 * gasalx_nv_score_*'s range check with the largest |entry| in place of match and mismatch; a
 * pattern above 1024 symbols or texts that do not fit the LDS (one byte per symbol). */
int gasalx_nv_matrix_score_device(gasalx_engine *eng, const gasalx_nv_aligner *aligner,
                                  const gasalx_nv_matrix *matrix, uint32_t n_pairs,
                                  const gasalx_nv_strings *dev_patterns, const gasalx_nv_strings *dev_texts,
                                  int32_t *dev_scores, uint32_t *dev_sinks, uint32_t max_pattern_len,
                                  uint32_t max_text_len, void *stream);
int gasalx_nv_matrix_score_host(gasalx_engine *eng, const gasalx_nv_aligner *aligner,
                                const gasalx_nv_matrix *matrix, uint32_t n_pairs,
                                const gasalx_nv_strings *patterns, uint64_t pattern_words,
                                const gasalx_nv_strings *texts, uint64_t text_words, int32_t *scores,
                                uint32_t *sinks);
/* The kernel such a call runs: "nvbio_matrix_gotoh_<global|local|semi>[_shared]_G<g>R<r>[_sink]"
 * (e.g. proteinsw's 128 x 1024 per-pair batch: "nvbio_matrix_gotoh_local_G8R16"), "none" when the
 * bounds do not plan, or the code the call would return for the aligner and matrix_n. */
int gasalx_nv_describe_matrix_plan(const gasalx_nv_aligner *aligner, uint32_t matrix_n, uint32_t max_pattern_len,
                                   uint32_t max_text_len, int per_pair_texts, int want_sinks, char *buf,
                                   uint32_t buf_len);

/* nvbio's BatchedBandedAlignmentScore<band_len> (NvB/nvbio/alignment/batched.h:337,
 * batched_banded_inl.h:44-75): the banded DP of sw_banded_inl.h / gotoh_banded_inl.h /
 * ed_banded_inl.h over cells (i, i + j), 0 <= j < band_len (2..32): two pairs per lane in
 * 16-bit halves for 2-bit texts inside the value window, else one pair per thread (int32).
 * BestSink score per pair; INT32_MIN when a text is shorter than its pattern (skipped,
 * as the reference does). */
int gasalx_nv_banded_score_device(gasalx_engine *eng, const gasalx_nv_aligner *aligner, uint32_t band_len,
                                  uint32_t n_pairs, const gasalx_nv_strings *dev_patterns,
                                  const gasalx_nv_strings *dev_texts, int32_t *dev_scores,
                                  uint32_t max_pattern_len, void *stream);   /* max_pattern_len: 0 = read back */
int gasalx_nv_banded_score_host(gasalx_engine *eng, const gasalx_nv_aligner *aligner, uint32_t band_len,
                                uint32_t n_pairs, const gasalx_nv_strings *patterns, uint64_t pattern_words,
                                const gasalx_nv_strings *texts, uint64_t text_words, int32_t *scores);

/* The banded scorer with the sink nvbio's call leaves beside the score
 * (banded_alignment_score<BAND_LEN>(aligner, pattern, quals, text, min_score, sink), what nvBowtie
 * places its banded traceback by): the BestSink score and position of every pair, the score and
 * sink gasalx_nv_banded_traceback_* computes, without the flags and the walk.  ED, SW and Gotoh
 * aligners.  sinks: two uint32 per pair in gasalx_nv_score_sinks_*'s layout, sinks[2k] = x (text),
 * sinks[2k + 1] = y (pattern), one-based; on ties the last maximum in report order
 * (sw_banded_inl.h:436,465,494-510, gotoh_banded_inl.h:642-659): LOCAL every cell (i + j + 1,
 * i + 1), rows top to bottom and band slots left to right, slots past the text's end included
 * (x may exceed the text length); SEMI_GLOBAL (M + j, M) for j < min(M + band - 1, N) - (M - 1);
 * GLOBAL (M + band - 1, M).  A text shorter than its pattern, and a LOCAL pair with an empty
 * pattern, report nothing: INT32_MIN and (0xFFFFFFFF, 0xFFFFFFFF).  scores or sinks may be NULL,
 * not both (GASALX_EINVAL).  Scores equal gasalx_nv_banded_score_*'s; the packed and the int32
 * kernel are chosen by the same rule and give the same outputs. */
int gasalx_nv_banded_score_sinks_device(gasalx_engine *eng, const gasalx_nv_aligner *aligner, uint32_t band_len,
                                        uint32_t n_pairs, const gasalx_nv_strings *dev_patterns,
                                        const gasalx_nv_strings *dev_texts, int32_t *dev_scores,
                                        uint32_t *dev_sinks, uint32_t max_pattern_len,
                                        void *stream);   /* max_pattern_len: 0 = read back */
int gasalx_nv_banded_score_sinks_host(gasalx_engine *eng, const gasalx_nv_aligner *aligner, uint32_t band_len,
                                      uint32_t n_pairs, const gasalx_nv_strings *patterns, uint64_t pattern_words,
                                      const gasalx_nv_strings *texts, uint64_t text_words, int32_t *scores,
                                      uint32_t *sinks);
/* The kernel such a call runs: "nvbio_banded16_<aligner>_<type>_b<8|16|32>_sink" (two pairs per
 * lane) or "nvbio_banded_..._sink" (int32), e.g. "nvbio_banded16_gotoh_local_b16_sink"; or the
 * code the call would return (band_len outside 2..32: GASALX_EINVAL).  max_pattern_len: the
 * longest pattern of the batch (0, a batch of empty patterns, takes the int32 kernel). */
int gasalx_nv_describe_banded_sinks_plan(const gasalx_nv_aligner *aligner, uint32_t band_len,
                                         uint32_t max_pattern_len, uint32_t text_bits, char *buf, uint32_t buf_len);

/* The same banded scorer with nvbio's Myers bit-vector aligner, EditDistanceAligner<TYPE,
 * MyersTag<alphabet_size>> (qmap's and fmmap's configuration; NvB/nvbio/alignment/myers/
 * myers_banded_inl.h:226-288, banded_myers<band_len, 0, TYPE, alphabet_size>).  Not the banded
 * DP's numbers: the function has its own report rule (SEMI_GLOBAL reports the text columns
 * min(N - 1, M) + 1 .. N while the pattern's last row is inside the 32-bit column, never column
 * M of a longer text; GLOBAL reports (N, M) once), so scores and sinks are those of nvbio's Myers
 * path.  type: GASALX_NV_GLOBAL or _SEMI_GLOBAL (_LOCAL: GASALX_EUNSUPPORTED, the reference has
 * none); alphabet_size 2, 4 or 5 (symbols are masked with 1 / 3; under 5, pattern symbols above 4
 * match nothing and text symbols above 4 read as 4; the mask of symbol 4 starts at 0); band_len
 * 2..32 (else GASALX_EINVAL).  scores: the BestSink score (minus the distance) per pair; sinks:
 * two uint32 per pair in gasalx_nv_score_sinks_*'s layout (x = text column, y = pattern row,
 * one-based, the last maximum); either may be NULL, not both.  A text shorter than its pattern
 * reports nothing: INT32_MIN and (0xFFFFFFFF, 0xFFFFFFFF).  max_pattern_len is accepted for
 * symmetry with gasalx_nv_banded_score_device and not needed. */
int gasalx_nv_banded_myers_device(gasalx_engine *eng, int32_t type, uint32_t alphabet_size, uint32_t band_len,
                                  uint32_t n_pairs, const gasalx_nv_strings *dev_patterns,
                                  const gasalx_nv_strings *dev_texts, int32_t *dev_scores, uint32_t *dev_sinks,
                                  uint32_t max_pattern_len, void *stream);
int gasalx_nv_banded_myers_host(gasalx_engine *eng, int32_t type, uint32_t alphabet_size, uint32_t band_len,
                                uint32_t n_pairs, const gasalx_nv_strings *patterns, uint64_t pattern_words,
                                const gasalx_nv_strings *texts, uint64_t text_words, int32_t *scores,
                                uint32_t *sinks);
/* The kernel such a call runs (e.g. "nvbio_myers_semi_a5"), or the code the call would return. */
int gasalx_nv_describe_myers_plan(int32_t type, uint32_t alphabet_size, uint32_t band_len, char *buf,
                                  uint32_t buf_len);

/* nvbio's BatchedAlignmentTraceback<CHECKPOINTS> (NvB/nvbio/alignment/batched.h:436,
 * batched_inl.h:612-664, alignment_inl.h:365-465): the full-DP traceback of the Gotoh,
 * Smith-Waterman and edit-distance aligners (ED runs as SW with 0 / -1 / -1 / -1, as
 * ed/ed_inl.h:347-365 does), GLOBAL / LOCAL /
 * SEMI_GLOBAL, one pair per thread.  Per pair: the BestSink score, the Alignment's source and
 * sink as (x, y) = (text, pattern) coordinates in sources[2k..] / sinks[2k..] (0xFFFFFFFF when no
 * cell was reported), and the backtracker's pushes in push order (end of the alignment first) at
 * ops + k * ops_stride: 0 SUBSTITUTION ('M'), 1 INSERTION ('I', a pattern symbol), 2 DELETION ('D',
 * a text symbol); n_ops[k] of them.  nvbio's Backtracer also receives clip(pattern_len - sink.y)
 * before the pushes and clip(source.y) after them (nvbio_batched.h replays both).
 * ops_stride >= max pattern + max text length; nvbio's int16 DP columns bound
 * (max pattern + max text + 2) * max |score| <= 32767, and pattern x text <= 16 M cells.
 * Workspace: pad8(pattern) x text bytes + 8 bytes per text symbol per pair, held by the engine; a
 * batch runs in chunks of at most 4 GB of it (gasalx_nv_traceback_workspace gives the bytes a
 * call reserves; the environment variable GASALX_NV_TB_BUDGET, in bytes, replaces the 4 GB for
 * both tracebacks: a test knob).  Calls that share an engine must be serialised (one workspace
 * per engine).  gasalx_nv_traceback_workspace also serves gasalx_nv_matrix_traceback_* below: the
 * same layout and size. */
uint64_t gasalx_nv_traceback_workspace(uint32_t max_pattern_len, uint32_t max_text_len, uint32_t n_pairs);
int gasalx_nv_traceback_device(gasalx_engine *eng, const gasalx_nv_aligner *aligner, uint32_t n_pairs,
                               const gasalx_nv_strings *dev_patterns, const gasalx_nv_strings *dev_texts,
                               uint32_t max_pattern_len, uint32_t max_text_len, int32_t *dev_scores,
                               uint32_t *dev_sources, uint32_t *dev_sinks, uint8_t *dev_ops, uint32_t ops_stride,
                               uint32_t *dev_n_ops, void *stream);   /* max lengths: 0 = read back */
int gasalx_nv_traceback_host(gasalx_engine *eng, const gasalx_nv_aligner *aligner, uint32_t n_pairs,
                             const gasalx_nv_strings *patterns, uint64_t pattern_words,
                             const gasalx_nv_strings *texts, uint64_t text_words, int32_t *scores,
                             uint32_t *sources, uint32_t *sinks, uint8_t *ops, uint32_t ops_stride,
                             uint32_t *n_ops);
/* The same traceback for a GotohAligner over a substitution matrix (gasalx_nv_matrix above; the
 * reference's cell update asks the scheme, gotoh/gotoh_inl.h:534, so its templates trace a
 * BlosumScheme unchanged): S(p, t) = scores[t + p * n] in the cell update, everything else
 * (flags, BestSink in the PatternBlockingTag report order, the walk, outputs and coordinates,
 * the sentinel outputs of a pair with an empty string, ops_stride >= max pattern + max text
 * length, max lengths 0 = read back, one shared text) as gasalx_nv_traceback_*.  GLOBAL, LOCAL and
 * SEMI_GLOBAL; the full DP only (the banded traceback has no matrix form).  The workspace has
 * gasalx_nv_traceback_*'s layout and size: gasalx_nv_traceback_workspace serves both, and both
 * run in chunks under the same budget.  The table is read during the call and is the caller's
 * again on return; a symbol >= n is read as n - 1; the aligner's match and mismatch are never read.
 * Checks, in this order: a NULL argument GASALX_EINVAL; a bad aligner or type GASALX_EINVAL, an
 * aligner other than GASALX_NV_GOTOH GASALX_EUNSUPPORTED, n outside 2..32 GASALX_EINVAL; a NULL
 * table GASALX_EINVAL; symbol bits other than 2 / 4 / 8 GASALX_EINVAL; then gasalx_nv_traceback_*'s
 * with the largest |entry| standing for match and mismatch: (max pattern + max text + 2) *
 * max(|entry|, |gap_open|, |gap_ext|) > 32767 GASALX_ERANGE, ops_stride too small GASALX_EINVAL,
 * pattern x text above 16 M cells GASALX_ERANGE. */
int gasalx_nv_matrix_traceback_device(gasalx_engine *eng, const gasalx_nv_aligner *aligner,
                                      const gasalx_nv_matrix *matrix, uint32_t n_pairs,
                                      const gasalx_nv_strings *dev_patterns, const gasalx_nv_strings *dev_texts,
                                      uint32_t max_pattern_len, uint32_t max_text_len, int32_t *dev_scores,
                                      uint32_t *dev_sources, uint32_t *dev_sinks, uint8_t *dev_ops,
                                      uint32_t ops_stride, uint32_t *dev_n_ops, void *stream);
int gasalx_nv_matrix_traceback_host(gasalx_engine *eng, const gasalx_nv_aligner *aligner,
                                    const gasalx_nv_matrix *matrix, uint32_t n_pairs,
                                    const gasalx_nv_strings *patterns, uint64_t pattern_words,
                                    const gasalx_nv_strings *texts, uint64_t text_words, int32_t *scores,
                                    uint32_t *sources, uint32_t *sinks, uint8_t *ops, uint32_t ops_stride,
                                    uint32_t *n_ops);
/* nvbio BatchedBandedAlignmentTraceback<BAND_LEN, CHECKPOINTS, stream> (NvB/nvbio/alignment/
 * batched.h:464-478, batched_banded_inl.h:248-297; nvBowtie's callers traceback_inl.h:239-257):
 * the banded traceback of every pair, band length 2..32 as an argument.  Outputs as
 * gasalx_nv_traceback_*: the BestSink score, source and sink (x = text, y = pattern end) and the
 * pushes in push order; INT32_MIN and (-1, -1) ends for a pair whose text is shorter than its
 * pattern.  ED, SW and Gotoh aligners.  ops_stride >= 2 x max pattern + band; nvbio's int16
 * checkpoints bound (max pattern + band + 3) * max |score| <= 32736.  Workspace: max pattern x
 * pad4(band) bytes per pair, held by the engine, in chunks of at most 4 GB
 * (gasalx_nv_banded_traceback_workspace); calls sharing an engine must be serialised.
 * max_pattern_len 0 = read back. */
uint64_t gasalx_nv_banded_traceback_workspace(uint32_t max_pattern_len, uint32_t band, uint32_t n_pairs);
int gasalx_nv_banded_traceback_device(gasalx_engine *eng, const gasalx_nv_aligner *aligner, uint32_t band,
                                      uint32_t n_pairs, const gasalx_nv_strings *dev_patterns,
                                      const gasalx_nv_strings *dev_texts, uint32_t max_pattern_len,
                                      int32_t *dev_scores, uint32_t *dev_sources, uint32_t *dev_sinks,
                                      uint8_t *dev_ops, uint32_t ops_stride, uint32_t *dev_n_ops, void *stream);
int gasalx_nv_banded_traceback_host(gasalx_engine *eng, const gasalx_nv_aligner *aligner, uint32_t band,
                                    uint32_t n_pairs, const gasalx_nv_strings *patterns, uint64_t pattern_words,
                                    const gasalx_nv_strings *texts, uint64_t text_words, int32_t *scores,
                                    uint32_t *sources, uint32_t *sinks, uint8_t *ops, uint32_t ops_stride,
                                    uint32_t *n_ops);

/* Quality-aware Gotoh scoring for the banded scorer and the banded traceback: what nvBowtie's
 * aligners run, GotohAligner over SmithWatermanScoringScheme<QualCost, ConstantCost>
 * (NvB/nvBowtie/bowtie2/cuda/scoring.h:203-346), whose substitution score depends on the base quality
 * of the pattern symbol: substitution(r_i, q_j, r, q, qq) = r == q ? m_match(qq) : -m_mmp(qq) (:289).
 * The banded Gotoh reads the quality once per row (gotoh/gotoh_banded_inl.h:470). */
typedef struct gasalx_nv_quals {
    const uint8_t *quals;     /* one byte per pattern symbol, indexed by the pattern set's own symbol
                                 offsets: quals[offsets[k] + i] belongs to symbol i of pattern k.
                                 Device memory for *_device, host memory for *_host. */
    const int16_t *match;     /* HOST: levels entries, the score of r == q at quality level l */
    const int16_t *mismatch;  /* HOST: levels entries, the score of r != q (signed: penalties negative) */
    uint32_t levels;          /* 1..256; a quality byte >= levels reads entry levels - 1 */
} gasalx_nv_quals;

/* gasalx_nv_banded_score_sinks_* and gasalx_nv_banded_traceback_* for the Gotoh aligner with the
 * substitution score of row i taken from the tables: S(i, j) = text == pattern ? match[l_i] :
 * mismatch[l_i], l_i = min(quals[i], levels - 1); a text slot past the text's end reads 255 and
 * mismatches.  The aligner's own match and mismatch are never read; gap_open and gap_ext are used
 * as given (the banded Gotoh reads the pattern gap scores only, gotoh_banded_inl.h:444-445).
 * GLOBAL, LOCAL and SEMI_GLOBAL.  Everything else is the plain entry points': the scorer's outputs,
 * sentinels (INT32_MIN, 0xFFFFFFFF), report order and "x may exceed N" rule, scores or sinks NULL
 * but not both; the traceback's five outputs, ops_stride rule, workspace
 * (gasalx_nv_banded_traceback_workspace serves both families) and chunking under
 * GASALX_NV_TB_BUDGET.  The tables are read during the call and are the caller's again on return;
 * calls on different streams share nothing.  The scorer runs two pairs per lane in 16-bit halves
 * for 2-bit texts when gasalx_nv_banded_score_sinks_*'s window rule holds with match = the largest
 * match entry and mismatch = the smallest mismatch entry, and at every level match >= mismatch and
 * match - mismatch <= 255 (GASALX_NVB16=0: int32 only); one pair per thread otherwise.
 * Checks, in this order: a NULL argument, struct or table GASALX_EINVAL; a bad aligner or type
 * GASALX_EINVAL; an aligner other than GASALX_NV_GOTOH GASALX_EUNSUPPORTED; levels outside 1..256
 * GASALX_EINVAL; band_len outside 2..32 GASALX_EINVAL; symbol bits other than 2 / 4 / 8
 * GASALX_EINVAL; then the plain entry points' range rules with the largest |entry| standing for
 * match and mismatch: for the traceback (max pattern + band + 3) * max(|entry|, |gap_open|,
 * |gap_ext|) > 32736 GASALX_ERANGE, then ops_stride < 2 x max pattern + band GASALX_EINVAL. */
int gasalx_nv_banded_qual_score_device(gasalx_engine *eng, const gasalx_nv_aligner *aligner,
                                       const gasalx_nv_quals *quals, uint32_t band_len, uint32_t n_pairs,
                                       const gasalx_nv_strings *dev_patterns, const gasalx_nv_strings *dev_texts,
                                       int32_t *dev_scores, uint32_t *dev_sinks, uint32_t max_pattern_len,
                                       void *stream);   /* max_pattern_len: 0 = read back */
int gasalx_nv_banded_qual_score_host(gasalx_engine *eng, const gasalx_nv_aligner *aligner,
                                     const gasalx_nv_quals *quals, uint32_t band_len, uint32_t n_pairs,
                                     const gasalx_nv_strings *patterns, uint64_t pattern_words,
                                     const gasalx_nv_strings *texts, uint64_t text_words, int32_t *scores,
                                     uint32_t *sinks);
int gasalx_nv_banded_qual_traceback_device(gasalx_engine *eng, const gasalx_nv_aligner *aligner,
                                           const gasalx_nv_quals *quals, uint32_t band, uint32_t n_pairs,
                                           const gasalx_nv_strings *dev_patterns,
                                           const gasalx_nv_strings *dev_texts, uint32_t max_pattern_len,
                                           int32_t *dev_scores, uint32_t *dev_sources, uint32_t *dev_sinks,
                                           uint8_t *dev_ops, uint32_t ops_stride, uint32_t *dev_n_ops,
                                           void *stream);
int gasalx_nv_banded_qual_traceback_host(gasalx_engine *eng, const gasalx_nv_aligner *aligner,
                                         const gasalx_nv_quals *quals, uint32_t band, uint32_t n_pairs,
                                         const gasalx_nv_strings *patterns, uint64_t pattern_words,
                                         const gasalx_nv_strings *texts, uint64_t text_words, int32_t *scores,
                                         uint32_t *sources, uint32_t *sinks, uint8_t *ops, uint32_t ops_stride,
                                         uint32_t *n_ops);
/* The kernel such a call runs, or the code it would return (the checks above in their order; the
 * struct's quality bytes are not read and may be NULL).  The scorer (want_traceback 0):
 * "nvbio_banded16_qual_gotoh_<type>_b<8|16|32>_sink" (two pairs per lane) or
 * "nvbio_banded_qual_gotoh_<type>_b<8|16|32>_sink" (int32); max_pattern_len 0 takes the int32 kernel.
 * The traceback: "nvbio_banded_qual_traceback_gotoh_<type>_b<N>", N = 7, 15 or 31 for those band
 * lengths (exact-length instances), 8, 16 or 32 otherwise. */
int gasalx_nv_describe_banded_qual_plan(const gasalx_nv_aligner *aligner, const gasalx_nv_quals *quals,
                                        uint32_t band_len, uint32_t max_pattern_len, uint32_t text_bits,
                                        int want_traceback, char *buf, uint32_t buf_len);

/* Multi-GPU from one host process.  A group holds one engine per
 * entry of a device list (entries may repeat a device); a host batch is split into
 * contiguous ranges of pairs with equal cell counts (Σ ql·tl; gasalx_shard_bounds),
 * and one host thread per entry runs gasalx_align_host (or the PairHMM call) on its
 * range, writing into that range of the caller's result arrays.  The reference's
 * pattern is STAR's static split (Non-CDP/STAR/src/cuda-nw.cu:296-367: per-GPU
 * workload, cudaSetDevice, one stream per device, disjoint host result ranges);
 * GASAL2 itself exposes only gasal_set_device (interfaces.cpp:98-125).
 * GASALX_MULTI_RCCL: build an RCCL communicator over the list (ncclCommInitAll, when
 * the entries are distinct devices and librccl can be opened) for
 * gasalx_multi_allgather; otherwise that call uses peer copies. */
typedef struct gasalx_multi gasalx_multi;
enum { GASALX_MULTI_RCCL = 1 };

int gasalx_multi_create(const int *devices, int n_devices, uint32_t flags, gasalx_multi **out);
int gasalx_multi_destroy(gasalx_multi *m);
int gasalx_multi_info(const gasalx_multi *m, int *n_devices, int *uses_rccl);
/* The engine of entry `index` (owned by the group), e.g. for device-resident calls. */
int gasalx_multi_engine(gasalx_multi *m, int index, gasalx_engine **out);
/* Contiguous ranges [bounds[k], bounds[k+1]) (world + 1 entries) balancing Σ a[i]·b[i]:
 * boundary k is one past the first pair whose prefix sum reaches k/world of the total. */
int gasalx_shard_bounds(const uint32_t *a, const uint32_t *b, uint32_t n, int world, uint32_t *bounds);
/* Host arrays in and out, as gasalx_align_host.  WITH_TB: the shards' query byte ranges
 * must not overlap (each pair's CIGAR lands at its query offset, get_tb.h:94). */
int gasalx_multi_align_host(gasalx_multi *m, const gasalx_params *params, const gasalx_batch *host_batch,
                            const gasalx_results *host_out);
int gasalx_multi_pairhmm_host(gasalx_multi *m, const gasalx_hmm_batch *host_batch, float *host_result);
int gasalx_multi_pairhmm_quals_host(gasalx_multi *m, const gasalx_hmm_qual_batch *host_batch, float *host_result);
/* Device-resident shards (a batch already split over the entries' devices, as config 4's
 * 10 M reads would sit in HBM): entry i aligns batches[i] -- device arrays on its own device,
 * max_q_len / max_t_len set, or the lengths are read back -- into outs[i] on streams[i] (NULL:
 * the entry's engine stream), one host thread per entry.  gather (optional, NULL to skip): the
 * exchange step in the same call, every entry's aln_score (padded to gather_stride int32 per
 * entry: each aln_score buffer holds gather_stride entries) lands at gather[j] + i * gather_stride
 * on every entry j (gasalx_multi_allgather: RCCL when the group has a communicator, else peer
 * copies).  With streams given the call returns once the work is queued; with NULL it waits. */
int gasalx_multi_align_device(gasalx_multi *m, const gasalx_params *params, const gasalx_batch *batches,
                              const gasalx_results *outs, void *const *streams, int32_t *const *gather,
                              uint32_t gather_stride);
/* The same for PairHMM: entry i scores batches[i] into results[i] (float, gather_stride entries
 * when gathering), then the optional gather of the float results. */
int gasalx_multi_pairhmm_device(gasalx_multi *m, const gasalx_hmm_batch *batches, float *const *results,
                                void *const *streams, float *const *gather, uint32_t gather_stride);
/* The exchange step: entry i's `bytes` at send[i] (device memory of its device) land at
 * recv[j] + i * bytes on every entry j.  streams: one hipStream_t per entry (the call
 * is then asynchronous), or NULL for the engines' streams and a synchronous call. */
int gasalx_multi_allgather(gasalx_multi *m, const void *const *send, void *const *recv, uint64_t bytes,
                           void *const *streams);

/* Synthetic workloads of SURVEY.md §8(d) (benchmark/test data, std::mt19937_64).
 * Writes a GASAL2-layout batch (N_CODE padding) into caller buffers sized by
 * gasalx_synth_sizes.  kind: 1..4 = configs 1..4.  Pairs come in blocks of 65,536,
 * each from its own seeded generator (block 0: `seed` itself), so
 * gasalx_synth_range can write pairs [start, start + n) of a larger batch on
 * their own (one rank's shard); offsets then start at 0. */
int gasalx_synth_sizes(int kind, uint32_t n_pairs, uint64_t *q_bytes, uint64_t *t_bytes);
int gasalx_synth_spec(int kind, uint32_t *q_len, uint32_t *t_len);
int gasalx_synth_pairs(int kind, uint64_t seed, uint32_t n_pairs, uint8_t *q_batch, uint32_t *q_offsets,
                       uint32_t *q_lens, uint8_t *t_batch, uint32_t *t_offsets, uint32_t *t_lens);
int gasalx_synth_range(int kind, uint64_t seed, uint64_t start, uint32_t n_pairs, uint8_t *q_batch,
                       uint32_t *q_offsets, uint32_t *q_lens, uint8_t *t_batch, uint32_t *t_offsets,
                       uint32_t *t_lens);

#ifdef __cplusplus
}
#endif
#endif
