// nvbio_qual_test — a client of include/nvbio_batched.h alone that scores reads the way nvBowtie's
// end-to-end mode does: a Gotoh SEMI_GLOBAL aligner over nvBowtie's default scheme (match 0,
// mismatch penalty QualCost(2, 6) of the read symbol's base quality, read gaps 5 + 3 / 3:
// QualityGotohScheme::nvbowtie_default()), BatchedBandedAlignmentScore<15> with sinks over a stream
// that carries the qualities, then BatchedBandedAlignmentTraceback<15, ...> on the same pairs.
// Checked on the host: (1) score and sink agree between the two; (2) replaying each alignment's
// ops from its source to its sink under the scheme (quality-dependent substitutions, affine gaps)
// gives the reported score and consumes exactly the symbols between source and sink.
// The data are generated: reads of 50..150 DNA_N symbols cut from a genome window of read length +
// 15 symbols, substitutions (N among them, most of them at a low quality) and the odd missing
// symbol; qualities 2..41 with a tenth anywhere in 0..255; every eleventh window one symbol
// shorter than its read (skipped).  4-bit big-endian reads against a 2-bit little-endian genome.
// Prints one summary line; exits 0 only when every pair agrees and replays.
//
// usage: nvbio_qual_test [n_pairs [seed]]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nvbio_batched.h"

using namespace nvbio;
using namespace nvbio::aln;

#define HIP_OK(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                            \
            exit(2);                                                                           \
        }                                                                                      \
    } while (0)

static const uint32 BAND_LEN = 15;

static uint32 lcg_state;
static uint32 lcg() {
    lcg_state = lcg_state * 1664525u + 1013904223u;
    return lcg_state >> 16;
}

static void append(std::vector<uint32> &w, uint64 &n, uint32 sym, uint32 bits, bool big) {
    const uint32 per = 32 / bits, p = (uint32)(n % per), sh = big ? 32 - bits * (p + 1) : bits * p;
    if (n / per >= w.size()) w.push_back(0u);
    w[n / per] |= sym << sh;
    ++n;
}

template <typename T>
static T *to_dev(const std::vector<T> &v) {
    T *d = nullptr;
    HIP_OK(hipMalloc(&d, v.size() * sizeof(T) + 16));
    HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

template <typename T>
static std::vector<T> to_host(const T *d, size_t n) {
    std::vector<T> v(n);
    HIP_OK(hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
    return v;
}

// The score of the ops (push order: the alignment's end first) walked forwards from the source, and
// whether they end on the sink.  SEMI_GLOBAL: the walk starts at 0 in row zero.
static bool replay_score(const QualityGotohScheme &sc, const std::vector<uint32> &read, const std::vector<uint8> &qual,
                         const std::vector<uint32> &genome, const uint32 *src, const uint32 *snk, const uint8 *ops,
                         uint32 n_ops, int32 *score) {
    uint32 x = src[0], y = src[1];
    int32 s = 0;
    int prev = SUBSTITUTION;
    for (uint32 i = n_ops; i-- > 0;) {
        const int op = ops[i];
        if (op == SUBSTITUTION) {
            if (y >= read.size()) return false;
            const uint8 r = x < genome.size() ? (uint8)genome[x] : (uint8)255;
            s += sc.substitution(x, y, r, (uint8)read[y], qual[y]);
            ++x; ++y;
        } else {
            s += op == prev ? sc.pattern_gap_extension() : sc.pattern_gap_open();
            if (op == INSERTION) ++y; else ++x;   // a read symbol, or a genome symbol
        }
        prev = op;
    }
    *score = s;
    return x == snk[0] && y == snk[1];
}

int main(int argc, char **argv) {
    const uint32 n = argc > 1 ? (uint32)atoi(argv[1]) : 2000u;
    lcg_state = argc > 2 ? (uint32)strtoul(argv[2], nullptr, 0) : 0x9A15u;
    std::vector<uint32> rw, gw, roff(1, 0u), goff(1, 0u);
    std::vector<std::vector<uint32>> reads(n), genomes(n);
    std::vector<std::vector<uint8>> quals(n);
    std::vector<uint8> qflat;
    uint64 rn = 0, gn = 0;
    uint32 max_read_len = 0;
    for (uint32 k = 0; k < n; ++k) {
        const uint32 len = 50 + lcg() % 101;
        std::vector<uint32> &read = reads[k], &genome = genomes[k];
        std::vector<uint8> &qual = quals[k];
        const uint32 start = lcg() % 8;
        genome.resize(len + BAND_LEN);
        for (uint32 &g : genome) g = lcg() % 4;
        for (uint32 i = 0; i < len; ++i) {
            const uint32 r = lcg() % 100;
            if (r == 0) continue;                                        // a symbol the read lacks
            const bool sub = r < 7;
            read.push_back(sub ? lcg() % 5 : genome[start + i]);         // a substitution, N among them
            const uint32 wide = lcg() % 10 == 0;
            qual.push_back((uint8)(wide ? lcg() % 256 : sub && lcg() % 4 ? lcg() % 12 : 2 + lcg() % 40));
        }
        if (k % 11 == 10) genome.resize(read.size() - 1);
        for (uint32 s : read) append(rw, rn, s, 4, true);
        for (uint32 g : genome) append(gw, gn, g, 2, false);
        qflat.insert(qflat.end(), qual.begin(), qual.end());
        roff.push_back((uint32)rn);
        goff.push_back((uint32)gn);
        if (read.size() > max_read_len) max_read_len = (uint32)read.size();
    }
    rw.push_back(0u);
    gw.push_back(0u);
    qflat.push_back(0);
    uint32 *d_rw = to_dev(rw), *d_gw = to_dev(gw), *d_roff = to_dev(roff), *d_goff = to_dev(goff);
    uint8 *d_quals = to_dev(qflat);

    typedef GotohAligner<SEMI_GLOBAL, QualityGotohScheme> aligner_type;
    const QualityGotohScheme scheme = QualityGotohScheme::nvbowtie_default();
    const aligner_type aligner = make_gotoh_aligner<SEMI_GLOBAL>(scheme);

    // 1. the banded scorer with a sink per pair
    int32 *d_scores;
    uint32 *d_sinks;
    HIP_OK(hipMalloc(&d_scores, (size_t)n * 4 + 16));
    HIP_OK(hipMalloc(&d_sinks, (size_t)n * 8 + 16));
    AlignmentStream<aligner_type> sstream(aligner, n, d_roff, d_rw, max_read_len, (uint32)rn, d_gw, 0, NULL);
    sstream.m_text_offsets = d_goff;
    sstream.m_scores32 = d_scores;
    sstream.m_sinks = d_sinks;
    sstream.set_quals(d_quals);
    BatchedBandedAlignmentScore<BAND_LEN, AlignmentStream<aligner_type>> scorer;
    scorer.enact(sstream);
    HIP_OK(hipDeviceSynchronize());

    // 2. the banded traceback of the same pairs
    const uint32 stride = 2 * max_read_len + BAND_LEN;
    int32 *d_tscores;
    uint32 *d_src, *d_snk, *d_nops;
    uint8 *d_ops;
    HIP_OK(hipMalloc(&d_tscores, (size_t)n * 4 + 16));
    HIP_OK(hipMalloc(&d_src, (size_t)n * 8 + 16));
    HIP_OK(hipMalloc(&d_snk, (size_t)n * 8 + 16));
    HIP_OK(hipMalloc(&d_nops, (size_t)n * 4 + 16));
    HIP_OK(hipMalloc(&d_ops, (size_t)n * stride + 16));
    TracebackStream<aligner_type> stream(aligner, n, d_roff, d_rw, max_read_len, (uint32)rn, d_gw, 0, d_tscores, d_src,
                                         d_snk, d_ops, stride, d_nops);
    stream.m_text_offsets = d_goff;
    stream.set_quals(d_quals);
    BatchedBandedAlignmentTraceback<BAND_LEN, 32, TracebackStream<aligner_type>> traceback;
    traceback.enact(stream);
    HIP_OK(hipDeviceSynchronize());

    const std::vector<int32> sc = to_host(d_scores, n), tsc = to_host(d_tscores, n);
    const std::vector<uint32> sk = to_host(d_sinks, 2 * (size_t)n), tsk = to_host(d_snk, 2 * (size_t)n);
    const std::vector<uint32> tsrc = to_host(d_src, 2 * (size_t)n), nops = to_host(d_nops, n);
    const std::vector<uint8> ops = to_host(d_ops, (size_t)n * stride);
    uint32 differ = 0, misreplayed = 0, skipped = 0;
    for (uint32 k = 0; k < n; ++k) {
        const bool same = sc[k] == tsc[k] && sk[2 * k] == tsk[2 * k] && sk[2 * k + 1] == tsk[2 * k + 1];
        if (!same && differ++ < 5)
            fprintf(stderr, "pair %u: scorer %d (%u, %u), traceback %d (%u, %u)\n", k, sc[k], sk[2 * k], sk[2 * k + 1],
                    tsc[k], tsk[2 * k], tsk[2 * k + 1]);
        if (tsc[k] == INT32_MIN) { ++skipped; continue; }
        int32 replayed = 0;
        const bool ends = replay_score(scheme, reads[k], quals[k], genomes[k], &tsrc[2 * k], &tsk[2 * k],
                                       &ops[(size_t)k * stride], nops[k], &replayed);
        if ((!ends || replayed != tsc[k]) && misreplayed++ < 5)
            fprintf(stderr, "pair %u: the ops replay to %d%s, reported %d\n", k, replayed, ends ? "" : " off the sink", tsc[k]);
    }
    printf("banded qualities: %u pairs, band %u, gotoh semi-global, nvBowtie's default scheme: %u differ from the banded "
           "traceback, %u replay to another score (%u skipped pairs)\n", n, BAND_LEN, differ, misreplayed, skipped);
    for (void *p : {(void *)d_rw, (void *)d_gw, (void *)d_roff, (void *)d_goff, (void *)d_quals, (void *)d_scores,
                    (void *)d_sinks, (void *)d_tscores, (void *)d_src, (void *)d_snk, (void *)d_nops, (void *)d_ops})
        HIP_OK(hipFree(p));
    return differ || misreplayed ? 1 : 0;
}
