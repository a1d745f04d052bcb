// nvbio_banded_sinks_test — a client of include/nvbio_batched.h alone that uses the banded scorer
// the way nvBowtie does: batch_banded_alignment_score<15> with a Gotoh LOCAL aligner into a vector
// of best sinks (the end cell nvBowtie places its banded traceback by), then
// BatchedBandedAlignmentTraceback<15, ...> on the same pairs, whose own score pass finds the same
// BestSink.  The two must agree on the score and the sink of every pair.  The data are generated:
// reads of 50..150 DNA_N symbols cut from a genome window of read length + 15 symbols, with
// substitutions (N among them) and the odd missing symbol; every fourth read is a run of one
// three-symbol unit against a longer run of it, so that equal maxima occur and the last one must
// be the one kept; every eleventh genome window is one symbol shorter than its read (skipped).
// 4-bit big-endian reads against a 2-bit little-endian genome, as sw-benchmark packs them.
// Prints one summary line; exits 0 only when every pair agrees.
//
// usage: nvbio_banded_sinks_test [n_pairs [seed]]
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

int main(int argc, char **argv) {
    const uint32 n = argc > 1 ? (uint32)atoi(argv[1]) : 2000u;
    lcg_state = argc > 2 ? (uint32)strtoul(argv[2], nullptr, 0) : 0xB0A7u;
    std::vector<uint32> rw, gw, roff(1, 0u), goff(1, 0u);
    uint64 rn = 0, gn = 0;
    uint32 max_read_len = 0;
    for (uint32 k = 0; k < n; ++k) {
        const uint32 len = 50 + lcg() % 101;
        std::vector<uint32> read, genome;
        if (k % 4 == 3) {
            const uint32 unit[3] = {lcg() % 4, lcg() % 4, lcg() % 4};
            for (uint32 i = 0; i < len; ++i) read.push_back(unit[i % 3]);
            for (uint32 i = 0; i < len + 9; ++i) genome.push_back(unit[i % 3]);
        } else {
            const uint32 start = lcg() % 8;
            genome.resize(len + BAND_LEN);
            for (uint32 &g : genome) g = lcg() % 4;
            for (uint32 i = 0; i < len; ++i) {
                const uint32 r = lcg() % 100;
                if (r == 0) continue;                                        // a symbol the read lacks
                read.push_back(r < 5 ? lcg() % 5 : genome[start + i]);       // a substitution, N among them
            }
        }
        if (k % 11 == 10) genome.resize(read.size() - 1);
        for (uint32 s : read) append(rw, rn, s, 4, true);
        for (uint32 g : genome) append(gw, gn, g, 2, false);
        roff.push_back((uint32)rn);
        goff.push_back((uint32)gn);
        if (read.size() > max_read_len) max_read_len = (uint32)read.size();
    }
    rw.push_back(0u);
    gw.push_back(0u);
    uint32 *d_rw = to_dev(rw), *d_gw = to_dev(gw), *d_roff = to_dev(roff), *d_goff = to_dev(goff);

    typedef GotohAligner<LOCAL, SimpleGotohScheme> aligner_type;
    const aligner_type aligner = make_gotoh_aligner<LOCAL>(SimpleGotohScheme(2, -3, -5, -3));

    // 1. the banded scorer with a sink per pair
    int32 *d_scores;
    uint32 *d_sinks;
    HIP_OK(hipMalloc(&d_scores, (size_t)n * 4 + 16));
    HIP_OK(hipMalloc(&d_sinks, (size_t)n * 8 + 16));
    const PackedStringSet read_set(n, d_rw, d_roff, 4, 1), genome_set(n, d_gw, d_goff, 2, 0);
    const BestSinks best = {d_scores, d_sinks};
    batch_banded_alignment_score<BAND_LEN>(aligner, read_set, genome_set, best, DeviceThreadScheduler(), max_read_len,
                                           max_read_len + BAND_LEN);
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
    BatchedBandedAlignmentTraceback<BAND_LEN, 32, TracebackStream<aligner_type>> traceback;
    traceback.enact(stream);
    HIP_OK(hipDeviceSynchronize());

    const std::vector<int32> sc = to_host(d_scores, n), tsc = to_host(d_tscores, n);
    const std::vector<uint32> sk = to_host(d_sinks, 2 * (size_t)n), tsk = to_host(d_snk, 2 * (size_t)n);
    uint32 differ = 0, skipped = 0;
    for (uint32 k = 0; k < n; ++k) {
        const bool same = sc[k] == tsc[k] && sk[2 * k] == tsk[2 * k] && sk[2 * k + 1] == tsk[2 * k + 1];
        if (!same && differ++ < 5)
            fprintf(stderr, "pair %u: scorer %d (%u, %u), traceback %d (%u, %u)\n", k, sc[k], sk[2 * k], sk[2 * k + 1],
                    tsc[k], tsk[2 * k], tsk[2 * k + 1]);
        skipped += sc[k] == INT32_MIN;
    }
    printf("banded sinks: %u pairs, band %u, gotoh local: %u differ from the banded traceback (%u skipped pairs)\n", n,
           BAND_LEN, differ, skipped);
    for (void *p : {(void *)d_rw, (void *)d_gw, (void *)d_roff, (void *)d_goff, (void *)d_scores, (void *)d_sinks,
                    (void *)d_tscores, (void *)d_src, (void *)d_snk, (void *)d_nops, (void *)d_ops})
        HIP_OK(hipFree(p));
    return differ ? 1 : 0;
}
