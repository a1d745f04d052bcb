// nvbio_myers_test — a client of include/nvbio_batched.h alone that makes qmap's alignment call
// (NvB/examples/qmap/qmap.cu:285-293): batch_banded_alignment_score<31> with
// make_edit_distance_aligner<SEMI_GLOBAL, MyersTag<5>>() over read and genome infix sets, into a
// vector of best sinks.  The data are generated: reads of 50..150 DNA_N symbols cut from a genome
// window of read length + 31 symbols, with substitutions (N among them) and the odd missing symbol,
// 4-bit big-endian reads against a 2-bit little-endian genome as sw-benchmark packs them (genome N
// stored as 0).  Prints "k score x y" per pair for tests/test_gpu_nvbio_myers.py, which builds the
// same data from the same generator.
//
// usage: nvbio_myers_test [n_pairs [seed]]
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

static const uint32 BAND_LEN = 31;
typedef MyersTag<5u> myers_dna5_tag;

// the generator the test restates: a 32-bit LCG, the top 16 bits of each step
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

int main(int argc, char **argv) {
    const uint32 n = argc > 1 ? (uint32)atoi(argv[1]) : 200u;
    lcg_state = argc > 2 ? (uint32)strtoul(argv[2], nullptr, 0) : 0x51A9u;
    std::vector<uint32> rw, gw, roff(1, 0u), goff(1, 0u);
    uint64 rn = 0, gn = 0;
    uint32 max_read_len = 0;
    for (uint32 k = 0; k < n; ++k) {
        const uint32 len = 50 + lcg() % 101, start = lcg() % 16;
        std::vector<uint32> genome(len + BAND_LEN);
        for (uint32 &g : genome) g = lcg() % 4;
        uint32 read_len = 0;
        for (uint32 i = 0; i < len; ++i) {
            const uint32 r = lcg() % 100;
            if (r == 0) continue;                                   // a symbol the read lacks
            const uint32 sym = r < 5 ? lcg() % 5 : genome[start + i];   // a substitution, N among them
            append(rw, rn, sym, 4, true);
            ++read_len;
        }
        for (uint32 g : genome) append(gw, gn, g, 2, false);
        roff.push_back((uint32)rn);
        goff.push_back((uint32)gn);
        if (read_len > max_read_len) max_read_len = read_len;
    }
    rw.push_back(0u);
    gw.push_back(0u);
    uint32 *d_rw = to_dev(rw), *d_gw = to_dev(gw), *d_roff = to_dev(roff), *d_goff = to_dev(goff);
    int32 *d_scores;
    uint32 *d_sinks;
    HIP_OK(hipMalloc(&d_scores, (size_t)n * 4 + 16));
    HIP_OK(hipMalloc(&d_sinks, (size_t)n * 8 + 16));

    const PackedStringSet read_infix_set(n, d_rw, d_roff, 4, 1), genome_infix_set(n, d_gw, d_goff, 2, 0);
    const BestSinks sinks = {d_scores, d_sinks};
    batch_banded_alignment_score<BAND_LEN>(make_edit_distance_aligner<SEMI_GLOBAL, myers_dna5_tag>(), read_infix_set,
                                           genome_infix_set, sinks, DeviceThreadScheduler(), max_read_len,
                                           max_read_len + BAND_LEN);
    HIP_OK(hipDeviceSynchronize());

    std::vector<int32> scores(n);
    std::vector<uint32> pos(2 * (size_t)n);
    HIP_OK(hipMemcpy(scores.data(), d_scores, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(pos.data(), d_sinks, (size_t)n * 8, hipMemcpyDeviceToHost));
    for (uint32 k = 0; k < n; ++k) printf("%u %d %u %u\n", k, scores[k], pos[2 * k], pos[2 * k + 1]);
    for (void *p : {(void *)d_rw, (void *)d_gw, (void *)d_roff, (void *)d_goff, (void *)d_scores, (void *)d_sinks})
        HIP_OK(hipFree(p));
    return 0;
}
