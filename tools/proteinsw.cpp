// proteinsw — protein Smith-Waterman through include/nvbio_batched.h: the four batch_alignment_score
// calls of nvbio's proteinsw example (LOCAL Gotoh with gaps -5 / -3 over n_strings pairs of a 128-symbol
// pattern and a 1024-symbol text, 8-bit concatenated string sets): a constant scheme and a 24 x 24
// substitution matrix, each under a PatternBlockingTag and a TextBlockingTag aligner.  A fifth step, which
// the example does not have, runs the matrix LOCAL traceback of the same batch (BatchedAlignmentTraceback
// over the matrix aligner), replays the first 16 alignments on the host and prints one of them.
//
// No BLOSUM table is shipped: the caller of the library supplies its own.  This tool scores with a
// seeded random symmetric table with entries in -4..11 (BLOSUM62's range); throughput does not depend
// on the values.  A few pairs of every call are checked against a host fill of the same recurrence.
//
//   proteinsw [n_strings = 50000] [n_tests = 10]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "nvbio_batched.h"

using namespace nvbio;

#define HIP_OK(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                            \
            exit(EXIT_FAILURE);                                                                \
        }                                                                                      \
    } while (0)

namespace {

const uint32 kSymbols = 24, kP = 128, kT = 1024;

template <class T>
T *to_device(const std::vector<T> &v) {
    T *d = nullptr;
    HIP_OK(hipMalloc(&d, v.size() * sizeof(T) + 16));
    HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

// LOCAL Gotoh score of one pair on the host, S(q, r) from the scheme: the check of the device scores
template <class Scheme>
int32 host_local_score(const Scheme &s, const uint8 *pat, uint32 m, const uint8 *txt, uint32 n) {
    const int32 go = s.pattern_gap_open(), ge = s.pattern_gap_extension(), inf = -(1 << 28);
    std::vector<int32> H(n + 1, 0), F(n + 1, inf);
    int32 best = 0;
    for (uint32 i = 0; i < m; ++i) {
        int32 diag = 0, left = 0, e = 0;
        for (uint32 c = 0; c < n; ++c) {
            F[c + 1] = std::max(F[c + 1] + ge, H[c + 1] + go);
            e = std::max(e + ge, left + go);
            const int32 h = std::max(std::max(0, diag + s.substitution(c, i, txt[c], pat[i])), std::max(e, F[c + 1]));
            diag = H[c + 1];
            H[c + 1] = left = h;
            best = std::max(best, h);
        }
    }
    return best;
}

// SimpleGotohScheme has no substitution(): the constant rule behind the same name
struct ConstantScheme : aln::SimpleGotohScheme {
    using aln::SimpleGotohScheme::SimpleGotohScheme;
    int32 substitution(uint32, uint32, uint8 r, uint8 q, uint8 = 0) const { return r == q ? match() : mismatch(); }
};

struct Batch {
    uint32 n;
    std::vector<uint8> pat, txt;
    uint8 *d_pat, *d_txt;
    uint32 *d_poff, *d_toff;
    int32 *d_scores;
    uint32 *d_sinks;
};

template <class Aligner, class Scheme, class Scheduler>
bool run(const char *label, const Aligner &aligner, const Scheme &check, const Batch &b, bool want_sinks, Scheduler sched,
         uint32 n_tests) {
    const aln::BestSinks out = {b.d_scores, want_sinks ? b.d_sinks : nullptr};
    auto call = [&] {
        aln::batch_alignment_score(aligner, make_concatenated_string_set(b.n, b.d_pat, b.d_poff),
                                   make_concatenated_string_set(b.n, b.d_txt, b.d_toff), out, sched, kP, kT);
    };
    call();   // warm-up: the first launch loads the code object
    HIP_OK(hipDeviceSynchronize());
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32 i = 0; i < n_tests; ++i) call();
    HIP_OK(hipDeviceSynchronize());
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("  GCUPS (%s): %.1f\n", label, 1.0e-9 * double(kP) * double(kT) * double(b.n) * double(n_tests) / sec);

    std::vector<int32> scores(b.n);
    HIP_OK(hipMemcpy(scores.data(), b.d_scores, (size_t)b.n * 4, hipMemcpyDeviceToHost));
    std::vector<uint32> sinks(2 * (size_t)b.n);
    if (want_sinks) HIP_OK(hipMemcpy(sinks.data(), b.d_sinks, sinks.size() * 4, hipMemcpyDeviceToHost));
    bool ok = true;
    const uint32 step = std::max<uint32>(1, b.n / 16);
    for (uint32 k = 0; k < b.n; k += step) {
        const int32 want = host_local_score(check, &b.pat[(size_t)k * kP], kP, &b.txt[(size_t)k * kT], kT);
        if (scores[k] != want) { fprintf(stderr, "%s: pair %u scores %d, host %d\n", label, k, scores[k], want); ok = false; }
        if (want_sinks && (sinks[2 * k] < 1 || sinks[2 * k] > kT || sinks[2 * k + 1] < 1 || sinks[2 * k + 1] > kP)) {
            fprintf(stderr, "%s: pair %u sink (%u, %u) outside the pair\n", label, k, sinks[2 * k], sinks[2 * k + 1]);
            ok = false;
        }
    }
    return ok;
}

// The fifth step: the matrix LOCAL traceback of the batch through BatchedAlignmentTraceback.  The first
// 16 alignments are replayed on the host from sink to source (a run of L equal gap ops costs
// gap_open + gap_ext * (L - 1); the spans must be the reported ones) and their scores printed beside the
// returned ones; the first is printed as pattern, marks and text.
bool run_traceback(const aln::SubstitutionMatrixScheme &scheme, const Batch &b) {
    typedef aln::GotohAligner<aln::LOCAL, aln::SubstitutionMatrixScheme> aligner_type;
    typedef aln::TracebackStream<aligner_type> stream_type;
    const uint32 stride = kP + kT;
    uint32 *d_sources, *d_n_ops;
    uint8 *d_ops;
    HIP_OK(hipMalloc(&d_sources, (size_t)b.n * 8));
    HIP_OK(hipMalloc(&d_n_ops, (size_t)b.n * 4));
    HIP_OK(hipMalloc(&d_ops, (size_t)b.n * stride));
    stream_type s(aligner_type(scheme), b.n, b.d_poff, reinterpret_cast<const uint32 *>(b.d_pat), kP, b.n * kP,
                  reinterpret_cast<const uint32 *>(b.d_txt), 0, b.d_scores, d_sources, b.d_sinks, d_ops, stride, d_n_ops);
    s.m_text_offsets = b.d_toff; s.m_max_text_len = kT;
    s.m_pattern_bits = 8; s.m_pattern_big_endian = 0; s.m_text_bits = 8; s.m_text_big_endian = 0;
    aln::BatchedAlignmentTraceback<0, stream_type> batch;
    const auto t0 = std::chrono::steady_clock::now();
    batch.enact(s);
    HIP_OK(hipDeviceSynchronize());
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("  traceback (Matrix/P): %.1f GCUPS, %.3f s, workspace %.1f MB\n",
           1.0e-9 * double(kP) * double(kT) * double(b.n) / sec, sec,
           1.0e-6 * double(aln::BatchedAlignmentTraceback<0, stream_type>::max_temp_storage(kP, kT, b.n)));

    const uint32 n_check = std::min<uint32>(16, b.n);
    std::vector<int32> scores(n_check);
    std::vector<uint32> sources(2 * n_check), sinks(2 * n_check), n_ops(n_check);
    std::vector<uint8> ops((size_t)n_check * stride);
    HIP_OK(hipMemcpy(scores.data(), b.d_scores, n_check * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(sources.data(), d_sources, n_check * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(sinks.data(), b.d_sinks, n_check * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(n_ops.data(), d_n_ops, n_check * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ops.data(), d_ops, ops.size(), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_sources)); HIP_OK(hipFree(d_n_ops)); HIP_OK(hipFree(d_ops));

    static const char letters[] = "ARNDCQEGHILKMFPSTWYVBZX*";
    const int32 go = scheme.pattern_gap_open(), ge = scheme.pattern_gap_extension();
    uint32 equal = 0;
    std::string line_p, line_m, line_t;
    for (uint32 k = 0; k < n_check; ++k) {
        const uint8 *pat = &b.pat[(size_t)k * kP], *txt = &b.txt[(size_t)k * kT];
        uint32 x = sinks[2 * k], y = sinks[2 * k + 1];
        bool inside = x <= kT && y <= kP && n_ops[k] <= stride;
        int32 total = 0;
        uint8 prev = aln::SUBSTITUTION;
        for (uint32 i = 0; inside && i < n_ops[k]; ++i) {
            const uint8 op = ops[(size_t)k * stride + i];
            char cp = '-', ct = '-', cm = ' ';
            if (op == aln::SUBSTITUTION) {
                if (x == 0 || y == 0) { inside = false; break; }
                --x; --y;
                total += scheme.substitution(x, y, txt[x], pat[y]);
                cp = letters[pat[y]]; ct = letters[txt[x]]; cm = pat[y] == txt[x] ? '|' : '.';
            } else if (op == aln::INSERTION) {
                if (y == 0) { inside = false; break; }
                --y;
                total += prev == op ? ge : go;
                cp = letters[pat[y]];
            } else {
                if (x == 0) { inside = false; break; }
                --x;
                total += prev == op ? ge : go;
                ct = letters[txt[x]];
            }
            prev = op;
            if (k == 0) { line_p.insert(line_p.begin(), cp); line_m.insert(line_m.begin(), cm); line_t.insert(line_t.begin(), ct); }
        }
        const bool same = inside && x == sources[2 * k] && y == sources[2 * k + 1] && total == scores[k];
        equal += same;
        printf("  pair %2u: text %u..%u, pattern %u..%u, %u ops, score %d, replayed %d%s\n", k, sources[2 * k], sinks[2 * k],
               sources[2 * k + 1], sinks[2 * k + 1], n_ops[k], scores[k], total, same ? "" : "  MISMATCH");
    }
    printf("  pair 0:\n    %s\n    %s\n    %s\n", line_p.c_str(), line_m.c_str(), line_t.c_str());
    printf("  replays equal: %u of %u\n", equal, n_check);
    return equal == n_check;
}

}  // namespace

int main(int argc, char **argv) {
    const uint32 n_strings = argc > 1 ? (uint32)atoi(argv[1]) : 50000u;
    const uint32 n_tests = argc > 2 ? (uint32)atoi(argv[2]) : 10u;
    if (n_strings == 0 || n_tests == 0 || (uint64)n_strings * kT > 0xFFFFFFFFull) {
        fprintf(stderr, "usage: proteinsw [n_strings] [n_tests]\n");
        return 2;
    }
    fprintf(stderr, "protein SW... started (%u pairs of %u x %u)\n", n_strings, kP, kT);

    std::mt19937 rng(0x5EED1024);
    std::vector<int8_t> table(kSymbols * kSymbols);
    for (uint32 q = 0; q < kSymbols; ++q)
        for (uint32 r = q; r < kSymbols; ++r)
            table[r + q * kSymbols] = table[q + r * kSymbols] = (int8_t)((int)(rng() % 16) - 4);   // -4..11, symmetric

    Batch b;
    b.n = n_strings;
    b.pat.resize((size_t)n_strings * kP);
    b.txt.resize((size_t)n_strings * kT);
    for (auto &c : b.pat) c = (uint8)(rng() % kSymbols);
    for (auto &c : b.txt) c = (uint8)(rng() % kSymbols);
    std::vector<uint32> poff(n_strings + 1), toff(n_strings + 1);
    for (uint32 k = 0; k <= n_strings; ++k) { poff[k] = k * kP; toff[k] = k * kT; }
    b.d_pat = to_device(b.pat); b.d_txt = to_device(b.txt);
    b.d_poff = to_device(poff); b.d_toff = to_device(toff);
    HIP_OK(hipMalloc(&b.d_scores, (size_t)n_strings * 4));
    HIP_OK(hipMalloc(&b.d_sinks, (size_t)n_strings * 8));

    bool ok = true;
    {
        const ConstantScheme check(1, -1, -5, -3);
        const aln::SimpleGotohScheme scoring(1, -1, -5, -3);
        ok &= run("Constant/P", aln::make_gotoh_aligner<aln::LOCAL, aln::PatternBlockingTag>(scoring), check, b, false,
                  aln::DeviceThreadScheduler(), n_tests);
        ok &= run("Constant/T", aln::make_gotoh_aligner<aln::LOCAL, aln::TextBlockingTag>(scoring), check, b, true,
                  aln::DeviceThreadScheduler(), n_tests);
    }
    {
        const aln::SubstitutionMatrixScheme scoring(table.data(), kSymbols, -5, -3);
        ok &= run("Matrix/P", aln::make_gotoh_aligner<aln::LOCAL, aln::PatternBlockingTag>(scoring), scoring, b, false,
                  aln::DeviceThreadBlockScheduler<128, 1>(), n_tests);
        ok &= run("Matrix/T", aln::make_gotoh_aligner<aln::LOCAL, aln::TextBlockingTag>(scoring), scoring, b, true,
                  aln::DeviceThreadBlockScheduler<128, 1>(), n_tests);
        ok &= run_traceback(scoring, b);
    }
    HIP_OK(hipFree(b.d_pat)); HIP_OK(hipFree(b.d_txt)); HIP_OK(hipFree(b.d_poff)); HIP_OK(hipFree(b.d_toff));
    HIP_OK(hipFree(b.d_scores)); HIP_OK(hipFree(b.d_sinks));
    if (!ok) { fprintf(stderr, "proteinsw: FAILED\n"); return 1; }
    fprintf(stderr, "protein SW... done\n");
    return 0;
}
