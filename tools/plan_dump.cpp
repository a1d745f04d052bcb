// plan_dump — every field of the Plan that gx::make_plan and gx::make_semi_cigar_plan give over a
// grid, one labelled line per row, for comparing two builds of the planner byte for byte (the plan
// names alone, tests/golden/plan_names.json, leave vmin, the LDS sizes, kf16, band_wd, the int32
// shape under a packed plan and everything that depends on n or has_ops unpinned).  No GPU needed.
//
// The grid is a superset of tests/test_capi.py's: its parameter sets, length pairs and switches with
// n = 0 and no ops; with no switch set, also each n of kPairs, has_ops, GASALX_GMIN, GASALX_TB_BAND_W
// and the score sets of kExtraScores; then the semi-CIGAR planner with HEAD = TAIL = TARGET over every
// score set and length pair, with and without GASALX_PACKED16=0.
//
// Links against libgasal.so (which exports both planners) or against csrc/plan.cpp alone: tools/Makefile
// plan_dump / plan_dump_host.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "engine.hpp"

namespace {

const uint32_t kLens[] = {8, 64, 150, 152, 182, 256, 257, 300, 512, 513, 1000, 4000};
const int kNoN = -1000000;   // "no N penalty" in a score set
struct Scores { int m, x, o, e, npen; };
const Scores kScores[] = {{1, 4, 6, 1, kNoN}, {2, 4, 6, 1, kNoN}, {3, 4, 6, 1, kNoN}, {1, 0, 6, 1, kNoN},
                          {2, -1, 4, 2, kNoN}, {1, 4, 6, 1, 2}, {1, 4, 6, 1, 6}};
const Scores kExtraScores[] = {{1, 1, 0, 1, kNoN}, {2, 3, 5, 2, kNoN}, {200, 56, 6, 1, kNoN}, {5, 250, 6, 1, kNoN},
                               {1, 4, 6, 0, kNoN}, {1, 4, 100, 50, kNoN}, {1, 4, 6, 1, -1}};
const char *kEnvs[] = {"", "GASALX_KF16=0", "GASALX_KSEG=0", "GASALX_KSEG=2", "GASALX_TB_BAND=0", "GASALX_PACKED16=0",
                       "GASALX_BAND16=0", "GASALX_LOCAL16=0"};
const char *kSwitches[] = {"GASALX_KF16", "GASALX_KSEG", "GASALX_TB_BAND", "GASALX_PACKED16", "GASALX_BAND16",
                           "GASALX_LOCAL16", "GASALX_GMIN", "GASALX_TB_BAND_W"};
const uint32_t kPairs[] = {1, 2000, 5000, 40000, 300000};
const int kSemi = 2, kBanded = 5, kTarget = 2;

// every length with itself, each neighbour in the list and 150, in both orientations, sorted
std::vector<std::pair<uint32_t, uint32_t>> length_pairs() {
    std::set<std::pair<uint32_t, uint32_t>> s;
    const int n = (int)(sizeof(kLens) / sizeof(kLens[0]));
    for (int i = 0; i < n; i++)
        for (uint32_t b : {kLens[i], kLens[std::max(i - 1, 0)], kLens[std::min(i + 1, n - 1)], 150u}) {
            s.insert({kLens[i], b});
            s.insert({b, kLens[i]});
        }
    return {s.begin(), s.end()};
}

void set_env(const char *assign) {
    for (const char *s : kSwitches) unsetenv(s);
    if (!*assign) return;
    const std::string a(assign);
    const size_t eq = a.find('=');
    setenv(a.substr(0, eq).c_str(), a.substr(eq + 1).c_str(), 1);
}

gasalx_params params(int algo, int start, int second, int head, int tail, const Scores &sc) {
    gasalx_params p = {};
    p.match = sc.m; p.mismatch = sc.x; p.gap_open = sc.o; p.gap_extend = sc.e;
    p.algo = algo; p.start_pos = start; p.second_best = second; p.head = head; p.tail = tail;
    p.k_band = algo == kBanded ? 16 : 0;
    p.n_code = 0x4E;
    p.has_n_penalty = sc.npen != kNoN;
    p.n_penalty = sc.npen != kNoN ? sc.npen : 0;
    return p;
}

long g_rows = 0;

void print_row(const char *what, const char *env, const gasalx_params &p, const gx::BatchShape &s, bool ops,
               const gx::Plan &pl, int rc, const std::string &why) {
    std::printf("%s env=%s algo=%d start=%d second=%d head=%d tail=%d scores=%d/%d/%d/%d/", what, *env ? env : "-",
                p.algo, p.start_pos, p.second_best, p.head, p.tail, p.match, p.mismatch, p.gap_open, p.gap_extend);
    if (p.has_n_penalty) std::printf("%d", p.n_penalty);
    else std::printf("-");
    std::printf(" q=%u t=%u n=%u ops=%d :", s.max_q, s.max_t, s.n, (int)ops);
    std::printf(" kind=%d wf_algo=%d keys=%d tb=%d packed16=%d key2=%d G16=%d R16=%d lds16_stride=%u lds16_bytes=%zu"
                " vmin=%d kf16=%u ku16=%d kseg_shift=%u G=%d R=%d lds_stride=%u lds_bytes=%zu need_pack=%d band16=%d"
                " local16=%d semi_tq=%d tb_band=%d band_w=%u band_wd=%u semi_tb=%d max_q=%u max_t=%u name=%s rc=%d"
                " why=%s\n",
                (int)pl.kind, pl.wf_algo, (int)pl.keys, (int)pl.tb, (int)pl.packed16, (int)pl.key2, pl.G16, pl.R16,
                pl.lds16_stride, pl.lds16_bytes, pl.vmin, pl.kf16, (int)pl.ku16, pl.kseg_shift, pl.G, pl.R,
                pl.lds_stride, pl.lds_bytes, (int)pl.need_pack, (int)pl.band16, (int)pl.local16, (int)pl.semi_tq,
                (int)pl.tb_band, pl.band_w, pl.band_wd, (int)pl.semi_tb, pl.max_q, pl.max_t, pl.name.c_str(), rc,
                why.empty() ? "-" : why.c_str());
    ++g_rows;
}

// make_plan over every parameter set x length pair x head of test_capi.py's grid, for the given scores
template <size_t N>
void plan_pass(const char *env, const Scores (&scores)[N], uint32_t n, bool ops) {
    static const auto pairs = length_pairs();
    set_env(env);
    for (int algo = 0; algo < 7; algo++)
        for (int start = 0; start < 3; start++)
            for (int second = 0; second < 2; second++)
                for (int tail = algo == kSemi ? 0 : kTarget; tail < (algo == kSemi ? 4 : kTarget + 1); tail++)
                    for (const Scores &sc : scores)
                        for (const auto &qt : pairs)
                            for (int head = algo == kSemi ? 0 : kTarget; head < (algo == kSemi ? 4 : kTarget + 1); head++) {
                                const gasalx_params p = params(algo, start, second, head, tail, sc);
                                gx::BatchShape s;
                                s.max_q = qt.first; s.max_t = qt.second; s.n = n;
                                print_row("plan", env, p, s, ops, gx::make_plan(p, s, ops), 0, "");
                            }
}

// heads: make_semi_cigar_plan as gasalx_semi_cigar_head_* calls it, over the four heads
template <size_t N>
void semi_cigar_pass(const char *env, const Scores (&scores)[N], bool heads = false) {
    static const auto pairs = length_pairs();
    set_env(env);
    for (const Scores &sc : scores)
        for (const auto &qt : pairs)
            for (int head = heads ? 0 : kTarget; head < (heads ? 4 : kTarget + 1); head++) {
                const gasalx_params p = params(kSemi, 0, 0, head, kTarget, sc);
                gx::BatchShape s;
                s.max_q = qt.first; s.max_t = qt.second;
                int rc = 0;
                std::string why;
                const gx::Plan pl = gx::make_semi_cigar_plan(p, s, false, &rc, &why, heads);
                print_row(heads ? "semi_cigar_head" : "semi_cigar", env, p, s, false, pl, rc, why);
            }
}

}  // namespace

int main() {
    for (const char *env : kEnvs) plan_pass(env, kScores, 0, false);
    for (uint32_t n : kPairs) plan_pass("", kScores, n, false);
    plan_pass("", kScores, 0, true);
    for (const char *env : {"GASALX_GMIN=8", "GASALX_GMIN=16", "GASALX_GMIN=32", "GASALX_GMIN=64", "GASALX_TB_BAND_W=0",
                            "GASALX_TB_BAND_W=10"})
        plan_pass(env, kScores, 0, false);
    plan_pass("", kExtraScores, 0, false);
    for (const char *env : {"", "GASALX_PACKED16=0"}) {
        semi_cigar_pass(env, kScores);
        semi_cigar_pass(env, kExtraScores);
    }
    // (after every earlier row, so that a dump of an older planner is a prefix of this one)
    for (const char *env : {"", "GASALX_PACKED16=0"}) {
        semi_cigar_pass(env, kScores, true);
        semi_cigar_pass(env, kExtraScores, true);
    }
    set_env("");
    std::fprintf(stderr, "%ld rows\n", g_rows);
    return 0;
}
