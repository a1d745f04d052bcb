// capi_host_check — the parts of the flat C API (csrc/capi.cpp) that run without a device, for a
// host sanitizer build: `make -C tools capi_host_check` compiles capi.cpp itself with
// -fsanitize=address,undefined into this program (the rest of the engine comes from libgasal.so).
// It creates no engine and touches no GPU; run it on the build host.  Exit status 0 = all checks held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gasalx.h"

static int fails = 0;
#define EXPECT(c)                                                              \
    do {                                                                       \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } \
    } while (0)

static bool null_arg(int rc) { return rc == GASALX_EINVAL && std::strstr(gasalx_last_error(), "null argument"); }

// the documented chunk rule, restated: budget / per pairs, at least one, at most n
static uint64_t chunk_of(uint64_t n, uint64_t budget, uint64_t per) {
    uint64_t c = budget / (per ? per : 1);
    if (c > n) c = n;
    return c ? c : 1;
}

int main() {
    // gasalx_pairhmm_params: heap arrays of exactly n entries, quality bytes over the whole range
    {
        const uint32_t n = 257;
        std::vector<uint8_t> bq(n), iq(n), dq(n);
        for (uint32_t k = 0; k < n; k++) { bq[k] = (uint8_t)k; iq[k] = (uint8_t)(255 - k); dq[k] = (uint8_t)(3 * k); }
        std::vector<float> qm(n), de(n), xi(n), al(n);
        EXPECT(gasalx_pairhmm_params(bq.data(), iq.data(), dq.data(), n, qm.data(), de.data(), xi.data(), al.data()) == GASALX_OK);
        EXPECT(qm[0] == 1.0f && qm[128] == 1.0f && qm[10] == qm[138] && qm[10] > 0.0999f && qm[10] < 0.1001f);
        EXPECT(gasalx_pairhmm_params(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == GASALX_OK);
        EXPECT(gasalx_pairhmm_params(nullptr, iq.data(), dq.data(), 1, qm.data(), de.data(), xi.data(), al.data()) == GASALX_EINVAL);
    }
    // the traceback workspace sizes under GASALX_NV_TB_BUDGET: unset, unusable values (4 GiB), real budgets
    {
        const uint64_t dflt = 4ull << 30;
        const struct { const char *env; uint64_t budget; } budgets[] = {
            {nullptr, dflt}, {"", dflt}, {"0", dflt}, {"12x", dflt}, {"-5", dflt}, {"99999999999999999999999", dflt},
            {"1", 1}, {"4096", 4096}, {"1000000", 1000000}, {"18446744073709551615", ~0ull}};
        const uint32_t shapes[][3] = {{0, 0, 0}, {1, 1, 1}, {150, 182, 1}, {150, 182, 203}, {4096, 4096, 7}, {100, 120, 1000000}};
        for (const auto &b : budgets) {
            if (b.env) setenv("GASALX_NV_TB_BUDGET", b.env, 1); else unsetenv("GASALX_NV_TB_BUDGET");
            for (const auto &s : shapes) {
                const uint64_t p = s[0], t = s[1], n = s[2];
                const uint64_t per = (p + 7) / 8 * 8 * t + t * 8;
                EXPECT(gasalx_nv_traceback_workspace(s[0], s[1], s[2]) == per * chunk_of(n, b.budget, per) + 128);
                for (uint32_t band : {2u, 15u, 16u, 32u}) {
                    const uint64_t bper = p * ((band + 3) / 4 * 4);
                    EXPECT(gasalx_nv_banded_traceback_workspace(s[0], band, s[2]) == bper * chunk_of(n, b.budget, bper) + 64);
                }
            }
        }
        unsetenv("GASALX_NV_TB_BUDGET");
    }
    // gasalx_describe_plan / gasalx_nv_describe_plan: every algorithm, a buffer that fits and one byte
    {
        gasalx_params p = {1, 4, 6, 1, 0, 0, 0, 2, 2, 16, 0, 0x4E, 0, 0, 0};
        for (int algo = 0; algo <= 6; algo++)
            for (int start = 0; start <= 2; start++) {
                p.algo = algo; p.start_pos = start;
                char big[128];
                EXPECT(gasalx_describe_plan(&p, 150, 182, big, sizeof(big)) == GASALX_OK);
                std::vector<char> exact(std::strlen(big) + 1), one(1);
                EXPECT(gasalx_describe_plan(&p, 150, 182, exact.data(), (uint32_t)exact.size()) == GASALX_OK);
                EXPECT(std::strcmp(exact.data(), big) == 0);
                EXPECT(gasalx_describe_plan(&p, 150, 182, one.data(), 1) == GASALX_OK && one[0] == 0);
            }
        char buf[128];
        for (int bad = 0; bad < 5; bad++) {
            gasalx_params q = p;
            q.algo = 3; q.start_pos = 0;
            if (bad == 0) q.algo = 7;
            if (bad == 1) q.algo = -1;
            if (bad == 2) q.start_pos = 3;
            if (bad == 3) q.head = 4;
            if (bad == 4) q.tail = 4;
            EXPECT(gasalx_describe_plan(&q, 150, 182, buf, sizeof(buf)) == GASALX_EINVAL);
        }
        EXPECT(gasalx_describe_plan(nullptr, 1, 1, buf, sizeof(buf)) == GASALX_EINVAL);
        EXPECT(gasalx_describe_plan(&p, 1, 1, nullptr, 8) == GASALX_EINVAL);
        EXPECT(gasalx_describe_plan(&p, 1, 1, buf, 0) == GASALX_EINVAL);
        gasalx_nv_aligner al = {GASALX_NV_GOTOH, GASALX_NV_LOCAL, 2, -1, -2, -1, 0, 0};
        EXPECT(gasalx_nv_describe_plan(&al, 150, 182, 1, 2, buf, sizeof(buf)) == GASALX_OK && buf[0]);
        std::vector<char> exact(std::strlen(buf) + 1);
        EXPECT(gasalx_nv_describe_plan(&al, 150, 182, 1, 2, exact.data(), (uint32_t)exact.size()) == GASALX_OK);
        EXPECT(null_arg(gasalx_nv_describe_plan(nullptr, 1, 1, 0, 2, buf, sizeof(buf))));
        EXPECT(null_arg(gasalx_nv_describe_plan(&al, 1, 1, 0, 2, buf, 0)));
        EXPECT(null_arg(gasalx_nv_describe_plan(&al, 1, 1, 0, 2, nullptr, 8)));
    }
    // the other four gasalx_nv_describe_*_plan: NULL aligner (where there is one) and buffer, no room, a
    // buffer that fits exactly and one byte, and what the three that can refuse do refuse, with its text
    {
        const gasalx_nv_aligner al = {GASALX_NV_GOTOH, GASALX_NV_LOCAL, 2, -1, -2, -1, 0, 0};
        const gasalx_nv_aligner sw = {GASALX_NV_SW, GASALX_NV_LOCAL, 2, -1, 0, 0, -1, -1};
        const gasalx_nv_aligner type3 = {GASALX_NV_GOTOH, 3, 2, -1, -2, -1, 0, 0};
        char buf[128];
        auto refused = [](int rc, int want, const char *text) { return rc == want && std::strstr(gasalx_last_error(), text); };
        auto fits = [&](auto describe) {   // describe(buffer, length): OK into 128 bytes, into the exact size, into one byte
            EXPECT(describe(buf, (uint32_t)sizeof(buf)) == GASALX_OK && buf[0]);
            std::vector<char> exact(std::strlen(buf) + 1), one(1, 'x');
            EXPECT(describe(exact.data(), (uint32_t)exact.size()) == GASALX_OK && std::strcmp(exact.data(), buf) == 0);
            EXPECT(describe(one.data(), 1) == GASALX_OK && one[0] == 0);
            EXPECT(null_arg(describe(nullptr, 8)));
            EXPECT(null_arg(describe(buf, 0)));
        };
        fits([&](char *b, uint32_t len) { return gasalx_nv_describe_sinks_plan(&al, 150, 182, 1, 2, b, len); });
        EXPECT(null_arg(gasalx_nv_describe_sinks_plan(nullptr, 150, 182, 1, 2, buf, sizeof(buf))));

        fits([&](char *b, uint32_t len) { return gasalx_nv_describe_matrix_plan(&al, 24, 150, 182, 1, 1, b, len); });
        EXPECT(null_arg(gasalx_nv_describe_matrix_plan(nullptr, 24, 150, 182, 1, 1, buf, sizeof(buf))));
        EXPECT(gasalx_nv_describe_matrix_plan(&al, 24, 5000, 182, 1, 0, buf, sizeof(buf)) == GASALX_OK && !std::strcmp(buf, "none"));
        for (uint32_t bad : {0u, 1u, 33u})
            EXPECT(refused(gasalx_nv_describe_matrix_plan(&al, bad, 150, 182, 1, 0, buf, sizeof(buf)), GASALX_EINVAL,
                           "matrix size must be 2..32"));
        EXPECT(refused(gasalx_nv_describe_matrix_plan(&type3, 24, 150, 182, 1, 0, buf, sizeof(buf)), GASALX_EINVAL, "bad aligner"));
        EXPECT(refused(gasalx_nv_describe_matrix_plan(&sw, 24, 150, 182, 1, 0, buf, sizeof(buf)), GASALX_EUNSUPPORTED,
                       "only the Gotoh aligner takes a substitution matrix"));
        EXPECT(null_arg(gasalx_nv_describe_matrix_plan(&sw, 33, 150, 182, 1, 0, buf, 0)));   // the null test comes first

        fits([&](char *b, uint32_t len) { return gasalx_nv_describe_banded_sinks_plan(&al, 16, 150, 2, b, len); });
        EXPECT(null_arg(gasalx_nv_describe_banded_sinks_plan(nullptr, 16, 150, 2, buf, sizeof(buf))));
        for (uint32_t bad : {1u, 33u})
            EXPECT(refused(gasalx_nv_describe_banded_sinks_plan(&al, bad, 150, 2, buf, sizeof(buf)), GASALX_EINVAL,
                           "band length must be 2..32"));
        EXPECT(refused(gasalx_nv_describe_banded_sinks_plan(&al, 16, 150, 3, buf, sizeof(buf)), GASALX_EINVAL,
                       "symbol bits must be 2, 4 or 8"));
        EXPECT(null_arg(gasalx_nv_describe_banded_sinks_plan(&al, 33, 150, 2, buf, 0)));

        fits([&](char *b, uint32_t len) { return gasalx_nv_describe_myers_plan(GASALX_NV_SEMI_GLOBAL, 5, 31, b, len); });
        EXPECT(refused(gasalx_nv_describe_myers_plan(3, 4, 16, buf, sizeof(buf)), GASALX_EINVAL, "bad aligner"));
        EXPECT(refused(gasalx_nv_describe_myers_plan(GASALX_NV_GLOBAL, 4, 33, buf, sizeof(buf)), GASALX_EINVAL,
                       "band length must be 2..32"));
        EXPECT(refused(gasalx_nv_describe_myers_plan(GASALX_NV_GLOBAL, 3, 16, buf, sizeof(buf)), GASALX_EINVAL,
                       "alphabet size must be 2, 4 or 5"));
        EXPECT(refused(gasalx_nv_describe_myers_plan(GASALX_NV_LOCAL, 4, 16, buf, sizeof(buf)), GASALX_EUNSUPPORTED,
                       "banded Myers has no LOCAL form"));
        EXPECT(null_arg(gasalx_nv_describe_myers_plan(GASALX_NV_LOCAL, 4, 16, nullptr, 8)));
    }
    // every engine entry point without an engine
    {
        gasalx_params p = {1, 4, 6, 1, 3, 0, 0, 2, 2, 0, 0, 0x4E, 0, 0, 0};
        gasalx_batch b = {};
        gasalx_results r = {};
        gasalx_hmm_batch hb = {};
        gasalx_hmm_qual_batch qb = {};
        gasalx_nv_aligner al = {GASALX_NV_ED, 0, 0, 0, 0, 0, 0, 0};
        uint32_t w[2] = {0, 0}, off[2] = {0, 4};
        gasalx_nv_strings s = {w, off, 0, 2, 0};
        std::vector<double> d(4);
        std::vector<float> f(4);
        std::vector<int32_t> i32(4);
        std::vector<uint32_t> u32(8);
        std::vector<uint8_t> u8(64);
        uint32_t cnt = 7;
        uint64_t h = 9, t = 9;
        EXPECT(null_arg(gasalx_align_device(nullptr, &p, &b, &r, nullptr)));
        EXPECT(null_arg(gasalx_align_host(nullptr, &p, &b, &r)));
        EXPECT(null_arg(gasalx_pairhmm_device(nullptr, &hb, f.data(), nullptr)));
        EXPECT(null_arg(gasalx_pairhmm_host(nullptr, &hb, f.data())));
        EXPECT(null_arg(gasalx_pairhmm_quals_device(nullptr, &qb, f.data(), nullptr)));
        EXPECT(null_arg(gasalx_pairhmm_quals_host(nullptr, &qb, f.data())));
        EXPECT(null_arg(gasalx_pairhmm64_device(nullptr, &hb, d.data(), nullptr)));
        EXPECT(null_arg(gasalx_pairhmm64_host(nullptr, &hb, d.data())));
        EXPECT(null_arg(gasalx_pairhmm64_quals_device(nullptr, &qb, d.data(), nullptr)));
        EXPECT(null_arg(gasalx_pairhmm64_quals_host(nullptr, &qb, d.data())));
        EXPECT(null_arg(gasalx_pairhmm_log10_device(nullptr, &hb, 0.f, d.data(), u8.data(), nullptr)));
        EXPECT(null_arg(gasalx_pairhmm_log10_host(nullptr, &hb, 0.f, d.data(), u8.data(), &cnt)));
        EXPECT(null_arg(gasalx_pairhmm_quals_log10_device(nullptr, &qb, 0.f, d.data(), u8.data(), nullptr)));
        EXPECT(null_arg(gasalx_pairhmm_quals_log10_host(nullptr, &qb, 0.f, d.data(), u8.data(), &cnt)));
        EXPECT(cnt == 7);
        EXPECT(null_arg(gasalx_nv_score_device(nullptr, &al, 1, &s, &s, i32.data(), nullptr, 0, 0, nullptr)));
        EXPECT(null_arg(gasalx_nv_score_host(nullptr, &al, 1, &s, 1, &s, 1, i32.data(), nullptr)));
        EXPECT(null_arg(gasalx_nv_banded_score_device(nullptr, &al, 16, 1, &s, &s, i32.data(), 0, nullptr)));
        EXPECT(null_arg(gasalx_nv_banded_score_host(nullptr, &al, 16, 1, &s, 1, &s, 1, i32.data())));
        EXPECT(null_arg(gasalx_nv_traceback_device(nullptr, &al, 1, &s, &s, 0, 0, i32.data(), u32.data(), u32.data(),
                                                   u8.data(), 8, u32.data(), nullptr)));
        EXPECT(null_arg(gasalx_nv_traceback_host(nullptr, &al, 1, &s, 1, &s, 1, i32.data(), u32.data(), u32.data(),
                                                 u8.data(), 8, u32.data())));
        EXPECT(null_arg(gasalx_nv_banded_traceback_device(nullptr, &al, 16, 1, &s, &s, 0, i32.data(), u32.data(),
                                                          u32.data(), u8.data(), 24, u32.data(), nullptr)));
        EXPECT(null_arg(gasalx_nv_banded_traceback_host(nullptr, &al, 16, 1, &s, 1, &s, 1, i32.data(), u32.data(),
                                                        u32.data(), u8.data(), 24, u32.data())));
        const int8_t tab[4] = {1, -1, -1, 1};
        gasalx_nv_matrix m = {tab, 2};
        EXPECT(null_arg(gasalx_nv_score_sinks_device(nullptr, &al, 1, &s, &s, i32.data(), u32.data(), 0, 0, nullptr)));
        EXPECT(null_arg(gasalx_nv_score_sinks_host(nullptr, &al, 1, &s, 1, &s, 1, i32.data(), u32.data())));
        EXPECT(null_arg(gasalx_nv_matrix_score_device(nullptr, &al, &m, 1, &s, &s, i32.data(), u32.data(), 0, 0, nullptr)));
        EXPECT(null_arg(gasalx_nv_matrix_score_host(nullptr, &al, &m, 1, &s, 1, &s, 1, i32.data(), u32.data())));
        EXPECT(null_arg(gasalx_nv_banded_score_sinks_device(nullptr, &al, 16, 1, &s, &s, i32.data(), u32.data(), 0, nullptr)));
        EXPECT(null_arg(gasalx_nv_banded_score_sinks_host(nullptr, &al, 16, 1, &s, 1, &s, 1, i32.data(), u32.data())));
        EXPECT(null_arg(gasalx_nv_banded_myers_device(nullptr, GASALX_NV_GLOBAL, 4, 16, 1, &s, &s, i32.data(), u32.data(), 0,
                                                      nullptr)));
        EXPECT(null_arg(gasalx_nv_banded_myers_host(nullptr, GASALX_NV_GLOBAL, 4, 16, 1, &s, 1, &s, 1, i32.data(), u32.data())));
        EXPECT(null_arg(gasalx_nv_matrix_traceback_device(nullptr, &al, &m, 1, &s, &s, 0, 0, i32.data(), u32.data(), u32.data(),
                                                          u8.data(), 8, u32.data(), nullptr)));
        EXPECT(null_arg(gasalx_nv_matrix_traceback_host(nullptr, &al, &m, 1, &s, 1, &s, 1, i32.data(), u32.data(), u32.data(),
                                                        u8.data(), 8, u32.data())));
        EXPECT(gasalx_packed_pairs(nullptr, &h, &t) == GASALX_EINVAL && h == 9 && t == 9);
        EXPECT(gasalx_engine_create(0, nullptr) == GASALX_EINVAL);
        EXPECT(gasalx_engine_destroy(nullptr) == GASALX_OK);
        EXPECT(gasalx_host_alloc(16, nullptr) == GASALX_EINVAL);
        EXPECT(gasalx_host_free(nullptr) == GASALX_OK);
        EXPECT(gasalx_device_count(nullptr) == GASALX_EINVAL);
        EXPECT(gasalx_abi_version() == GASALX_ABI_VERSION);
    }
    std::printf(fails ? "capi_host_check: %d check(s) FAILED\n" : "capi_host_check: ok\n", fails);
    return fails ? 1 : 0;
}
