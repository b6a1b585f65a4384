// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
// Sequential-Monte-Carlo section of the sanitizer driver (mentflow_amd/csrc/smc.hip).  tests/emu/build_sanitize.sh links every
// tests/emu/sanitize_*.cpp into tests/emu/sanitize_emu; main (in sanitize_main.cpp) knows nothing of this section, so it runs
// from the constructor of a namespace-scope object of this translation unit, before main, and prints its own marker (sound for
// the reasons given at the top of sanitize_swd_grad.cpp).  It calls mf_smc_resample on small synthetic inputs whose buffers have
// exactly the documented sizes: islands of S = 1, 2, 256, a ragged 257 and 1 500 chains (one and two elements per thread of the
// workgroup), 1, 3 and 8 islands, d = 1 .. 8 (rows copied as floats, float2 and float4), log-weights that are random, shifted
// by -5 000, partly -inf, NaN, equal, and all -inf in one island; every threshold side; u at and beyond both ends of [0, 1);
// and the refusals.  Any out-of-range index or undefined arithmetic aborts.
#include <cstring>

#include "sanitize_common.h"

struct SmcRun {
    std::vector<float> x, x_out;
    std::vector<double> logw, u, stats, scratch;
    std::vector<int32_t> ancestors;
};

static SmcRun make_run(int64_t S, int64_t groups, int d, int pattern) {
    SmcRun r;
    const int64_t chains = S * groups;
    r.x.resize((size_t)chains * d);
    for (float& v : r.x) v = nrand();
    r.x_out.assign((size_t)chains * d, NAN);
    r.logw.resize(chains);
    for (int64_t i = 0; i < chains; ++i) {
        double v = 3.0 * nrand();
        if (pattern == 1) v -= 5000.0;
        if (pattern == 2 && urand() < 0.25f) v = -INFINITY;
        if (pattern == 3) v = 0.7;
        if (pattern == 4 && i / S == groups - 1) v = -INFINITY;      // the last island has no weight at all
        r.logw[i] = v;
    }
    if (pattern == 2) r.logw[chains / 2] = NAN;
    r.u.resize(groups);
    for (double& v : r.u) v = urand();
    r.stats.assign((size_t)groups * 4, NAN);
    r.scratch.assign(chains, NAN);
    r.ancestors.assign(chains, -1);
    return r;
}

static int smc(SmcRun& r, int64_t chains, int d, int64_t groups, float threshold) {
    return mf_smc_resample(r.x.data(), r.x_out.data(), chains, d, groups, r.logw.data(), r.u.data(), threshold,
                           r.ancestors.data(), r.stats.data(), r.scratch.data(), nullptr);
}

static void smc_on(int64_t S, int64_t groups, int d, int pattern, float threshold) {
    const int64_t chains = S * groups;
    SmcRun r = make_run(S, groups, d, pattern);
    const std::vector<double> before = r.logw;
    CK(smc(r, chains, d, groups, threshold));
    for (int64_t g = 0; g < groups; ++g) {
        const double* st = &r.stats[(size_t)g * 4];
        const bool went = st[2] == 1.0;
        check(st[2] == 0.0 || st[2] == 1.0, "the resampled flag is 0 or 1");
        check(!std::isnan(st[0]) && !std::isnan(st[1]) && !std::isnan(st[3]), "no NaN in stats");
        check(st[1] >= 0.0 && st[1] <= (double)S * (1.0 + 1e-12), "0 <= ess <= S");
        int32_t last = -1;
        for (int64_t j = g * S; j < (g + 1) * S; ++j) {
            const int32_t a = r.ancestors[j];
            check(a >= g * S && a < (g + 1) * S, "a parent lies in its own island");
            check(a >= last, "parents do not decrease");
            last = a;
            check(memcmp(&r.x_out[(size_t)j * d], &r.x[(size_t)a * d], d * sizeof(float)) == 0, "x_out is x[parent]");
            if (went) {
                check(std::isfinite(before[a]), "a parent has weight > 0");
                check(r.logw[j] == st[0], "logw of a resampled island is its log mean weight");
            } else {
                check(a == j, "identity parents where an island does not resample");
                check(memcmp(&r.logw[j], &before[j], sizeof(double)) == 0, "and its logw bits are kept");
            }
        }
    }
}

// (external like sanitize_ais: as a static function it is inlined into the dynamic initialiser below, whose string constants
// ASan then registers at unaligned addresses and refuses)
void sanitize_smc() {
    seed(2026u);
    const int64_t sizes[] = {1, 2, 256, 257, 1500};
    const int64_t islands[] = {1, 3, 8};
    int turn = 0;
    for (int64_t S : sizes)
        for (int64_t groups : islands)
            for (int pattern = 0; pattern < 5; ++pattern, ++turn) {
                const int d = 1 + turn % 8;
                smc_on(S, groups, d, pattern, 1.1f);              // every island with weight resamples
                smc_on(S, groups, d, pattern, 0.5f);              // decided per island
                smc_on(S, groups, d, pattern, 0.0f);              // none does
            }
    smc_on(257, 3, 6, 0, NAN);                                    // a NaN threshold resamples nothing
    // u at and beyond both ends, and NaN: clamped
    const double ends[] = {0.0, 1.0 - 1.1102230246251565e-16, 1.0, -0.5, 3.0, NAN, INFINITY};
    for (double u0 : ends) {
        SmcRun r = make_run(257, 3, 6, 3);
        for (double& v : r.u) v = u0;
        CK(smc(r, 257 * 3, 6, 3, 1.1f));
        for (int64_t j = 0; j < 257 * 3; ++j) check(r.ancestors[j] == j, "equal weights: the identity for every u");
        r = make_run(257, 3, 5, 2);
        for (double& v : r.u) v = u0;
        CK(smc(r, 257 * 3, 5, 3, 1.1f));
        for (int64_t j = 0; j < 257 * 3; ++j) check(r.ancestors[j] >= 0 && r.ancestors[j] < 257 * 3, "parents in range");
    }
    // no chains: nothing to do; refusals: no launch, an error instead
    SmcRun r = make_run(8, 3, 3, 0);
    CK(smc(r, 0, 3, 3, 0.5f));
    check(smc(r, 24, 9, 3, 0.5f) != 0, "d = 9 refused");
    check(smc(r, 24, 0, 3, 0.5f) != 0, "d = 0 refused");
    check(smc(r, 24, 3, 5, 0.5f) != 0, "chains % groups != 0 refused");
    check(smc(r, 24, 3, 0, 0.5f) != 0, "groups = 0 refused");
    check(smc(r, -1, 3, 1, 0.5f) != 0, "a negative chain count refused");
    check(smc(r, (int64_t)3 << 30, 3, 3, 0.5f) != 0, "a chain count beyond the limit refused");
    check(mf_smc_resample(r.x.data(), r.x.data(), 24, 3, 3, r.logw.data(), r.u.data(), 0.5f, r.ancestors.data(), r.stats.data(),
                          r.scratch.data(), nullptr) != 0, "x_out == x refused");
    check(mf_smc_resample(r.x.data(), r.x_out.data(), 24, 3, 3, nullptr, r.u.data(), 0.5f, r.ancestors.data(), r.stats.data(),
                          r.scratch.data(), nullptr) != 0, "a null logw refused");
    check(mf_smc_resample(r.x.data(), r.x_out.data(), 24, 3, 3, r.logw.data(), nullptr, 0.5f, r.ancestors.data(), r.stats.data(),
                          r.scratch.data(), nullptr) != 0, "a null u refused");
    check(mf_smc_resample(r.x.data(), r.x_out.data(), 24, 3, 3, r.logw.data(), r.u.data(), 0.5f, r.ancestors.data(), r.stats.data(),
                          nullptr, nullptr) != 0, "a null scratch refused");
    for (float v : r.x_out) check(std::isnan(v), "a refused call writes nothing");
    for (int32_t v : r.ancestors) check(v == -1, "nor any parent");
    printf("SANITIZE SMC OK\n");
    fflush(stdout);
}

namespace {
struct SmcSection {
    SmcSection() { sanitize_smc(); }
} smc_section;
}  // namespace
