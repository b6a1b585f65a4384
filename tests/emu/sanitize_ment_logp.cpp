// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
// Log-density section of the sanitizer driver (mentflow_amd/csrc/ment_logp.hip).  tests/emu/build_sanitize.sh links every
// tests/emu/sanitize_*.cpp into tests/emu/sanitize_emu; main (in sanitize_main.cpp) knows nothing of this section, so it runs
// from the constructor of a namespace-scope object of this translation unit, before main, and prints its own marker (sound for
// the reasons given at the top of sanitize_swd_grad.cpp: nothing it reaches depends on another translation unit's dynamic
// initialisation).  It calls mf_ment_logprob on small synthetic inputs whose buffers have exactly the documented sizes: tables in
// LDS and beyond it, grad NULL and non-NULL, d = 1, 3 and 8, a point count that is no multiple of the workgroup, NaN / inf rows,
// points far outside every hull, zero slots with each prior, no points, and the refusals.
#include <cstring>

#include "sanitize_common.h"

static void logp_on(const Slots& s, int d, int kind) {
    const int64_t n = 300;                                   // two workgroups, the second with 44 lanes
    const float a = kind == 1 ? 1.5f : 3.0f;
    const float lognorm = kind == 1 ? -d * (std::log(a) + 0.9189385f) : -d * std::log(2.0f * a);
    std::vector<float> x((size_t)n * d);
    for (auto& v : x) v = 0.9f * nrand();
    for (int j = 0; j < d; ++j) x[(size_t)(n - 1) * d + j] = 25.0f;               // outside every hull
    x[(size_t)5 * d] = NAN;
    x[(size_t)6 * d + (d - 1)] = INFINITY;
    x[(size_t)7 * d] = -INFINITY;
    std::vector<float> logp(n, 0.0f), grad((size_t)n * d, 0.0f), only(n, 0.0f);
    CK(mf_ment_logprob(x.data(), n, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(), kind, a,
                       lognorm, logp.data(), grad.data(), nullptr));
    CK(mf_ment_logprob(x.data(), n, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(), kind, a,
                       lognorm, only.data(), nullptr, nullptr));
    check(memcmp(logp.data(), only.data(), n * sizeof(float)) == 0, "grad == NULL gives the same logp bits");
    if (s.n > 0 || kind == 1) check(std::isnan(logp[5]), "a NaN coordinate gives NaN");     // (no factor reads it otherwise)
    int64_t finite = 0;
    for (int64_t i = 0; i < n; ++i) {
        check(!(std::isinf(logp[i]) && logp[i] > 0.0f), "logp is never +inf");
        finite += std::isfinite(logp[i]) ? 1 : 0;
        for (int j = 0; j < d; ++j) {
            const float g = grad[(size_t)i * d + j];
            if (std::isnan(logp[i])) check(std::isnan(g), "NaN rows have NaN gradients");
            else if (std::isinf(logp[i])) check(g == 0.0f, "-inf rows have zero gradients");
            else check(!std::isnan(g), "finite rows have no NaN gradient");
        }
    }
    if (s.n == 0 && kind != 2) check(finite >= n - 3, "without slots only the NaN / inf rows are not finite");
    if (s.n > 0) check(std::isinf(logp[n - 1]), "a point outside every hull is outside the support");
}

// (external like sanitize_swd_grad: as a static function it is inlined into the dynamic initialiser below, whose string constants
// ASan then registers at unaligned addresses and refuses)
void sanitize_ment_logp() {
    seed(4242u);
    for (int d = 1; d <= 8; d += d == 1 ? 2 : 5) {               // d = 1, 3, 8
        std::vector<int> small(3, 1);                              // 1-D slots; with d > 1 two 2-D slots join them
        if (d > 1) small.insert(small.begin() + 1, 2), small.push_back(2);
        for (int kind = 0; kind < 3; ++kind) {
            logp_on(make_slots(d, small, 12), d, kind);            // tables in LDS
            logp_on(make_slots(d, std::vector<int>(), 4), d, kind);   // zero slots: the prior alone
        }
        if (d > 1) logp_on(make_slots(d, std::vector<int>(2, 2), 85), d, 1);   // 2 x 85^2 floats: tables read from global memory
        else logp_on(make_slots(d, std::vector<int>(130, 1), 85), d, 1);   // 130 x 85 floats: beyond the LDS budget in 1-D
        logp_on(make_slots(d, std::vector<int>(40, 1), 8), d, 0);  // 40 slots: the running product is renormalised twice
    }
    // no points: nothing to do; refusals: no launch, an error instead
    Slots s = make_slots(3, std::vector<int>(1, 1), 8);
    std::vector<float> x(3 * 8, 0.1f), logp(8), grad(3 * 8);
    CK(mf_ment_logprob(x.data(), 0, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, logp.data(), grad.data(),
                       nullptr));
    check(mf_ment_logprob(x.data(), 8, 9, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, logp.data(),
                          grad.data(), nullptr) != 0, "d = 9 refused");
    check(mf_ment_logprob(x.data(), -1, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, logp.data(),
                          grad.data(), nullptr) != 0, "negative n refused");
    check(mf_ment_logprob(x.data(), 8, 3, 513, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, logp.data(),
                          grad.data(), nullptr) != 0, "513 slots refused");
    check(mf_ment_logprob(x.data(), 8, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 3, 0.f, 0.f, logp.data(),
                          grad.data(), nullptr) != 0, "prior kind 3 refused");
    printf("SANITIZE MENT LOGP OK\n");
    fflush(stdout);
}

namespace {
struct MentLogpSection {
    MentLogpSection() { sanitize_ment_logp(); }
} ment_logp_section;
}  // namespace
