// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
// Annealed-importance-sampling section of the sanitizer driver (mentflow_amd/csrc/ais.hip).  tests/emu/build_sanitize.sh links
// every tests/emu/sanitize_*.cpp into tests/emu/sanitize_emu; main (in sanitize_main.cpp) knows nothing of this section, so it
// runs from the constructor of a namespace-scope object of this translation unit, before main, and prints its own marker (sound
// for the reasons given at the top of sanitize_swd_grad.cpp).  It calls mf_ais_ment_steps on small synthetic inputs whose buffers
// have exactly the documented sizes, on the slot shapes of sanitize_mala.cpp: tables in LDS and beyond it, d = 1 .. 8, zero
// slots, a chain count that is not a multiple of the workgroup, out and logp NULL and non-NULL, a ladder cut into launches,
// steps_per_temp = 0, repeated temperatures, NaN noise, a chain that starts outside every hull, drift_clip = 0, and the refusals.
// Any out-of-range index or undefined arithmetic aborts.
#include <cstring>

#include "sanitize_common.h"

struct AisRun {
    std::vector<float> x, noise, scale, out, logp, betas, mean, base;
    std::vector<double> logw;
    std::vector<int32_t> accepted;
};

static AisRun make_run(int64_t chains, int d, int64_t ntemps, int64_t spt, bool want_out) {
    AisRun r;
    const int64_t steps = ntemps * spt;
    r.mean.resize(d);
    r.base.resize(d);
    for (int j = 0; j < d; ++j) {
        r.mean[j] = 0.1f * (j % 2 ? -1.0f : 1.0f);
        r.base[j] = 0.8f + 0.05f * j;
    }
    r.x.resize((size_t)chains * d);
    for (size_t i = 0; i < r.x.size(); ++i) r.x[i] = r.mean[i % d] + r.base[i % d] * nrand();
    for (int j = 0; j < d; ++j) r.x[(size_t)(chains - 1) * d + j] = 25.0f;        // a chain that starts outside every hull
    r.noise.resize((size_t)steps * (d + 1) * chains);
    for (int64_t t = 0; t < steps; ++t)
        for (int a = 0; a <= d; ++a)
            for (int64_t c = 0; c < chains; ++c) r.noise[(size_t)((t * (d + 1) + a) * chains + c)] = a < d ? nrand() : urand();
    r.betas.resize(ntemps + 1);
    for (int64_t k = 0; k <= ntemps; ++k) r.betas[k] = (float)k / (float)(ntemps > 0 ? ntemps : 1);
    if (ntemps >= 4) {
        r.betas[1] = 0.0f;                                   // transitions on the base alone
        r.betas[3] = r.betas[2];                             // an increment of exactly 0
    }
    r.scale.assign(d, 0.3f);
    r.out.assign(want_out ? (size_t)steps * chains * d : 0, NAN);
    r.logp.assign(chains, NAN);
    r.logw.assign(chains, 0.0);
    r.accepted.assign(chains, 0);
    return r;
}

static int ais(const Slots& s, AisRun& r, int64_t chains, int d, int kind, float a, float lognorm, const float* noise,
               int64_t ntemps, int64_t temp_offset, int64_t spt, float clip, bool want_out, bool want_logp) {
    return mf_ais_ment_steps(r.x.data(), chains, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(),
                             kind, a, lognorm, noise, r.betas.data(), (int64_t)r.betas.size(), ntemps, temp_offset, spt,
                             r.scale.data(), clip, r.mean.data(), r.base.data(), r.logw.data(),
                             want_out ? r.out.data() : nullptr, r.accepted.data(), want_logp ? r.logp.data() : nullptr, nullptr);
}

static void ais_on(const Slots& s, int d, int kind, float clip) {
    const int64_t chains = 300, K = 6, spt = 2;              // two workgroups, the second with 44 lanes
    const float a = kind == 1 ? 1.5f : 3.0f;
    const float lognorm = kind == 1 ? -d * (std::log(a) + 0.9189385f) : -d * std::log(2.0f * a);
    // the whole ladder in one launch, every state and logp written
    AisRun r = make_run(chains, d, K, spt, true);
    r.noise[(size_t)((3 * (d + 1) + 0) * chains + 5)] = NAN;                      // chain 5 meets a NaN proposal at transition 3
    r.noise[(size_t)((4 * (d + 1) + d) * chains + 6)] = NAN;                      // chain 6 a NaN uniform at transition 4
    r.noise[(size_t)((2 * (d + 1) + 0) * chains + (chains - 1))] = NAN;           // the outside chain a NaN proposal
    AisRun q = r;                                            // the same run, cut in two launches below
    CK(ais(s, r, chains, d, kind, a, lognorm, r.noise.data(), K, 0, spt, clip, true, true));
    for (float v : r.out) check(std::isfinite(v), "every state is finite");
    for (int64_t c = 0; c < chains; ++c) {
        check(r.accepted[c] >= 0 && r.accepted[c] <= K * spt, "acceptance count in range");
        check(!std::isnan(r.logp[c]) && !(std::isinf(r.logp[c]) && r.logp[c] > 0.0f), "logp of a final state is finite or -inf");
        check(!std::isnan(r.logw[c]) && !(std::isinf(r.logw[c]) && r.logw[c] > 0.0), "logw is finite or -inf");
    }
    if (s.n > 0) check(std::isinf(r.logw[chains - 1]), "a start outside every hull has weight 0");
    // 2 + 4 temperatures; out NULL and logp NULL in the first launch
    const size_t cut = (size_t)2 * spt * (d + 1) * chains;
    CK(ais(s, q, chains, d, kind, a, lognorm, q.noise.data(), 2, 0, spt, clip, false, false));
    CK(ais(s, q, chains, d, kind, a, lognorm, q.noise.data() + cut, K - 2, 2, spt, clip, true, true));
    for (size_t i = 0; i < q.out.size(); ++i)
        check(i < (size_t)2 * spt * chains * d ? std::isnan(q.out[i]) : q.out[i] == r.out[i],
              "the second launch writes its own rows");
    check(memcmp(q.x.data(), r.x.data(), q.x.size() * sizeof(float)) == 0, "two launches give the states of one");
    check(memcmp(q.logw.data(), r.logw.data(), q.logw.size() * sizeof(double)) == 0, "and the same logw bits");
    check(memcmp(q.logp.data(), r.logp.data(), q.logp.size() * sizeof(float)) == 0, "and the same logp bits");
    check(memcmp(q.accepted.data(), r.accepted.data(), q.accepted.size() * sizeof(int32_t)) == 0, "and the same counts");
    // no moves at all: a zero-sized noise buffer, a zero-sized out
    AisRun n = make_run(chains, d, 1, 0, true);
    std::vector<float> x0 = n.x;
    CK(ais(s, n, chains, d, kind, a, lognorm, n.noise.data(), 1, 0, 0, clip, true, true));
    check(memcmp(n.x.data(), x0.data(), x0.size() * sizeof(float)) == 0, "plain importance sampling leaves x alone");
    // no temperatures: nothing happens
    CK(ais(s, n, chains, d, kind, a, lognorm, n.noise.data(), 0, 1, 0, clip, true, true));
    check(memcmp(n.x.data(), x0.data(), x0.size() * sizeof(float)) == 0, "no temperatures: x untouched");
}

// (external like sanitize_ment_logp: as a static function it is inlined into the dynamic initialiser below, whose string
// constants ASan then registers at unaligned addresses and refuses)
void sanitize_ais() {
    seed(2025u);
    for (int d = 1; d <= 8; ++d) {
        std::vector<int> small = d == 1 ? std::vector<int>{1, 1, 1} : std::vector<int>{1, 2, 1, 1, 2};
        ais_on(make_slots(d, small, 12), d, 1, 1.0f);             // tables in LDS, Gaussian prior
        if (d != 1 && d != 3 && d != 8) continue;                 // the other shapes at sanitize_mala.cpp's dimensions
        ais_on(make_slots(d, small, 12), d, 0, 0.0f);             // no prior, no drift
        ais_on(make_slots(d, {}, 4), d, 2, 1.0f);                 // zero slots: the uniform prior alone
        ais_on(make_slots(d, {}, 4), d, 1, 2.5f);                 // zero slots: the Gaussian prior alone, a wide clip
        if (d > 1) ais_on(make_slots(d, {2, 2}, 85), d, 0, 1.0f);   // 2 x 85^2 floats: tables read from global memory
        else ais_on(make_slots(d, std::vector<int>(130, 1), 85), d, 0, 1.0f);   // 130 x 85 floats: beyond the LDS budget in 1-D
    }
    // no chains: nothing to do; refusals: no launch, an error instead
    Slots s = make_slots(3, {1}, 8);
    AisRun r = make_run(8, 3, 4, 2, true);
    CK(ais(s, r, 0, 3, 0, 0.f, 0.f, r.noise.data(), 4, 0, 2, 1.f, true, true));
    check(ais(s, r, 8, 9, 0, 0.f, 0.f, r.noise.data(), 4, 0, 2, 1.f, true, true) != 0, "d = 9 refused");
    check(ais(s, r, 8, 3, 0, 0.f, 0.f, r.noise.data(), 4, 0, -1, 1.f, true, true) != 0, "negative steps_per_temp refused");
    check(ais(s, r, 8, 3, 0, 0.f, 0.f, r.noise.data(), -1, 0, 2, 1.f, true, true) != 0, "negative ntemps refused");
    check(ais(s, r, 8, 3, 0, 0.f, 0.f, r.noise.data(), 4, 1, 2, 1.f, true, true) != 0, "temperatures beyond the ladder refused");
    check(ais(s, r, -1, 3, 0, 0.f, 0.f, r.noise.data(), 4, 0, 2, 1.f, true, true) != 0, "a negative chain count refused");
    check(ais(s, r, 8, 3, 0, 0.f, 0.f, r.noise.data(), 4, 0, 2, -0.5f, true, true) != 0, "drift_clip < 0 refused");
    check(ais(s, r, 8, 3, 0, 0.f, 0.f, r.noise.data(), 4, 0, 2, NAN, true, true) != 0, "a NaN drift_clip refused");
    r.base[1] = 0.0f;
    check(ais(s, r, 8, 3, 0, 0.f, 0.f, r.noise.data(), 4, 0, 2, 1.f, true, true) != 0, "base_scale = 0 refused");
    r.base[1] = 1.0f;
    check(mf_ais_ment_steps(r.x.data(), 8, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, r.noise.data(),
                            r.betas.data(), 5, 4, 0, 2, r.scale.data(), 1.f, r.mean.data(), r.base.data(), nullptr, r.out.data(),
                            r.accepted.data(), r.logp.data(), nullptr) != 0, "a null logw refused");
    for (float v : r.out) check(std::isnan(v), "a refused call writes nothing");
    printf("SANITIZE AIS OK\n");
    fflush(stdout);
}

namespace {
struct AisSection {
    AisSection() { sanitize_ais(); }
} ais_section;
}  // namespace
