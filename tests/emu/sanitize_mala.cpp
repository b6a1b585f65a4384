// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
// Langevin section of the sanitizer driver (mentflow_amd/csrc/mala.hip).  tests/emu/build_sanitize.sh links every
// tests/emu/sanitize_*.cpp into tests/emu/sanitize_emu; main (in sanitize_main.cpp) knows nothing of this section, so it runs
// from the constructor of a namespace-scope object of this translation unit, before main, and prints its own marker (sound for
// the reasons given at the top of sanitize_swd_grad.cpp: nothing it reaches depends on another translation unit's dynamic
// initialisation).  It calls mf_mala_ment_steps on small synthetic inputs whose buffers have exactly the documented sizes, the
// cases of sanitize_mcmc.cpp: tables in LDS and beyond it, d = 1, 3 and 8, zero slots, a chain count that is not a multiple of
// the workgroup, out == NULL, logp == NULL and non-NULL, a keep_every that never hits, runs cut into launches, NaN noise, a
// chain that starts outside every hull, drift_clip = 0, and the refusals.  Any out-of-range index or undefined arithmetic aborts.
#include <cstring>

#include "sanitize_common.h"

struct MalaRun {
    std::vector<float> x, noise, scale, out, logp;
    std::vector<int32_t> accepted;
};

static MalaRun make_run(int64_t chains, int d, int64_t steps, int64_t n_keep) {
    MalaRun r;
    r.x.resize((size_t)chains * d);
    for (auto& v : r.x) v = 0.7f * nrand();
    for (int j = 0; j < d; ++j) r.x[(size_t)(chains - 1) * d + j] = 25.0f;        // a chain that starts outside every hull
    r.noise.resize((size_t)steps * (d + 1) * chains);
    for (int64_t t = 0; t < steps; ++t)
        for (int a = 0; a <= d; ++a)
            for (int64_t c = 0; c < chains; ++c) r.noise[(size_t)((t * (d + 1) + a) * chains + c)] = a < d ? nrand() : urand();
    r.scale.assign(d, 0.3f);
    r.out.assign((size_t)n_keep * chains * d, NAN);
    r.logp.assign(chains, NAN);
    r.accepted.assign(chains, 0);
    return r;
}

static void mala_on(const Slots& s, int d, int kind, float clip) {
    const int64_t chains = 300, steps = 12;                  // two workgroups, the second with 44 lanes
    const float a = kind == 1 ? 1.5f : 3.0f;
    const float lognorm = kind == 1 ? -d * (std::log(a) + 0.9189385f) : -d * std::log(2.0f * a);
    // the full trajectory in one launch, logp written
    MalaRun r = make_run(chains, d, steps, steps);
    r.noise[(size_t)((3 * (d + 1) + 0) * chains + 5)] = NAN;                      // chain 5 meets a NaN proposal at step 3
    r.noise[(size_t)((4 * (d + 1) + d) * chains + 6)] = NAN;                      // chain 6 a NaN uniform at step 4
    r.noise[(size_t)((2 * (d + 1) + 0) * chains + (chains - 1))] = NAN;           // the outside chain a NaN proposal at step 2
    std::vector<float> x0 = r.x;
    CK(mf_mala_ment_steps(r.x.data(), chains, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(),
                          kind, a, lognorm, r.noise.data(), steps, 0, r.scale.data(), clip, 0, 1, r.out.data(),
                          r.accepted.data(), r.logp.data(), nullptr));
    for (float v : r.out) check(std::isfinite(v), "every kept state is finite");
    for (int64_t c = 0; c < chains; ++c) {
        check(r.accepted[c] >= 0 && r.accepted[c] <= steps, "acceptance count in range");
        check(!std::isnan(r.logp[c]) && !(std::isinf(r.logp[c]) && r.logp[c] > 0.0f), "logp of a final state is finite or -inf");
    }
    // the same run cut in two launches, every 5th state from step 2 kept (rows of steps 2, 7), into exactly two rows; logp NULL
    // in the first launch
    MalaRun q = make_run(chains, d, steps, 2);
    q.x = x0;
    q.noise = r.noise;
    const size_t cut = (size_t)7 * (d + 1) * chains;
    CK(mf_mala_ment_steps(q.x.data(), chains, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(),
                          kind, a, lognorm, q.noise.data(), 7, 0, q.scale.data(), clip, 2, 5, q.out.data(), q.accepted.data(),
                          nullptr, nullptr));
    CK(mf_mala_ment_steps(q.x.data(), chains, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(),
                          kind, a, lognorm, q.noise.data() + cut, steps - 7, 7, q.scale.data(), clip, 2, 5, q.out.data(),
                          q.accepted.data(), q.logp.data(), nullptr));
    for (float v : q.out) check(std::isfinite(v), "both kept rows written");
    check(memcmp(q.x.data(), r.x.data(), q.x.size() * sizeof(float)) == 0, "two launches give the states of one");
    check(memcmp(q.logp.data(), r.logp.data(), q.logp.size() * sizeof(float)) == 0, "and the same logp bits");
    check(memcmp(q.accepted.data(), r.accepted.data(), q.accepted.size() * sizeof(int32_t)) == 0, "and the same counts");
    // out == NULL, and a keep_from / keep_every that never hit with a one-row buffer that must stay untouched
    MalaRun n = make_run(chains, d, steps, 1);
    n.noise = r.noise;
    CK(mf_mala_ment_steps(n.x.data(), chains, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(),
                          kind, a, lognorm, n.noise.data(), steps, 0, n.scale.data(), clip, 0, 1, nullptr, n.accepted.data(),
                          nullptr, nullptr));
    CK(mf_mala_ment_steps(n.x.data(), chains, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(),
                          kind, a, lognorm, n.noise.data(), steps, 1, n.scale.data(), clip, 0, 1000, n.out.data(),
                          n.accepted.data(), n.logp.data(), nullptr));
    CK(mf_mala_ment_steps(n.x.data(), chains, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(),
                          kind, a, lognorm, n.noise.data(), steps, 0, n.scale.data(), clip, steps, 1, n.out.data(),
                          n.accepted.data(), nullptr, nullptr));
    for (float v : n.out) check(std::isnan(v), "nothing kept");
    for (float v : n.x) check(std::isfinite(v), "finite states");
}

// (external like sanitize_ment_logp: as a static function it is inlined into the dynamic initialiser below, whose string
// constants ASan then registers at unaligned addresses and refuses)
void sanitize_mala() {
    seed(2024u);
    for (int d : {1, 3, 8}) {
        std::vector<int> small = d == 1 ? std::vector<int>{1, 1, 1} : std::vector<int>{1, 2, 1, 1, 2};
        mala_on(make_slots(d, small, 12), d, 1, 1.0f);             // tables in LDS, Gaussian prior
        mala_on(make_slots(d, small, 12), d, 0, 0.0f);             // no prior, no drift
        mala_on(make_slots(d, {}, 4), d, 2, 1.0f);                 // zero slots: the uniform prior alone
        mala_on(make_slots(d, {}, 4), d, 1, 2.5f);                 // zero slots: the Gaussian prior alone, a wide clip
        if (d > 1) mala_on(make_slots(d, {2, 2}, 85), d, 0, 1.0f);   // 2 x 85^2 floats: tables read from global memory
        else mala_on(make_slots(d, std::vector<int>(130, 1), 85), d, 0, 1.0f);   // 130 x 85 floats: beyond the LDS budget in 1-D
    }
    // no chains: nothing to do; refusals: no launch, an error instead
    Slots s = make_slots(3, {1}, 8);
    MalaRun r = make_run(8, 3, 4, 4);
    CK(mf_mala_ment_steps(r.x.data(), 0, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, r.noise.data(), 4,
                          0, r.scale.data(), 1.f, 0, 1, r.out.data(), r.accepted.data(), r.logp.data(), nullptr));
    check(mf_mala_ment_steps(r.x.data(), 8, 9, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, r.noise.data(),
                             4, 0, r.scale.data(), 1.f, 0, 1, r.out.data(), r.accepted.data(), r.logp.data(), nullptr) != 0,
          "d = 9 refused");
    check(mf_mala_ment_steps(r.x.data(), 8, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, r.noise.data(),
                             4, 0, r.scale.data(), 1.f, 0, 0, r.out.data(), r.accepted.data(), r.logp.data(), nullptr) != 0,
          "keep_every = 0 refused");
    check(mf_mala_ment_steps(r.x.data(), 8, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, r.noise.data(),
                             -1, 0, r.scale.data(), 1.f, 0, 1, r.out.data(), r.accepted.data(), r.logp.data(), nullptr) != 0,
          "negative steps refused");
    check(mf_mala_ment_steps(r.x.data(), 8, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, r.noise.data(),
                             4, 0, r.scale.data(), 1.f, 0, (int64_t)1 << 50, r.out.data(), r.accepted.data(), r.logp.data(),
                             nullptr) != 0, "keep_every beyond 2^40 refused");
    check(mf_mala_ment_steps(r.x.data(), -1, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, r.noise.data(),
                             4, 0, r.scale.data(), 1.f, 0, 1, r.out.data(), r.accepted.data(), r.logp.data(), nullptr) != 0,
          "a negative chain count refused");
    check(mf_mala_ment_steps(r.x.data(), 8, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, r.noise.data(),
                             4, 0, r.scale.data(), -0.5f, 0, 1, r.out.data(), r.accepted.data(), r.logp.data(), nullptr) != 0,
          "drift_clip < 0 refused");
    check(mf_mala_ment_steps(r.x.data(), 8, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, r.noise.data(),
                             4, 0, r.scale.data(), NAN, 0, 1, r.out.data(), r.accepted.data(), r.logp.data(), nullptr) != 0,
          "a NaN drift_clip refused");
    for (float v : r.out) check(std::isnan(v), "a refused call writes nothing");
    printf("SANITIZE MALA OK\n");
    fflush(stdout);
}

namespace {
struct MalaSection {
    MalaSection() { sanitize_mala(); }
} mala_section;
}  // namespace
