// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
// Metropolis-Hastings section of the sanitizer driver (mentflow_amd/csrc/mcmc.hip).  tests/emu/build_sanitize.sh links it into
// tests/emu/sanitize_emu (AddressSanitizer + UndefinedBehaviorSanitizer, the fiber emulator's exactly-sized, guard-paged
// dynamic LDS), whose main, in sanitize_main.cpp, calls sanitize_mcmc().  It calls mf_mcmc_ment_steps on small synthetic inputs
// whose buffers have exactly the documented sizes: tables in LDS and beyond it, d = 1 and d = 8, zero slots, a chain count that
// is not a multiple of the workgroup, out == NULL, a keep_every that never hits, runs cut into launches, NaN noise, and the
// refusals.  Any out-of-range index or undefined arithmetic aborts.
#include "sanitize_common.h"

struct Run {
    std::vector<float> x, noise, scale, out;
    std::vector<int32_t> accepted;
};

static Run make_run(int64_t chains, int d, int64_t steps, int64_t n_keep) {
    Run r;
    r.x.resize((size_t)chains * d);
    for (auto& v : r.x) v = 0.7f * nrand();
    for (int j = 0; j < d; ++j) r.x[(size_t)(chains - 1) * d + j] = 25.0f;        // a chain that starts outside every hull
    r.noise.resize((size_t)steps * (d + 1) * chains);
    for (int64_t t = 0; t < steps; ++t)
        for (int a = 0; a <= d; ++a)
            for (int64_t c = 0; c < chains; ++c) r.noise[(size_t)((t * (d + 1) + a) * chains + c)] = a < d ? nrand() : urand();
    r.scale.assign(d, 0.3f);
    r.out.assign((size_t)n_keep * chains * d, NAN);
    r.accepted.assign(chains, 0);
    return r;
}

static void steps_on(const Slots& s, int d, int kind) {
    const int64_t chains = 300, steps = 12;                  // two workgroups, the second with 44 lanes
    const float a = kind == 1 ? 1.5f : 3.0f;
    const float lognorm = kind == 1 ? -d * (std::log(a) + 0.9189385f) : -d * std::log(2.0f * a);
    // the full trajectory in one launch
    Run r = make_run(chains, d, steps, steps);
    r.noise[(size_t)((3 * (d + 1) + 0) * chains + 5)] = NAN;                      // chain 5 meets a NaN proposal at step 3
    CK(mf_mcmc_ment_steps(r.x.data(), chains, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(),
                          kind, a, lognorm, r.noise.data(), steps, 0, r.scale.data(), 0, 1, r.out.data(), r.accepted.data(),
                          nullptr));
    for (float v : r.out) check(std::isfinite(v), "every kept state is finite");
    for (int64_t c = 0; c < chains; ++c) check(r.accepted[c] >= 0 && r.accepted[c] <= steps, "acceptance count in range");
    // the same run cut in two launches, every 5th state from step 2 kept (rows of steps 2, 7), into exactly two rows
    Run q = make_run(chains, d, steps, 2);
    q.x = make_run(chains, d, steps, 0).x;
    std::vector<float> x0 = q.x;
    q.noise = r.noise;
    const size_t cut = (size_t)7 * (d + 1) * chains;
    CK(mf_mcmc_ment_steps(q.x.data(), chains, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(),
                          kind, a, lognorm, q.noise.data(), 7, 0, q.scale.data(), 2, 5, q.out.data(), q.accepted.data(),
                          nullptr));
    CK(mf_mcmc_ment_steps(q.x.data(), chains, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(),
                          kind, a, lognorm, q.noise.data() + cut, steps - 7, 7, q.scale.data(), 2, 5, q.out.data(),
                          q.accepted.data(), nullptr));
    for (float v : q.out) check(std::isfinite(v), "both kept rows written");
    // out == NULL, and a keep_from / keep_every that never hit with a one-row buffer that must stay untouched
    Run n = make_run(chains, d, steps, 1);
    n.noise = r.noise;
    CK(mf_mcmc_ment_steps(n.x.data(), chains, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(),
                          kind, a, lognorm, n.noise.data(), steps, 0, n.scale.data(), 0, 1, nullptr, n.accepted.data(), nullptr));
    CK(mf_mcmc_ment_steps(n.x.data(), chains, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(),
                          kind, a, lognorm, n.noise.data(), steps, 1, n.scale.data(), 0, 1000, n.out.data(), n.accepted.data(),
                          nullptr));
    CK(mf_mcmc_ment_steps(n.x.data(), chains, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), (int64_t)s.tables.size(),
                          kind, a, lognorm, n.noise.data(), steps, 0, n.scale.data(), steps, 1, n.out.data(), n.accepted.data(),
                          nullptr));
    for (float v : n.out) check(std::isnan(v), "nothing kept");
    for (float v : n.x) check(std::isfinite(v), "finite states");
}

void sanitize_mcmc() {
    seed(777u);
    for (int d : {1, 3, 8}) {
        std::vector<int> small = d == 1 ? std::vector<int>{1, 1, 1} : std::vector<int>{1, 2, 1, 1, 2};
        steps_on(make_slots(d, small, 12), d, 1);              // tables in LDS, Gaussian prior
        steps_on(make_slots(d, {}, 4), d, 2);                  // zero slots: the uniform prior alone
        if (d > 1) steps_on(make_slots(d, {2, 2}, 85), d, 0);  // 2 x 85^2 floats: tables read from global memory
        else steps_on(make_slots(d, std::vector<int>(130, 1), 85), d, 0);   // 130 x 85 floats: beyond the LDS budget in 1-D
    }
    // no chains: nothing to do; refusals: no launch, an error instead
    Slots s = make_slots(3, {1}, 8);
    Run r = make_run(8, 3, 4, 4);
    CK(mf_mcmc_ment_steps(r.x.data(), 0, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, r.noise.data(), 4,
                          0, r.scale.data(), 0, 1, r.out.data(), r.accepted.data(), nullptr));
    check(mf_mcmc_ment_steps(r.x.data(), 8, 9, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, r.noise.data(),
                             4, 0, r.scale.data(), 0, 1, r.out.data(), r.accepted.data(), nullptr) != 0, "d = 9 refused");
    check(mf_mcmc_ment_steps(r.x.data(), 8, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, r.noise.data(),
                             4, 0, r.scale.data(), 0, 0, r.out.data(), r.accepted.data(), nullptr) != 0, "keep_every = 0 refused");
    check(mf_mcmc_ment_steps(r.x.data(), 8, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, r.noise.data(),
                             -1, 0, r.scale.data(), 0, 1, r.out.data(), r.accepted.data(), nullptr) != 0, "negative steps refused");
    check(mf_mcmc_ment_steps(r.x.data(), 8, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, r.noise.data(),
                             4, 0, r.scale.data(), 0, (int64_t)1 << 50, r.out.data(), r.accepted.data(), nullptr) != 0,
          "keep_every beyond 2^40 refused");
    printf("SANITIZE MCMC OK\n");
}
