// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
// Classical-MENT section of the sanitizer driver (mentflow_amd/csrc/ment.hip).  tests/emu/build_sanitize.sh links it into
// tests/emu/sanitize_emu (AddressSanitizer + UndefinedBehaviorSanitizer, the fiber emulator's exactly-sized, guard-paged
// dynamic LDS), whose main, in sanitize_main.cpp, calls sanitize_ment().  It calls every mf_ment_* entry point on small synthetic
// inputs: tables in LDS and beyond it, multiply mode, NaN rows, every prior kind, grids with a tail block, sampling over several
// blocks with and without noise, and integrals of more than one 4096-point chunk.  Any out-of-range index or undefined
// arithmetic aborts.
#include "sanitize_common.h"

static std::vector<float> points(int64_t n, int d) {
    std::vector<float> x((size_t)n * d);
    for (auto& v : x) v = 7.0f * (urand() - 0.5f);
    for (int j = 0; j < d; ++j) x[(size_t)(n - 1) * d + j] = NAN;             // a NaN row
    x[(size_t)(n - 2) * d] = NAN;                                               // a row with one NaN coordinate
    return x;
}

static void prob_points() {
    const int64_t n = 1000;                                   // not a multiple of the 256-thread block
    for (int d : {3, 8}) {
        Slots small = make_slots(d, {1, 2, 1, 1, 2}, 12);      // tables in LDS
        Slots big = make_slots(d, {2, 2}, 85);                 // 2 x 85^2 floats: read from global memory
        Slots none = make_slots(d, {}, 4);                     // prior only
        std::vector<float> x = points(n, d), out(n);
        for (int kind = 0; kind <= 2; ++kind) {
            const float a = kind == 1 ? 1.5f : 3.0f;
            const float lognorm = kind == 1 ? -d * (std::log(a) + 0.9189385f) : -d * std::log(2.0f * a);
            CK(mf_ment_prob(x.data(), n, d, small.n, small.desc.data(), small.meta.data(), small.tables.data(),
                            (int64_t)small.tables.size(), kind, a, lognorm, 0, out.data(), nullptr));
            CK(mf_ment_prob(x.data(), n, d, big.n, big.desc.data(), big.meta.data(), big.tables.data(),
                            (int64_t)big.tables.size(), 0, 0.0f, 0.0f, 1, out.data(), nullptr));
            CK(mf_ment_prob(x.data(), n, d, none.n, none.desc.data(), none.meta.data(), none.tables.data(),
                            (int64_t)none.tables.size(), kind, a, lognorm, 1, out.data(), nullptr));
            check(std::isnan(out[n - 1]) && std::isnan(out[n - 2]), "NaN rows give NaN");
            for (int64_t p = 0; p < n - 2; ++p) check(std::isfinite(out[p]) && out[p] >= 0.0f, "finite prob");
        }
    }
    // refusals: no launch, an error instead
    Slots s = make_slots(3, {1}, 8);
    std::vector<float> x = points(16, 3), out(16);
    check(mf_ment_prob(x.data(), 16, 9, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, 0, out.data(),
                       nullptr) != 0, "d = 9 refused");
    check(mf_ment_prob(x.data(), 16, 3, 600, s.desc.data(), s.meta.data(), s.tables.data(), 8, 0, 0.f, 0.f, 0, out.data(),
                       nullptr) != 0, "600 slots refused");
}

static void grid_and_sample() {
    const int d = 3;
    const int64_t shape[3] = {13, 11, 9};                     // 1287 cells: one full 1024-cell block and a tail
    const int64_t ncells = 13 * 11 * 9;
    std::vector<float> coords, edges;
    for (int j = 0; j < d; ++j) {
        const float lo = -3.2f, hi = 3.1f, dl = (hi - lo) / shape[j];
        for (int k = 0; k <= shape[j]; ++k) edges.push_back(lo + k * dl);
        for (int k = 0; k < shape[j]; ++k) coords.push_back(lo + (k + 0.5f) * dl);
    }
    const int64_t nb = mf_ment_blocks(ncells);
    check(nb == 2, "two sampling blocks");
    std::vector<float> prob(ncells), prob2(ncells);
    std::vector<double> sums(nb), sums2(nb), prefix(nb + 1);
    for (int variant = 0; variant < 2; ++variant) {
        Slots s = variant == 0 ? make_slots(d, {1, 2, 1}, 10) : make_slots(d, {2, 2}, 85);   // LDS / global tables
        CK(mf_ment_prob_grid(coords.data(), shape, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(),
                             (int64_t)s.tables.size(), 1, 2.0f, -3.0f, prob.data(), sums.data(), nullptr));
        CK(mf_ment_block_sums(prob.data(), ncells, sums2.data(), nullptr));
        for (int64_t b = 0; b < nb; ++b) check(std::fabs(sums[b] - sums2[b]) <= 1e-9 * (1.0 + std::fabs(sums[b])), "block sums");
        for (int noise = 0; noise <= 1; ++noise) {
            const int64_t size = 700;
            std::vector<float> rnd((size_t)size * (1 + 2 * d)), x((size_t)size * d);
            for (auto& r : rnd) r = urand();
            rnd[0] = 0.0f;                                    // the first cell's lower edge
            rnd[(size_t)(size - 1) * (1 + 2 * d)] = 0.99999994f;   // the largest uniform below 1: the last cells
            CK(mf_ment_sample(prob.data(), shape, d, sums.data(), prefix.data(), edges.data(), rnd.data(), size, noise,
                              x.data(), nullptr));
            for (int64_t p = 0; p < size; ++p)
                for (int j = 0; j < d; ++j) {
                    const float lo = -3.2f, hi = 3.1f, dl = (hi - lo) / shape[j];
                    const float v = x[(size_t)p * d + j];
                    check(v >= lo - (noise ? 0.5f * dl : 0.0f) - 1e-5f && v <= hi + (noise ? 0.5f * dl : 0.0f) + 1e-5f,
                          "sample inside the grid");
                }
        }
    }
    // sample_hist on a 1-D histogram of 3000 bins (three blocks)
    const int64_t s1[1] = {3000};
    std::vector<float> h(3000), e(3001), x(500), rnd(500 * 3);
    for (int k = 0; k <= 3000; ++k) e[k] = -1.0f + k * (2.0f / 3000);
    for (auto& v : h) v = urand() < 0.5f ? 0.0f : urand();
    for (auto& r : rnd) r = urand();
    std::vector<double> bs(mf_ment_blocks(3000)), pf(mf_ment_blocks(3000) + 1);
    CK(mf_ment_block_sums(h.data(), 3000, bs.data(), nullptr));
    CK(mf_ment_sample(h.data(), s1, 1, bs.data(), pf.data(), e.data(), rnd.data(), 500, 1, x.data(), nullptr));
    check(mf_ment_block_sums(h.data(), 0, bs.data(), nullptr) != 0, "empty histogram refused");
}

static void integrate() {
    // 3-D, measured axis 1 (5 bins), integration axes 0 and 2 at 70 x 70 = 4900 points: two 4096-point chunks per bin
    {
        const int d = 3;
        Slots s = make_slots(d, {1, 2, 1}, 10);
        const int64_t counts[3] = {70, 5, 70};
        std::vector<float> coords;
        for (int j = 0; j < d; ++j)
            for (int k = 0; k < counts[j]; ++k) coords.push_back(-3.0f + 6.0f * (k + 0.5f) / counts[j]);
        const float minv[9] = {0.8f, 0.6f, 0.0f, -0.6f, 0.8f, 0.0f, 0.0f, 0.0f, 1.0f};
        const int32_t meas[1] = {1};
        const int64_t ws = mf_ment_integrate_ws_doubles(5, 4900);
        check(ws == 5 * 2, "two chunks per bin");
        std::vector<double> partial(ws);
        std::vector<float> pred(5);
        CK(mf_ment_integrate(d, minv, coords.data(), counts, 1, meas, s.n, s.desc.data(), s.meta.data(), s.tables.data(),
                             (int64_t)s.tables.size(), 1, 2.0f, -3.0f, partial.data(), pred.data(), nullptr));
        for (float v : pred) check(std::isfinite(v) && v >= 0.0f, "finite integral");
    }
    // 4-D plane integral (measured axes 2, 0 in that order) with tables beyond LDS
    {
        const int d = 4;
        Slots s = make_slots(d, {2, 2}, 85);
        const int64_t counts[4] = {6, 9, 4, 8};
        std::vector<float> coords;
        for (int j = 0; j < d; ++j)
            for (int k = 0; k < counts[j]; ++k) coords.push_back(-2.5f + 5.0f * (k + 0.5f) / counts[j]);
        float minv[16] = {};
        for (int i = 0; i < 4; ++i) minv[i * 4 + i] = 1.0f;
        const int32_t meas[2] = {2, 0};
        std::vector<double> partial(mf_ment_integrate_ws_doubles(24, 72));
        std::vector<float> pred(24);
        CK(mf_ment_integrate(d, minv, coords.data(), counts, 2, meas, s.n, s.desc.data(), s.meta.data(), s.tables.data(),
                             (int64_t)s.tables.size(), 2, 3.0f, -4.0f * std::log(6.0f), partial.data(), pred.data(),
                             nullptr));
        for (float v : pred) check(std::isfinite(v) && v >= 0.0f, "finite integral");
        const int32_t dup[2] = {1, 1};
        check(mf_ment_integrate(d, minv, coords.data(), counts, 2, dup, s.n, s.desc.data(), s.meta.data(), s.tables.data(),
                                (int64_t)s.tables.size(), 0, 0.f, 0.f, partial.data(), pred.data(), nullptr) != 0,
              "repeated measured axis refused");
    }
}

void sanitize_ment() {
    seed(4242u);
    prob_points();
    grid_and_sample();
    integrate();
    printf("SANITIZE MENT OK\n");
}
