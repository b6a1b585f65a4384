// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
// Weighted-projection section of the sanitizer driver (mentflow_amd/csrc/wproj.hip).  tests/emu/build_sanitize.sh links every
// tests/emu/sanitize_*.cpp into tests/emu/sanitize_emu; main (in sanitize_main.cpp) knows nothing of this section, so it runs
// from the constructor of a namespace-scope object of this translation unit, before main, and prints its own marker, as
// sanitize_smc.cpp does.  It calls mf_proj_wkde1d_fwd / _bwd, mf_proj_wkde2d_fwd / _bwd, mf_proj_whist1d_sums and
// mf_proj_whist2d_sums on buffers of exactly the documented sizes: ragged n (1, 255, 257, 1 500 and 8 193, which crosses one
// workgroup's particle bound), d = 1, 2, 6, 8, one, three and 101 projections (several projection groups), radius 4 (the
// factorised window) and 5 (the run-time one), NaN / inf rows, weights that are random, partly zero, hold a negative, a NaN and
// an inf, and are all invalid; either gradient alone and both with accumulate; and the refusals.  Any out-of-range index or
// undefined arithmetic aborts.
#include <cstring>

#include "sanitize_common.h"

struct Grid {
    std::vector<float> edges, coords;
    float delta;
};

static Grid make_grid(int B, float lo, float hi) {
    Grid g;
    g.delta = (hi - lo) / B;
    for (int i = 0; i <= B; ++i) g.edges.push_back(lo + g.delta * i);
    for (int i = 0; i < B; ++i) g.coords.push_back(lo + g.delta * (i + 0.5f));
    return g;
}

static std::vector<float> make_rows(int64_t n, int d) {
    std::vector<float> x((size_t)n * d);
    for (float& v : x) v = 1.5f * nrand();
    if (n >= 255) {
        x[(size_t)7 * d + (d - 1)] = NAN;
        x[(size_t)11 * d] = INFINITY;
        x[(size_t)13 * d] = -1.0e30f;
    }
    return x;
}

static std::vector<float> make_dirs(int P, int d) {
    std::vector<float> V((size_t)P * d);
    for (float& v : V) v = urand() - 0.5f;
    return V;
}

// pattern 0: random; 1: a tenth zero; 2: one negative, one NaN, one inf, one zero; 3: none valid
static std::vector<float> make_weights(int64_t n, int pattern, float* wmax) {
    std::vector<float> w(n);
    for (int64_t i = 0; i < n; ++i) {
        w[i] = std::exp(2.0f * nrand());
        if (pattern == 1 && urand() < 0.1f) w[i] = 0.0f;
        if (pattern == 3) w[i] = (i % 4 == 0) ? 0.0f : (i % 4 == 1) ? -1.0f : (i % 4 == 2) ? NAN : INFINITY;
    }
    if (pattern == 2 && n >= 4) {
        w[n / 5] = -1.5f;
        w[n / 3] = NAN;
        w[n / 2] = INFINITY;
        w[n - 1] = 0.0f;
    }
    *wmax = 0.0f;
    for (float v : w)
        if (std::isfinite(v) && v > *wmax) *wmax = v;
    return w;
}

static void all_finite(const std::vector<float>& v, const char* what) {
    for (float f : v) check(std::isfinite(f), what);
}

static void wproj_on(int64_t n, int d, int P, int B, int radius, int pattern) {
    const Grid g = make_grid(B, -4.0f, 4.0f), gy = make_grid(B > 20 ? 13 : B + 1, -3.0f, 3.5f);
    const int By = (int)gy.coords.size();
    const float bw = radius == 4 ? 0.5f : 0.6f;
    const std::vector<float> x = make_rows(n, d), V0 = make_dirs(P, d), V1 = make_dirs(P, d);
    float wmax;
    const std::vector<float> w = make_weights(n, pattern, &wmax);
    // 1-D
    std::vector<float> S((size_t)P * B, NAN), gS((size_t)P * B);
    for (float& v : gS) v = nrand();
    std::vector<char> ws((size_t)mf_proj_kde_ws_bytes(P, B));
    CK(mf_proj_wkde1d_fwd(x.data(), w.data(), &wmax, n, d, V0.data(), P, g.coords.data(), B, bw * g.delta, radius, S.data(),
                          ws.data(), nullptr));
    all_finite(S, "1-D sums are finite");
    if (pattern == 3)
        for (float v : S) check(v == 0.0f, "no valid weight: S == 0");
    std::vector<float> gx((size_t)n * d, 1.0f), gw(n, 1.0f);
    CK(mf_proj_wkde1d_bwd(x.data(), w.data(), n, d, V0.data(), P, g.coords.data(), B, bw * g.delta, radius, gS.data(), gx.data(),
                          gw.data(), 0, nullptr));
    CK(mf_proj_wkde1d_bwd(x.data(), w.data(), n, d, V0.data(), P, g.coords.data(), B, bw * g.delta, radius, gS.data(), gx.data(),
                          gw.data(), 1, nullptr));
    CK(mf_proj_wkde1d_bwd(x.data(), w.data(), n, d, V0.data(), P, g.coords.data(), B, bw * g.delta, radius, gS.data(), nullptr,
                          gw.data(), 0, nullptr));
    CK(mf_proj_wkde1d_bwd(x.data(), w.data(), n, d, V0.data(), P, g.coords.data(), B, bw * g.delta, radius, gS.data(), gx.data(),
                          nullptr, 0, nullptr));
    all_finite(gx, "1-D gx is finite");
    all_finite(gw, "1-D gw is finite");
    for (int64_t i = 0; i < n; ++i)
        if (!(std::isfinite(w[i]) && w[i] >= 0.0f)) check(gw[i] == 0.0f, "gw == 0 at a negative, NaN or infinite weight");
    // hard bins, 1-D
    std::vector<float> H((size_t)P * B, NAN);
    CK(mf_proj_whist1d_sums(x.data(), w.data(), &wmax, n, d, V0.data(), P, g.edges.data(), B, H.data(), ws.data(), nullptr));
    all_finite(H, "1-D hard-binned sums are finite");
    // 2-D: a B x By image (radius_y one less, so the two axes differ unless both are 4)
    const int ry = radius == 4 ? 4 : radius - 2;
    const float bwy = radius == 4 ? 0.5f : 0.38f;
    std::vector<float> S2((size_t)P * B * By, NAN), gS2((size_t)P * B * By);
    for (float& v : gS2) v = nrand();
    std::vector<char> ws2((size_t)mf_proj_kde_ws_bytes(P, B * By));
    CK(mf_proj_wkde2d_fwd(x.data(), w.data(), &wmax, n, d, V0.data(), V1.data(), P, g.coords.data(), B, bw * g.delta, radius,
                          gy.coords.data(), By, bwy * gy.delta, ry, S2.data(), ws2.data(), nullptr));
    all_finite(S2, "2-D sums are finite");
    CK(mf_proj_wkde2d_bwd(x.data(), w.data(), n, d, V0.data(), V1.data(), P, g.coords.data(), B, bw * g.delta, radius,
                          gy.coords.data(), By, bwy * gy.delta, ry, gS2.data(), gx.data(), gw.data(), 0, nullptr));
    CK(mf_proj_wkde2d_bwd(x.data(), w.data(), n, d, V0.data(), V1.data(), P, g.coords.data(), B, bw * g.delta, radius,
                          gy.coords.data(), By, bwy * gy.delta, ry, gS2.data(), gx.data(), nullptr, 1, nullptr));
    CK(mf_proj_wkde2d_bwd(x.data(), w.data(), n, d, V0.data(), V1.data(), P, g.coords.data(), B, bw * g.delta, radius,
                          gy.coords.data(), By, bwy * gy.delta, ry, gS2.data(), nullptr, gw.data(), 1, nullptr));
    all_finite(gx, "2-D gx is finite");
    all_finite(gw, "2-D gw is finite");
    std::vector<float> H2((size_t)P * B * By, NAN);
    CK(mf_proj_whist2d_sums(x.data(), w.data(), &wmax, n, d, V0.data(), V1.data(), P, g.edges.data(), B, gy.edges.data(), By,
                            H2.data(), ws2.data(), nullptr));
    all_finite(H2, "2-D hard-binned sums are finite");
}

// (external like sanitize_smc: see the note there)
void sanitize_wproj() {
    seed(2027u);
    const int64_t sizes[] = {1, 255, 257, 1500, 8193};
    const int dims[] = {1, 2, 6, 8};
    int turn = 0;
    for (int64_t n : sizes)
        for (int pattern = 0; pattern < 4; ++pattern, ++turn) {
            const int d = dims[turn % 4];
            const int P = (turn % 3 == 0) ? 1 : 3;
            wproj_on(n, d, P, turn % 2 ? 16 : 85, turn % 2 ? 5 : 4, pattern);
            wproj_on(n, dims[(turn + 1) % 4], P, turn % 2 ? 64 : 17, turn % 2 ? 4 : 5, pattern);
        }
    wproj_on(257, 6, 101, 64, 4, 2);                 // several projection groups
    wproj_on(8193, 2, 101, 17, 5, 1);
    // no particles: the sums are zero, the backwards do nothing; then the refusals
    const Grid g = make_grid(16, -4.0f, 4.0f);
    std::vector<float> x(24 * 3, 0.5f), w(24, 1.0f), V(3 * 3, 0.3f), S(3 * 16, NAN), gS(3 * 16, 1.0f), gx(24 * 3, NAN), gw(24, NAN);
    std::vector<float> S2(3 * 16 * 16, NAN);
    std::vector<char> ws((size_t)mf_proj_kde_ws_bytes(3, 16 * 16));
    float wmax = 1.0f;
    const float sg = 0.5f * g.delta;
    CK(mf_proj_wkde1d_fwd(nullptr, nullptr, &wmax, 0, 3, V.data(), 3, g.coords.data(), 16, sg, 4, S.data(), ws.data(), nullptr));
    for (float v : S) check(v == 0.0f, "n = 0: S == 0");
    CK(mf_proj_whist1d_sums(nullptr, nullptr, &wmax, 0, 3, V.data(), 3, g.edges.data(), 16, S.data(), ws.data(), nullptr));
    CK(mf_proj_wkde1d_bwd(nullptr, nullptr, 0, 3, V.data(), 3, g.coords.data(), 16, sg, 4, gS.data(), gx.data(), gw.data(), 0, nullptr));
    std::fill(S.begin(), S.end(), NAN);
#define REFUSED(call, what) check((call) != 0 && strlen(mf_last_error()) > 0, what)
    REFUSED(mf_proj_wkde1d_fwd(x.data(), w.data(), &wmax, 24, 9, V.data(), 3, g.coords.data(), 16, sg, 4, S.data(), ws.data(), nullptr), "d = 9");
    REFUSED(mf_proj_wkde1d_fwd(x.data(), w.data(), &wmax, 24, 0, V.data(), 3, g.coords.data(), 16, sg, 4, S.data(), ws.data(), nullptr), "d = 0");
    REFUSED(mf_proj_wkde1d_fwd(x.data(), w.data(), &wmax, -1, 3, V.data(), 3, g.coords.data(), 16, sg, 4, S.data(), ws.data(), nullptr), "n < 0");
    REFUSED(mf_proj_wkde1d_fwd(x.data(), w.data(), &wmax, 24, 3, V.data(), 0, g.coords.data(), 16, sg, 4, S.data(), ws.data(), nullptr), "P = 0");
    REFUSED(mf_proj_wkde1d_fwd(x.data(), w.data(), &wmax, 24, 3, V.data(), 3, g.coords.data(), 1, sg, 4, S.data(), ws.data(), nullptr), "one bin");
    REFUSED(mf_proj_wkde1d_fwd(x.data(), w.data(), &wmax, 24, 3, V.data(), 3, g.coords.data(), 16, 0.0f, 4, S.data(), ws.data(), nullptr), "sigma = 0");
    REFUSED(mf_proj_wkde1d_fwd(x.data(), w.data(), &wmax, 24, 3, V.data(), 3, g.coords.data(), 16, NAN, 4, S.data(), ws.data(), nullptr), "sigma NaN");
    REFUSED(mf_proj_wkde1d_fwd(x.data(), nullptr, &wmax, 24, 3, V.data(), 3, g.coords.data(), 16, sg, 4, S.data(), ws.data(), nullptr), "null w");
    REFUSED(mf_proj_wkde1d_fwd(x.data(), w.data(), nullptr, 24, 3, V.data(), 3, g.coords.data(), 16, sg, 4, S.data(), ws.data(), nullptr), "null wmax");
    REFUSED(mf_proj_wkde1d_fwd(x.data(), w.data(), &wmax, 24, 3, V.data(), 3, g.coords.data(), 16, sg, 4, S.data(), nullptr, nullptr), "null ws");
    REFUSED(mf_proj_wkde1d_bwd(x.data(), w.data(), 24, 3, V.data(), 3, g.coords.data(), 16, sg, 4, gS.data(), nullptr, nullptr, 0, nullptr), "no output");
    REFUSED(mf_proj_wkde1d_bwd(x.data(), w.data(), 24, 3, V.data(), 3, g.coords.data(), 16, sg, 4, nullptr, gx.data(), gw.data(), 0, nullptr), "null gS");
    REFUSED(mf_proj_wkde1d_bwd(x.data(), w.data(), 24, 9, V.data(), 3, g.coords.data(), 16, sg, 4, gS.data(), gx.data(), gw.data(), 0, nullptr), "d = 9");
    REFUSED(mf_proj_wkde2d_fwd(x.data(), w.data(), &wmax, 24, 3, V.data(), V.data(), 3, g.coords.data(), 16, sg, 6, g.coords.data(), 16, sg, 4, S2.data(), ws.data(), nullptr), "radius 6");
    REFUSED(mf_proj_wkde2d_fwd(x.data(), w.data(), &wmax, 24, 3, V.data(), V.data(), 3, g.coords.data(), 16, sg, -1, g.coords.data(), 16, sg, 4, S2.data(), ws.data(), nullptr), "radius -1");
    REFUSED(mf_proj_wkde2d_fwd(x.data(), w.data(), &wmax, 24, 3, V.data(), V.data(), 3, g.coords.data(), 16, sg, 4, g.coords.data(), 16, -sg, 4, S2.data(), ws.data(), nullptr), "sigma_y < 0");
    REFUSED(mf_proj_wkde2d_fwd(x.data(), w.data(), &wmax, 24, 3, V.data(), nullptr, 3, g.coords.data(), 16, sg, 4, g.coords.data(), 16, sg, 4, S2.data(), ws.data(), nullptr), "null V1");
    REFUSED(mf_proj_wkde2d_fwd(x.data(), w.data(), &wmax, 24, 3, V.data(), V.data(), 3, g.coords.data(), 400, sg, 4, g.coords.data(), 400, sg, 4, S2.data(), ws.data(), nullptr), "an image beyond LDS");
    REFUSED(mf_proj_wkde2d_bwd(x.data(), w.data(), 24, 3, V.data(), V.data(), 3, g.coords.data(), 16, sg, 4, g.coords.data(), 16, sg, 4, gS.data(), nullptr, nullptr, 0, nullptr), "no output");
    REFUSED(mf_proj_wkde2d_bwd(x.data(), w.data(), 24, 3, V.data(), V.data(), 3, g.coords.data(), 16, sg, 4, g.coords.data(), 1, sg, 4, gS.data(), gx.data(), gw.data(), 0, nullptr), "one bin in y");
    REFUSED(mf_proj_whist1d_sums(x.data(), w.data(), &wmax, 24, 3, V.data(), 3, g.edges.data(), 1, S.data(), ws.data(), nullptr), "one bin");
    REFUSED(mf_proj_whist1d_sums(x.data(), w.data(), &wmax, 24, 3, V.data(), 3, g.edges.data(), 20000, S.data(), ws.data(), nullptr), "too many bins");
    REFUSED(mf_proj_whist1d_sums(x.data(), w.data(), &wmax, 24, 3, V.data(), 3, g.edges.data(), 16, nullptr, ws.data(), nullptr), "null sums");
    REFUSED(mf_proj_whist2d_sums(x.data(), w.data(), &wmax, 24, 9, V.data(), V.data(), 3, g.edges.data(), 16, g.edges.data(), 16, S2.data(), ws.data(), nullptr), "d = 9");
    REFUSED(mf_proj_whist2d_sums(x.data(), w.data(), &wmax, 24, 3, V.data(), V.data(), 3, g.edges.data(), 200, g.edges.data(), 200, S2.data(), ws.data(), nullptr), "an image beyond LDS");
    REFUSED(mf_proj_whist2d_sums(x.data(), nullptr, &wmax, 24, 3, V.data(), V.data(), 3, g.edges.data(), 16, g.edges.data(), 16, S2.data(), ws.data(), nullptr), "null w");
#undef REFUSED
    for (float v : S) check(std::isnan(v), "a refused call writes nothing");
    for (float v : S2) check(std::isnan(v), "a refused call writes nothing (2-D)");
    for (float v : gx) check(std::isnan(v), "nor any gradient");
    for (float v : gw) check(std::isnan(v), "nor any weight gradient");
    printf("SANITIZE WPROJ OK\n");
    fflush(stdout);
}

namespace {
struct WprojSection {
    WprojSection() { sanitize_wproj(); }
} wproj_section;
}  // namespace
