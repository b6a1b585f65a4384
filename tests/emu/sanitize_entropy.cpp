// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
// Entropy-estimator section of the sanitizer driver (mentflow_amd/csrc/entropy.hip).  tests/emu/build_sanitize.sh links it into
// tests/emu/sanitize_emu (AddressSanitizer + UndefinedBehaviorSanitizer on the fiber emulator), whose main, in
// sanitize_main.cpp, calls sanitize_entropy().  It calls every mf_knn_entropy_* and mf_cov_entropy_* entry point on small
// synthetic inputs: ragged N (no multiple of the 256-query workgroup, the candidate tile or four), k = 1 and 16, every padded
// feature count, one and several candidate chunks (also more chunks than tiles), duplicate points, NaN and inf rows, N = k + 1,
// and the refusals.  Every buffer has exactly the documented size, so any out-of-range index or undefined arithmetic aborts.
#include "sanitize_common.h"

static std::vector<float> cloud(int64_t n, int d) {
    std::vector<float> x((size_t)n * d);
    for (auto& v : x) v = 4.0f * (urand() - 0.5f);
    return x;
}

// forward + backward with exactly sized buffers; returns H
static float knn(const std::vector<float>& x, int64_t n, int d, int k, int chunks, bool expect_finite) {
    const int64_t bytes = mf_knn_entropy_ws_bytes(n, d, k, chunks);
    check(bytes > 0 && bytes % 8 == 0, "workspace size");
    std::vector<double> ws((size_t)bytes / 8);
    std::vector<int32_t> idx(n);
    std::vector<float> rho2(n), gx((size_t)n * d);
    float H = 0.0f;
    double S = 0.0;
    const float coef = 1.0f;
    CK(mf_knn_entropy_fwd(x.data(), n, d, k, chunks, &H, &S, idx.data(), rho2.data(), ws.data(), nullptr));
    for (int64_t i = 0; i < n; ++i) check(idx[i] >= 0 && idx[i] < n, "neighbour index in range");
    CK(mf_knn_entropy_bwd(x.data(), n, d, idx.data(), rho2.data(), &coef, -(float)d / (float)n, gx.data(), nullptr));
    if (expect_finite) {
        check(std::isfinite(H) && std::isfinite(S), "finite H");
        for (float g : gx) check(std::isfinite(g), "finite gradient");
        for (int64_t i = 0; i < n; ++i) check(idx[i] != i, "no point is its own neighbour");
    } else {
        check(!std::isfinite(H), "non-finite input gives a non-finite H");
    }
    return H;
}

static void knn_cases() {
    for (int d : {1, 2, 3, 5, 6, 7, 11, 16}) {
        const int64_t n = 531 + 3 * d;                       // ragged
        std::vector<float> x = cloud(n, d);
        for (int k : {1, 5, 16}) {
            const float h1 = knn(x, n, d, k, 1, true);
            const float h0 = knn(x, n, d, k, 0, true);
            const float h7 = knn(x, n, d, k, 7, true);
            const float hm = knn(x, n, d, k, 400, true);     // chunks of two candidates
            check(h0 == h1 && h1 == h7 && h7 == hm, "H does not depend on the chunking");
        }
    }
    {   // duplicates, N = k + 1, all identical
        std::vector<float> x = cloud(300, 4);
        for (int i = 0; i < 50 * 4; ++i) x[200 * 4 + i] = x[i];
        knn(x, 300, 4, 1, 3, true);
        std::vector<float> same(17 * 6, 0.75f);
        knn(same, 17, 6, 16, 0, true);
        std::vector<float> two = {0.0f, 1.0f};
        knn(two, 2, 1, 1, 0, true);
    }
    {   // NaN and inf rows; a cloud where nobody has k finite neighbours
        std::vector<float> x = cloud(700, 6);
        x[345 * 6 + 2] = NAN;
        knn(x, 700, 6, 5, 3, false);
        x[345 * 6 + 2] = INFINITY;
        x[10 * 6] = -INFINITY;
        knn(x, 700, 6, 16, 0, false);
        std::vector<float> bad(20 * 3, NAN);
        knn(bad, 20, 3, 4, 2, false);
    }
    std::vector<float> x = cloud(64, 2), gx(128), rho2(64);
    std::vector<int32_t> idx(64);
    std::vector<double> ws(1 << 16);
    float H;
    double S;
    const float coef = 1.0f;
    check(mf_knn_entropy_ws_bytes(64, 2, 17, 0) < 0 && mf_knn_entropy_ws_bytes(64, 17, 5, 0) < 0, "k = 17, d = 17 refused");
    check(mf_knn_entropy_ws_bytes(5, 2, 5, 0) < 0 && mf_knn_entropy_ws_bytes(64, 2, 5, -1) < 0, "N = k, chunks = -1 refused");
    check(mf_knn_entropy_fwd(x.data(), 64, 2, 0, 0, &H, &S, idx.data(), rho2.data(), ws.data(), nullptr) != 0, "k = 0 refused");
    check(mf_knn_entropy_fwd(x.data(), 64, 2, 64, 0, &H, &S, idx.data(), rho2.data(), ws.data(), nullptr) != 0, "k = N refused");
    check(mf_knn_entropy_fwd(x.data(), 64, 2, 5, 0, &H, &S, idx.data(), rho2.data(), nullptr, nullptr) != 0, "no workspace");
    check(mf_knn_entropy_bwd(x.data(), 64, 0, idx.data(), rho2.data(), &coef, 1.0f, gx.data(), nullptr) != 0, "d = 0 refused");
    // the backward clamps indices it is handed from outside
    for (auto& j : idx) j = 1 << 30;
    for (auto& r : rho2) r = 1.0f;
    CK(mf_knn_entropy_bwd(x.data(), 64, 2, idx.data(), rho2.data(), &coef, 1.0f, gx.data(), nullptr));
}

static void cov_cases() {
    const float coef = 0.5f;
    for (int d : {1, 2, 6, 16}) {
        for (int64_t n : {(int64_t)2, (int64_t)37, (int64_t)1001, (int64_t)4099}) {
            std::vector<float> x = cloud(n, d);
            const int64_t nws = mf_cov_entropy_ws_doubles(n, d);
            check(nws > 0, "workspace size");
            std::vector<double> ws(nws), aux(d + d * d);
            std::vector<float> gx((size_t)n * d);
            float H = 0.0f;
            CK(mf_cov_entropy_fwd(x.data(), n, d, 1e-12, &H, aux.data(), ws.data(), nullptr));
            CK(mf_cov_entropy_bwd(x.data(), n, d, aux.data(), &coef, gx.data(), nullptr));
            if (n > d) {
                check(std::isfinite(H), "finite H");
                for (float g : gx) check(std::isfinite(g), "finite gradient");
            }
        }
    }
    {   // degenerate and non-finite clouds must not trip anything
        std::vector<float> x(200 * 3, 1.0f);
        std::vector<double> ws(mf_cov_entropy_ws_doubles(200, 3)), aux(12);
        std::vector<float> gx(600);
        float H;
        CK(mf_cov_entropy_fwd(x.data(), 200, 3, 1e-12, &H, aux.data(), ws.data(), nullptr));
        CK(mf_cov_entropy_bwd(x.data(), 200, 3, aux.data(), &coef, gx.data(), nullptr));
        check(std::isfinite(H), "a point mass has a finite padded H");
        x[7] = NAN;
        CK(mf_cov_entropy_fwd(x.data(), 200, 3, 1e-12, &H, aux.data(), ws.data(), nullptr));
        CK(mf_cov_entropy_bwd(x.data(), 200, 3, aux.data(), &coef, gx.data(), nullptr));
        check(!std::isfinite(H), "NaN input gives a non-finite H");
    }
    check(mf_cov_entropy_ws_doubles(1, 2) < 0 && mf_cov_entropy_ws_doubles(10, 17) < 0, "N = 1, d = 17 refused");
    float H;
    check(mf_cov_entropy_fwd(nullptr, 1, 2, 0.0, &H, nullptr, nullptr, nullptr) != 0, "N = 1 refused");
    check(mf_cov_entropy_bwd(nullptr, 10, 0, nullptr, nullptr, nullptr, nullptr) != 0, "d = 0 refused");
}

void sanitize_entropy() {
    seed(777u);
    knn_cases();
    cov_cases();
    printf("SANITIZE ENTROPY OK\n");
}
