// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
// Sliced-Wasserstein section of the sanitizer driver (mentflow_amd/csrc/swd.hip).  tests/emu/build_sanitize.sh links it into
// tests/emu/sanitize_emu (AddressSanitizer + UndefinedBehaviorSanitizer, the fiber emulator's exactly-sized, guard-paged
// dynamic LDS), whose main, in sanitize_main.cpp, calls sanitize_swd().  It calls the projection, the segmented sort and the
// quantile cost on the smallest shapes that reach every branch of the sort plan (one key, one tile, odd and even numbers of
// merge passes, ragged last tile, in place, the default tile) and of the cost kernels (equal and unequal sizes, swapped
// arguments, several chunks, p = 1, 2 and general, more directions than one LDS chunk), and the refusals.  Every buffer has
// exactly the documented size, so any out-of-range index or undefined arithmetic aborts.
#include "sanitize_common.h"

static std::vector<float> keys(size_t n) {
    std::vector<float> x(n);
    for (auto& v : x) v = 8.0f * (urand() - 0.5f);
    return x;
}

static void segsort(int P, int64_t n, int tile_log2, bool in_place, std::vector<float> k) {
    const int64_t bytes = mf_segsort_workspace_bytes(P, n, tile_log2);
    check(bytes >= 0, "workspace size");
    std::vector<unsigned char> ws((size_t)bytes);
    std::vector<float> sorted(in_place ? 0 : k.size(), NAN);
    float* out = in_place ? k.data() : sorted.data();
    CK(mf_segsort_f32(k.data(), P, n, tile_log2, out, bytes ? ws.data() : nullptr, nullptr));
    for (int s = 0; s < P; ++s)
        for (int64_t i = 1; i < n; ++i) {
            const float a = out[s * n + i - 1], b = out[s * n + i];
            check(std::isnan(b) || a <= b, "every row ascending, NaN last");
        }
}

static void sort_cases() {
    segsort(3, 1, 0, false, keys(3));                       // a single key
    check(mf_segsort_workspace_bytes(2, 16, 4) == 0, "one tile needs no workspace");
    segsort(2, 16, 4, false, keys(2 * 16));                 // exactly one tile, ws == NULL
    std::vector<float> k = keys(3 * 17);                    // 2 tiles, one (odd) pass
    k[3] = NAN;
    k[17 + 5] = -0.0f;
    k[17 + 6] = 0.0f;
    k[2 * 17 + 16] = INFINITY;
    segsort(3, 17, 4, true, k);
    k = keys(3 * 1000);                                     // 63 tiles, 6 passes, ragged last tile
    k[1000 + 999] = NAN;
    segsort(3, 1000, 4, false, k);
    segsort(2, 333, 5, true, keys(2 * 333));                // 11 tiles, 4 passes
    segsort(1, 300, 6, false, keys(300));                   // 5 tiles, 3 passes
    segsort(2, 5000, 0, false, keys(2 * 5000));             // default 2^12 tile, merge chunk 2048, ragged
    segsort(1, 9000, 12, true, keys(9000));                 // 3 tiles, 2 passes
}

// projection -> sort (in place, one tile per row where 2^12 keys hold it: fewest emulated threads) -> quantile cost
static void swd(int64_t n1, int64_t n2, int d, int P, float p) {
    std::vector<float> dir = keys((size_t)d * P);
    const std::vector<float> x[2] = {keys((size_t)n1 * d), keys((size_t)n2 * d)};
    const int64_t n[2] = {n1, n2};
    std::vector<float> u[2];
    for (int s = 0; s < 2; ++s) {
        u[s].assign((size_t)P * n[s], NAN);
        CK(mf_swd_project(x[s].data(), n[s], d, dir.data(), P, u[s].data(), nullptr));
        int tile_log2 = 4;
        while (tile_log2 < 12 && ((int64_t)1 << tile_log2) < n[s]) ++tile_log2;
        const int64_t bytes = mf_segsort_workspace_bytes(P, n[s], tile_log2);
        check(bytes >= 0, "workspace size");
        std::vector<unsigned char> ws((size_t)bytes);
        CK(mf_segsort_f32(u[s].data(), P, n[s], tile_log2, u[s].data(), bytes ? ws.data() : nullptr, nullptr));
    }
    std::vector<double> partial((size_t)mf_swd_cost_ws_doubles(P, n1, n2)), wpp(P);
    float dist = NAN;
    CK(mf_swd_quantile_cost(u[0].data(), n1, u[1].data(), n2, P, p, partial.data(), wpp.data(), &dist, nullptr));
    check(std::isfinite(dist), "finite distance");
}

void sanitize_swd() {
    seed(2024u);
    sort_cases();
    swd(300, 300, 6, 7, 2.0f);                              // equal sizes, the p = 2 fast path
    swd(257, 100, 1, 3, 1.0f);                              // unequal sizes, d = 1, the p = 1 fast path
    check(mf_swd_cost_ws_doubles(2, 100, 4500) == 2 * 2, "two cost chunks per projection");
    swd(100, 4500, 8, 2, 1.5f);                             // n2 > n1: swapped, two cost chunks, general p
    swd(64, 64, 3, 1100, 2.0f);                             // more directions than one chunk of LDS
    // refusals: no launch, an error instead
    std::vector<float> x = keys(16 * 9), u(16);
    check(mf_swd_project(x.data(), 16, 9, x.data(), 1, u.data(), nullptr) != 0, "d = 9 refused");
    check(mf_segsort_workspace_bytes(1, 8, 3) == -1, "tile_log2 = 3 refused");
    check(mf_segsort_f32(x.data(), 1, 16, 13, u.data(), nullptr, nullptr) != 0, "tile_log2 = 13 refused");
    printf("SANITIZE SWD OK\n");
}
