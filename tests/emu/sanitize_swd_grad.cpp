// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
// Gradient section of the sanitizer driver for mentflow_amd/csrc/swd.hip: the pair sort, the adjoint of the quantile cost and
// the back-projection.  tests/emu/build_sanitize.sh links every tests/emu/sanitize_*.cpp into tests/emu/sanitize_emu; main (in
// sanitize_main.cpp) knows nothing of this section, so it runs from the constructor of a namespace-scope object of this
// translation unit, before main, and prints its own marker.  That is sound because nothing it reaches depends on another
// translation unit's dynamic initialisation: the emulator's scheduler state is a null pointer and four dim3 that every launch
// overwrites, its stack pool is function-local, the library's error text is a constant-initialised thread_local array, and
// the kernels' __shared__ arrays are zero-initialised function-local statics.
// Shapes: the smallest that reach every branch: one key, one tile, 2 / 11 / 63 ragged tiles and both workspace layouts of the
// pair sort, rows of NaN / inf / signed zeros; equal and unequal sizes of the cost adjoint with lane groups of 2 .. 256, both
// argument orders, p = 1, 2 and general, with and without the fused un-sort, one side left out, identical clouds; one and two
// chunks of directions in the back-projection.  Every buffer has exactly the documented size.
#include <algorithm>
#include <cstring>

#include "sanitize_common.h"

static std::vector<float> keys(size_t n) {
    std::vector<float> x(n);
    for (auto& v : x) v = 8.0f * (urand() - 0.5f);
    return x;
}

static uint32_t bits(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

// sorts k[P, n] into (out, perm) and checks them: rows ascending with NaN last, perm a permutation, keys[perm] == out bitwise
static void pair_sort(int P, int64_t n, int tile_log2, bool in_place, std::vector<float> k, std::vector<float>* sorted = nullptr,
                      std::vector<int32_t>* positions = nullptr) {
    const std::vector<float> input = k;
    const int64_t bytes = mf_segsort_pairs_workspace_bytes(P, n, tile_log2);
    check(bytes >= 0, "size of the pair sort scratch");
    std::vector<unsigned char> ws((size_t)bytes);
    std::vector<float> other(in_place ? 0 : k.size(), NAN);
    std::vector<int32_t> perm(k.size(), -1);
    float* out = in_place ? k.data() : other.data();
    CK(mf_segsort_pairs_f32(k.data(), P, n, tile_log2, out, perm.data(), bytes ? ws.data() : nullptr, nullptr));
    for (int s = 0; s < P; ++s) {
        std::vector<char> seen((size_t)n, 0);
        for (int64_t r = 0; r < n; ++r) {
            const int32_t q = perm[s * n + r];
            check(q >= 0 && q < n && !seen[q], "perm is a permutation");
            seen[q] = 1;
            check(bits(input[s * n + q]) == bits(out[s * n + r]), "keys[perm] == out bitwise");
            if (r > 0) check(std::isnan(out[s * n + r]) || out[s * n + r - 1] <= out[s * n + r], "every row ascending, NaN last");
        }
    }
    if (sorted) sorted->assign(out, out + k.size());
    if (positions) *positions = perm;
}

static void sort_cases() {
    pair_sort(3, 1, 0, false, keys(3));                     // a single key
    check(mf_segsort_pairs_workspace_bytes(2, 16, 4) == 0, "one tile needs no workspace");
    pair_sort(2, 16, 4, true, keys(2 * 16));                // exactly one tile, ws == NULL, in place
    check(mf_segsort_pairs_workspace_bytes(3, 17, 4) == 8 * 3 * 17 + 4 * 3 * 2, "one pass: one buffer of composites and the splits");
    pair_sort(3, 17, 4, false, keys(3 * 17));               // 2 tiles, one pass
    check(mf_segsort_pairs_workspace_bytes(2, 333, 5) == 2 * 8 * 2 * 333 + 4 * 2 * 11, "several passes: two buffers");
    pair_sort(2, 333, 5, true, keys(2 * 333));              // 11 tiles, 4 passes
    std::vector<float> k = keys(3 * 1000);                  // 63 tiles, 6 passes, ragged last tile
    for (int i = 0; i < 1000; i += 7) k[1000 + i] = k[1000 + (i * 13) % 1000];          // duplicates: ties go by position
    pair_sort(3, 1000, 4, false, k);
    // a row of NaN, +-inf, +-0 and nothing else (the NaN in the bits the sort writes back, so that the comparison is bitwise)
    float qnan;
    const uint32_t qnan_bits = 0x7FFFFFFFu;
    memcpy(&qnan, &qnan_bits, 4);
    const float pool[5] = {qnan, INFINITY, -INFINITY, 0.0f, -0.0f};
    k.assign(2 * 100, 0.0f);
    for (size_t i = 0; i < k.size(); ++i) k[i] = pool[(size_t)(urand() * 5.0f) % 5];
    pair_sort(2, 100, 4, false, k);
    pair_sort(2, 100, 0, true, k);
    pair_sort(2, 5000, 0, false, keys(2 * 5000));           // the built-in tile: 2 tiles, merge chunk 2048
    pair_sort(1, 9000, 12, true, keys(9000));               // 3 tiles, 2 passes
}

static void all_finite(const std::vector<float>& v, const char* what) {
    for (float x : v) check(std::isfinite(x), what);
}

// sorted rows -> cost -> its adjoint: both sides, each side alone, with the un-sort fused into the store, identical clouds
static void cost_bwd(int64_t n1, int64_t n2, int P, float p) {
    std::vector<float> u, v;
    std::vector<int32_t> pu, pv;
    const int64_t n[2] = {n1, n2};
    std::vector<float>* rows[2] = {&u, &v};
    std::vector<int32_t>* perms[2] = {&pu, &pv};
    for (int s = 0; s < 2; ++s) {
        int tile_log2 = 4;
        while (tile_log2 < 12 && ((int64_t)1 << tile_log2) < n[s]) ++tile_log2;
        pair_sort(P, n[s], tile_log2, true, keys((size_t)P * n[s]), rows[s], perms[s]);
    }
    std::vector<double> partial((size_t)mf_swd_cost_ws_doubles(P, n1, n2)), wpp(P);
    float dist = NAN;
    const float gdist = 0.75f;
    CK(mf_swd_quantile_cost(u.data(), n1, v.data(), n2, P, p, partial.data(), wpp.data(), &dist, nullptr));
    std::vector<float> gu(u.size(), NAN), gv(v.size(), NAN), su(u.size(), NAN), sv(v.size(), NAN), only(std::max(u.size(), v.size()));
    CK(mf_swd_quantile_cost_bwd(u.data(), n1, nullptr, v.data(), n2, nullptr, P, p, wpp.data(), &gdist, gu.data(), gv.data(), nullptr));
    all_finite(gu, "gu finite, every entry written");
    all_finite(gv, "gv finite, every entry written");
    CK(mf_swd_quantile_cost_bwd(u.data(), n1, pu.data(), v.data(), n2, pv.data(), P, p, wpp.data(), &gdist, su.data(), sv.data(), nullptr));
    for (size_t s = 0; s < (size_t)P; ++s) {
        for (int64_t r = 0; r < n1; ++r) check(bits(su[s * n1 + pu[s * n1 + r]]) == bits(gu[s * n1 + r]), "gu lands at perm");
        for (int64_t r = 0; r < n2; ++r) check(bits(sv[s * n2 + pv[s * n2 + r]]) == bits(gv[s * n2 + r]), "gv lands at perm");
    }
    only.assign(u.size(), NAN);
    CK(mf_swd_quantile_cost_bwd(u.data(), n1, nullptr, v.data(), n2, nullptr, P, p, wpp.data(), &gdist, only.data(), nullptr, nullptr));
    check(memcmp(only.data(), gu.data(), 4 * gu.size()) == 0, "gu alone is the same bits");
    only.assign(v.size(), NAN);
    CK(mf_swd_quantile_cost_bwd(u.data(), n1, pu.data(), v.data(), n2, nullptr, P, p, wpp.data(), &gdist, nullptr, only.data(), nullptr));
    check(memcmp(only.data(), gv.data(), 4 * gv.size()) == 0, "gv alone is the same bits");
    if (n1 == n2) {                                         // identical clouds: M == 0, zero gradients
        CK(mf_swd_quantile_cost(u.data(), n1, u.data(), n1, P, p, partial.data(), wpp.data(), &dist, nullptr));
        check(dist == 0.0f, "identical clouds are at distance 0");
        CK(mf_swd_quantile_cost_bwd(u.data(), n1, pu.data(), u.data(), n1, nullptr, P, p, wpp.data(), &gdist, gu.data(), gv.data(), nullptr));
        for (size_t i = 0; i < gu.size(); ++i) check(gu[i] == 0.0f && gv[i] == 0.0f, "M == 0 gives zero gradients");
    }
}

static void project_bwd(int64_t n, int d, int P) {
    const std::vector<float> g = keys((size_t)P * n), dir = keys((size_t)d * P);
    std::vector<float> gx((size_t)n * d, NAN);
    CK(mf_swd_project_bwd(g.data(), n, d, dir.data(), P, gx.data(), 0, nullptr));
    all_finite(gx, "gx finite, every entry written");
    const std::vector<float> first = gx;
    CK(mf_swd_project_bwd(g.data(), n, d, dir.data(), P, gx.data(), 1, nullptr));
    for (size_t i = 0; i < gx.size(); ++i) check(gx[i] == first[i] + first[i], "accumulate adds onto the buffer");
}

// The section itself, with external linkage like the other sections' entry functions: keep it so.  A translation unit without
// a strong symbol has no unique module name for AddressSanitizer, which then keeps every instrumented global of the unit in one
// section; there this compiler puts some labels in front of their alignment padding, and the binary stops at start-up with a
// false odr-violation report on a string literal of this file.
void sanitize_swd_grad() {
    if (mf_is_emulation() != 1) return;                 // main reports that
    seed(4242u);
    sort_cases();
    for (float p : {1.0f, 1.5f, 2.0f}) {
        cost_bwd(300, 300, 3, p);                       // equal sizes: both sides in one launch
        cost_bwd(257, 100, 2, p);                       // lane groups of 4
        cost_bwd(100, 4500, 2, p);                      // swapped, two chunks of the larger set, lane groups of 64
        cost_bwd(2, 4097, 2, p);                        // lane groups of 256, 9 strides each
        cost_bwd(4097, 1, 2, p);                        // the whole segment meets one element
    }
    project_bwd(300, 1, 7);
    project_bwd(300, 8, 7);
    project_bwd(70, 1, 1100);                           // two chunks of directions
    project_bwd(70, 8, 1100);
    // refusals: no launch, an error instead
    std::vector<float> x = keys(16 * 9), y(16 * 9);
    std::vector<int32_t> perm(16);
    std::vector<double> wpp(1, 1.0);
    const float gdist = 1.0f;
    check(mf_swd_project_bwd(x.data(), 16, 9, x.data(), 1, y.data(), 0, nullptr) != 0, "d = 9 refused");
    check(mf_segsort_pairs_workspace_bytes(1, 8, 3) == -1, "tile_log2 = 3 refused");
    check(mf_segsort_pairs_f32(x.data(), 1, 16, 3, y.data(), perm.data(), nullptr, nullptr) != 0, "tile_log2 = 3 refused");
    check(mf_segsort_pairs_f32(x.data(), 1, 16, 4, y.data(), nullptr, nullptr, nullptr) != 0, "perm is required");
    check(mf_swd_quantile_cost_bwd(x.data(), 16, nullptr, x.data(), 16, nullptr, 1, 0.5f, wpp.data(), &gdist, y.data(), nullptr,
                                   nullptr) != 0, "p < 1 refused");
    printf("SANITIZE SWD GRAD OK\n");
    fflush(stdout);
}

namespace {
struct SwdGradSection {
    SwdGradSection() { sanitize_swd_grad(); }
} swd_grad_section;
}  // namespace
