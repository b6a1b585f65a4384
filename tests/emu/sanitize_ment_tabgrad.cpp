// TEST INFRASTRUCTURE — NOT PRODUCT CODE.
// Table-gradient section of the sanitizer driver (mentflow_amd/csrc/ment_tabgrad.hip).  Like sanitize_ment_logp.cpp it runs from
// the constructor of a namespace-scope object of this translation unit, before main, and prints its own marker.  It calls
// mf_ment_logprob_tables_bwd on small synthetic inputs whose buffers have exactly the documented sizes: the LDS instance and the
// global one, d = 1, 3 and 8, grad_tab NULL and non-NULL, a point count that leaves the last workgroup of either instance ragged,
// NaN / inf rows, rows outside every hull with NaN weights, the poison rule, no points, and the refusals.
#include <cstring>

#include "sanitize_common.h"

static int tabgrad(const Slots& s, const std::vector<float>& x, int64_t n, int d, const std::vector<float>& logp,
                   const std::vector<float>& weight, std::vector<float>& grad_log, float* grad_tab) {
    const int64_t tf = (int64_t)s.tables.size();
    float wmax = 0.0f;
    for (int64_t i = 0; i < n; ++i)
        if (std::isfinite(logp[i])) wmax = std::isnan(weight[i]) ? NAN : std::fmax(wmax, std::fabs(weight[i]));
    std::vector<unsigned long long> acc(tf, 0xdeadbeefULL);
    int32_t status = -7;
    grad_log.assign(tf, NAN);
    CK(mf_ment_logprob_tables_bwd(x.data(), n, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), tf, logp.data(),
                                  weight.data(), &wmax, acc.data(), grad_log.data(), grad_tab, &status, nullptr));
    return status;
}

static void tabgrad_on(const Slots& s, int d) {
    const int64_t n = 1300;                                  // LDS instance: 1024 + 276 lanes; global: five workgroups and 20 lanes
    const int64_t tf = (int64_t)s.tables.size();
    std::vector<float> x((size_t)n * d);
    for (auto& v : x) v = 0.9f * nrand();
    for (int j = 0; j < d; ++j) x[(size_t)(n - 1) * d + j] = 25.0f;               // outside every hull
    x[(size_t)5 * d] = NAN;
    x[(size_t)6 * d + (d - 1)] = INFINITY;
    x[(size_t)7 * d] = -INFINITY;
    std::vector<float> logp(n, 0.0f), weight(n);
    CK(mf_ment_logprob(x.data(), n, d, s.n, s.desc.data(), s.meta.data(), s.tables.data(), tf, 0, 0.f, 0.f, logp.data(), nullptr,
                       nullptr));
    if (s.n > 0) check(std::isnan(logp[5]) && std::isinf(logp[n - 1]), "the NaN row and the row outside every hull");
    int64_t live = 0;
    for (int64_t i = 0; i < n; ++i) {
        weight[i] = nrand();
        if (std::isnan(logp[i])) weight[i] = 0.0f;            // masked by the caller
        if (std::isinf(logp[i]) && (i % 3) == 0) weight[i] = NAN;   // ignored whatever it is
        live += std::isfinite(logp[i]) ? 1 : 0;
    }
    check(live > 0, "some rows are inside the support");
    std::vector<float> gl, gl2, gt(tf, NAN);
    check(tabgrad(s, x, n, d, logp, weight, gl, gt.data()) == 0, "no poison");
    check(tabgrad(s, x, n, d, logp, weight, gl2, nullptr) == 0, "no poison without grad_tab");
    check(memcmp(gl.data(), gl2.data(), tf * sizeof(float)) == 0, "grad_tab == NULL gives the same grad_log bits");
    bool any = false;
    for (int64_t e = 0; e < tf; ++e) {
        check(std::isfinite(gl[e]) && std::isfinite(gt[e]), "finite outputs");
        if (!(s.tables[e] > 0.0f)) check(gt[e] == 0.0f && gl[e] == 0.0f, "a zero entry gets no gradient");
        any = any || gl[e] != 0.0f;
    }
    if (s.n > 0) check(any, "live rows contribute");
    // poison: a non-zero weight on the NaN row, a non-finite weight on a live row; the outputs stay finite
    std::vector<float> bad = weight;
    bad[5] = 1.0f;
    if (s.n > 0) check(tabgrad(s, x, n, d, logp, bad, gl2, gt.data()) != 0, "NaN logp with a non-zero weight poisons");
    for (int64_t e = 0; e < tf; ++e) check(std::isfinite(gl2[e]) && std::isfinite(gt[e]), "the kernel itself never writes NaN");
    bad = weight;
    for (int64_t i = 0; i < n; ++i)
        if (std::isfinite(logp[i])) {
            bad[i] = INFINITY;
            break;
        }
    check(tabgrad(s, x, n, d, logp, bad, gl2, gt.data()) != 0, "a non-finite weight on a live row poisons");
    for (int64_t e = 0; e < tf; ++e) check(std::isfinite(gl2[e]) && std::isfinite(gt[e]), "finite outputs under poison");
    // all weights zero: exact zeros
    std::vector<float> zero(n, 0.0f);
    check(tabgrad(s, x, n, d, logp, zero, gl2, gt.data()) == 0, "zero weights: no poison");
    for (int64_t e = 0; e < tf; ++e) check(gl2[e] == 0.0f && gt[e] == 0.0f, "zero weights give zeros");
    // no points
    check(tabgrad(s, x, 0, d, logp, weight, gl2, gt.data()) == 0, "no points: no poison");
    for (int64_t e = 0; e < tf; ++e) check(gl2[e] == 0.0f && gt[e] == 0.0f, "no points give zeros");
}

// (external for the reason given in sanitize_ment_logp.cpp)
void sanitize_ment_tabgrad() {
    seed(777u);
    for (int d = 1; d <= 8; d += d == 1 ? 2 : 5) {               // d = 1, 3, 8
        std::vector<int> small(3, 1);                              // 1-D slots; with d > 1 two 2-D slots join them
        if (d > 1) small.insert(small.begin() + 1, 2), small.push_back(2);
        tabgrad_on(make_slots(d, small, 12), d);                   // the LDS instance
        tabgrad_on(make_slots(d, std::vector<int>(3, 1), 11), d);  // 33 table floats: the image starts after a padding word
        if (d > 1) tabgrad_on(make_slots(d, std::vector<int>(2, 2), 85), d);   // 2 x 85^2 floats: the global instance
        else tabgrad_on(make_slots(d, std::vector<int>(130, 1), 85), d);       // 130 x 85 floats: beyond the LDS rule in 1-D
        tabgrad_on(make_slots(d, std::vector<int>(), 4), d);       // zero slots
    }
    Slots s = make_slots(3, std::vector<int>(1, 1), 8);
    std::vector<float> x(3 * 8, 0.1f), logp(8, 0.0f), w(8, 1.0f), gl(8), gt(8);
    std::vector<unsigned long long> acc(8);
    float wmax = 1.0f;
    int32_t status = 0;
    check(mf_ment_logprob_tables_bwd(x.data(), 8, 9, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, logp.data(), w.data(),
                                     &wmax, acc.data(), gl.data(), gt.data(), &status, nullptr) != 0, "d = 9 refused");
    check(mf_ment_logprob_tables_bwd(x.data(), -1, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), 8, logp.data(), w.data(),
                                     &wmax, acc.data(), gl.data(), gt.data(), &status, nullptr) != 0, "negative n refused");
    check(mf_ment_logprob_tables_bwd(x.data(), 8, 3, 513, s.desc.data(), s.meta.data(), s.tables.data(), 8, logp.data(), w.data(),
                                     &wmax, acc.data(), gl.data(), gt.data(), &status, nullptr) != 0, "513 slots refused");
    check(mf_ment_logprob_tables_bwd(x.data(), 8, 3, s.n, s.desc.data(), s.meta.data(), s.tables.data(), -1, logp.data(), w.data(),
                                     &wmax, acc.data(), gl.data(), gt.data(), &status, nullptr) != 0, "negative table size refused");
    printf("SANITIZE MENT TABGRAD OK\n");
    fflush(stdout);
}

namespace {
struct MentTabgradSection {
    MentTabgradSection() { sanitize_ment_tabgrad(); }
} ment_tabgrad_section;
}  // namespace
