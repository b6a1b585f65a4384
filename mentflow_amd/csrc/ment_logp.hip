// Differentiable log-density of classical MENT on gfx950: logp(x) = sum_s log clamp(h_s(u_s(x)), 0, 1e10) + log prior(x) and
// its gradient with respect to x, for the slots of ment.hip (layout and density at the top of that file).  The reference has no
// counterpart: its interpolators are scipy on the host, and its log_prob is log(prob + pad) of the fp32 product, which leaves
// fp32's range with a hundred factors long before the log-density stops being meaningful.
//
// One lane per point.  x[d <= 8] and the gradient accumulators live in registers; descriptors (and the tables, under the rule
// of ment_slots.h) are staged in LDS once per workgroup, which then strides over the points.  Per slot, the factor is
// slot_value of ment_slots.h, the function mf_ment_prob multiplies, so the support is bit for bit that of mf_ment_prob, slot
// order and early exit included: the first zero factor ends the row with -inf, the first NaN factor with NaN.
//
// Range.  No per-slot log: each factor is split into mantissa and exponent (frexpf: exact), the mantissas are multiplied into a
// running product in (2^-17, 1] that is renormalised every 16 slots, the exponents are summed in an integer, and one logf per
// point finishes: logp = E ln 2 + log(m).  The product carries half an ulp per factor (6e-6 after 100 factors, absolute in
// logp); where the fp32 product of mf_ment_prob would underflow or overflow, logp stays finite and as accurate.
//
// Gradient (template flag GRAD): grad = sum_s (h_s' / h_s) rows_s + d log prior / dx with the derivative of the cell grid_pos
// selects (the right derivative at an interior centre, the left one at the last centre), one v_rcp per slot.  A slot whose
// factor sits on the upper clamp (h >= 1e10) contributes nothing.  Rows with logp = -inf get the gradient 0 (nothing pulls a
// point that is outside the support), rows with logp = NaN get NaN.  Tables are constants.
//
// No atomics, no reductions: rows are independent and every output is bitwise reproducible.
#include "ment_logp_point.h"

namespace mf {

template <bool TAB_LDS, bool GRAD>
__global__ __launch_bounds__(MENT_BLOCK) void ment_logprob_kernel(const float* __restrict__ x, int64_t n, int d, SlotArgs sa,
                                                                  float* __restrict__ logp, float* __restrict__ grad) {
    MF_DYN_SMEM(float, lds);
    float* desc;
    int* meta;
    const float* tab = stage_slots<TAB_LDS>(sa, lds, desc, meta);
    const float inv_a2 = prior_inv_a2(sa);
    for (int64_t p = (int64_t)blockIdx.x * MENT_BLOCK + threadIdx.x; p < n; p += (int64_t)gridDim.x * MENT_BLOCK) {
        float xv[MENT_DMAX], g[MENT_DMAX];
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j) xv[j] = (j < d) ? x[p * d + j] : 0.0f;
        const float lp = logp_point<GRAD>(xv, d, desc, meta, tab, sa, inv_a2, g);     // ment_logp_point.h
        logp[p] = lp;
        if (GRAD) {
#pragma unroll
            for (int j = 0; j < MENT_DMAX; ++j)
                if (j < d) grad[p * d + j] = g[j];
        }
    }
}

}  // namespace mf

using namespace mf;

extern "C" int mf_ment_logprob(const float* x, int64_t n, int d, int nslot, const float* desc, const int32_t* meta,
                               const float* tables, int64_t table_floats, int prior_kind, float prior_a, float prior_lognorm,
                               float* logp, float* grad, void* stream) {
    size_t smem;
    bool tl;
    if (slot_geometry(d, nslot, table_floats, prior_kind, &smem, &tl)) return 1;
    if (n < 0) return fail("negative point count");
    if (n == 0) return 0;
    const SlotArgs sa = slot_args(nslot, desc, meta, tables, table_floats, prior_kind, prior_a, prior_lognorm);
    int64_t blocks = (n + MENT_BLOCK - 1) / MENT_BLOCK;
    if (blocks > NUM_CU * 16) blocks = NUM_CU * 16;
    const int G = (int)blocks;
    if (grad)
        MF_LAUNCH_TAB(tl, (ment_logprob_kernel<true, true>), (ment_logprob_kernel<false, true>), G, MENT_BLOCK, smem, stream, x, n,
                      d, sa, logp, grad);
    else
        MF_LAUNCH_TAB(tl, (ment_logprob_kernel<true, false>), (ment_logprob_kernel<false, false>), G, MENT_BLOCK, smem, stream, x,
                      n, d, sa, logp, grad);
    return check_launch("mf_ment_logprob");
}
