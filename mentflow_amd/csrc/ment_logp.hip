// Differentiable log-density of classical MENT on gfx950: logp(x) = sum_s log clamp(h_s(u_s(x)), 0, 1e10) + log prior(x) and
// its gradient with respect to x, for the slots of ment.hip (layout and density at the top of that file).  The reference has no
// counterpart: its interpolators are scipy on the host, and its log_prob is log(prob + pad) of the fp32 product, which leaves
// fp32's range with a hundred factors long before the log-density stops being meaningful.
//
// One lane per point.  x[d <= 8] and the gradient accumulators live in registers; descriptors (and the tables, under the rule
// of ment_slots.h) are staged in LDS once per workgroup, which then strides over the points.  Per slot, u and the cell (i, w)
// come from the fmaf chain and grid_pos of slot_product, so the support is bit for bit that of mf_ment_prob, slot order and
// early exit included: the first zero factor ends the row with -inf, the first NaN factor with NaN.
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
#include "ment_slots.h"

namespace mf {

constexpr int LOGP_RENORM = 16;        // slots between renormalisations of the running product (a mantissa is >= 1/2)

// h and, when GRAD, its partials along the slot's projected axes, from the arithmetic of slot_product
template <bool TAB_LDS, bool GRAD>
__device__ __forceinline__ float slot_value(const float (&xv)[MENT_DMAX], int d, const float* __restrict__ ds,
                                            const int* __restrict__ ms, const float* __restrict__ tab, float& h0, float& h1) {
    float u0 = 0.0f;
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j)
        if (j < d) u0 = fmaf(xv[j], ds[j], u0);
    const float* t = tab + ms[3];
    h0 = 0.0f;
    h1 = 0.0f;
    if (ms[0] == 1) {
        int i;
        float w;
        if (u0 != u0) return u0;
        if (!grid_pos(u0, ds[16], ds[17], ds[18], ms[1], i, w)) return 0.0f;
        const float a = t[i], b = t[i + 1];
        if (GRAD) h0 = (b - a) * ds[18];
        return a * (1.0f - w) + b * w;
    }
    float u1 = 0.0f;
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j)
        if (j < d) u1 = fmaf(xv[j], ds[8 + j], u1);
    int i, k;
    float wx, wy;
    const int By = ms[2];
    if (u0 != u0 || u1 != u1) return u0 + u1;
    if (!grid_pos(u0, ds[16], ds[17], ds[18], ms[1], i, wx) || !grid_pos(u1, ds[19], ds[20], ds[21], By, k, wy)) return 0.0f;
    const float* r0 = t + i * By + k;
    const float* r1 = r0 + By;
    const float v00 = r0[0], v01 = r0[1], v10 = r1[0], v11 = r1[1];
    if (GRAD) {
        h0 = ((v10 - v00) * (1.0f - wy) + (v11 - v01) * wy) * ds[18];
        h1 = ((v01 - v00) * (1.0f - wx) + (v11 - v10) * wx) * ds[21];
    }
    return v00 * ((1.0f - wx) * (1.0f - wy)) + v01 * ((1.0f - wx) * wy) + v10 * (wx * (1.0f - wy)) + v11 * (wx * wy);
}

template <bool TAB_LDS, bool GRAD>
__global__ __launch_bounds__(MENT_BLOCK) void ment_logprob_kernel(const float* __restrict__ x, int64_t n, int d, SlotArgs sa,
                                                                  float* __restrict__ logp, float* __restrict__ grad) {
    MF_DYN_SMEM(float, lds);
    float* desc;
    int* meta;
    const float* tab = stage_slots<TAB_LDS>(sa, lds, desc, meta);
    const float inv_a2 = sa.prior_kind == 1 ? 1.0f / (sa.prior_a * sa.prior_a) : 0.0f;
    for (int64_t p = (int64_t)blockIdx.x * MENT_BLOCK + threadIdx.x; p < n; p += (int64_t)gridDim.x * MENT_BLOCK) {
        float xv[MENT_DMAX], g[MENT_DMAX];
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j) {
            xv[j] = (j < d) ? x[p * d + j] : 0.0f;
            g[j] = 0.0f;
        }
        float m = 1.0f;                 // running product of the factors' mantissas; NaN once a factor was NaN
        int e = 0;                      // running sum of their exponents
        bool dead = false;              // a zero factor: logp = -inf
        for (int s = 0; s < sa.nslot; ++s) {
            const float* ds = desc + s * MENT_DESC;
            float h0, h1;
            const float h = clamp_factor(slot_value<TAB_LDS, GRAD>(xv, d, ds, meta + s * MENT_META, tab, h0, h1));
            if (h != h) {
                m = h;
                break;
            }
            if (h == 0.0f) {
                dead = true;
                break;
            }
            int eh;
            m *= frexpf(h, &eh);
            e += eh;
            if ((s & (LOGP_RENORM - 1)) == LOGP_RENORM - 1) {
                m = frexpf(m, &eh);
                e += eh;
            }
            if (GRAD) {
                const float r = h < 1.0e10f ? __frcp_rn(h) : 0.0f;      // on the upper clamp the factor is a constant
                const float c0 = h0 * r, c1 = h1 * r;
#pragma unroll
                for (int j = 0; j < MENT_DMAX; ++j)
                    if (j < d) g[j] = fmaf(c0, ds[j], g[j]);
                if (meta[s * MENT_META] == 2) {
#pragma unroll
                    for (int j = 0; j < MENT_DMAX; ++j)
                        if (j < d) g[j] = fmaf(c1, ds[8 + j], g[j]);
                }
            }
        }
        float lp;
        if (dead) {
            lp = -INFINITY;
        } else if (m != m) {
            lp = m;
        } else {
            int em;
            m = frexpf(m, &em);
            lp = fmaf((float)(e + em), 0.693147180559945f, logf(m));
            if (sa.prior_kind == 1) {               // prior.Gaussian.log_prob(x), the argument of prior_factor's exp
                float q = 0.0f;
#pragma unroll
                for (int j = 0; j < MENT_DMAX; ++j)
                    if (j < d) q = q + xv[j] * xv[j];
                lp += sa.prior_lognorm - (0.5f * q) / (sa.prior_a * sa.prior_a);
#pragma unroll
                for (int j = 0; j < MENT_DMAX; ++j) g[j] = fmaf(-xv[j], inv_a2, g[j]);
            } else if (sa.prior_kind == 2) {        // uniform density on [-a, a]^d
                bool inside = true;
#pragma unroll
                for (int j = 0; j < MENT_DMAX; ++j)
                    if (j < d) inside = inside && fabsf(xv[j]) <= sa.prior_a;
                lp = inside ? lp + sa.prior_lognorm : -INFINITY;
            }
        }
        logp[p] = lp;
        if (GRAD) {
            const bool out = lp == -INFINITY, nan = lp != lp;
#pragma unroll
            for (int j = 0; j < MENT_DMAX; ++j)
                if (j < d) grad[p * d + j] = out ? 0.0f : (nan ? lp : g[j]);
        }
    }
}

template <bool TAB_LDS, bool GRAD>
static void launch_logprob(int G, size_t smem, void* stream, const float* x, int64_t n, int d, const SlotArgs& sa, float* logp,
                           float* grad) {
    MF_ALLOW_DYN_SMEM((ment_logprob_kernel<TAB_LDS, GRAD>), smem);
    MF_LAUNCH((ment_logprob_kernel<TAB_LDS, GRAD>), G, MENT_BLOCK, smem, stream, x, n, d, sa, logp, grad);
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
    if (tl) {
        if (grad) launch_logprob<true, true>(G, smem, stream, x, n, d, sa, logp, grad);
        else launch_logprob<true, false>(G, smem, stream, x, n, d, sa, logp, grad);
    } else {
        if (grad) launch_logprob<false, true>(G, smem, stream, x, n, d, sa, logp, grad);
        else launch_logprob<false, false>(G, smem, stream, x, n, d, sa, logp, grad);
    }
    return check_launch("mf_ment_logprob");
}
