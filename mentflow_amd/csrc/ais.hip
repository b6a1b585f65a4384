// Annealed importance sampling (Neal 2001) on the density of classical MENT, on gfx950: the Langevin chains of mala.hip walked
// along a temperature ladder from a normalised Gaussian to the MENT density, each carrying the logarithm of its importance
// weight.  The mean of the weights estimates the normaliser Z of the density, which nothing else here can give without a grid of
// res^ndim cells.  The reference has no counterpart.
//
// The layout is that of mala.hip.  One lane per chain; the state x[d <= 8], lp = logp(x), g = grad logp(x) (logp_point<true>: the
// bits mf_ment_logprob returns), lq(x) and the log-weight live in registers for the whole launch; descriptors (and the tables,
// under the rule of ment_slots.h) are staged in LDS once per workgroup.  The base q0 = N(m, diag b^2) comes as host arrays and
// travels in the kernel arguments (scalar registers): m_j, ib_j = 1 / b_j (fp32 division on the host) and
// c0 = -sum log b_j - (d / 2) log 2 pi (formed in fp64, rounded once).
//
// fp32 operation order (this file is compiled with contraction off in its own code, so every line below is one rounding per
// operation, and tests/_ais_fp64.py restates it; logp_point keeps the form and the bits it has in ment_logp.hip):
//   t_j   = (x_j - m_j) * ib_j
//   lq(x) = c0 - 0.5 * q,          q = (..((0 + t_0 t_0) + t_1 t_1) + ..) + t_{d-1} t_{d-1}
//   gq_j  = -(t_j * ib_j)
//   l_b   = b > 0 ? lq + b * (lp - lq) : lq            (b == 0: lq whatever lp is, no 0 * -inf)
//   gb_j  = l_b == -inf ? 0 : (b > 0 ? gq_j + b * (g_j - gq_j) : gq_j)
// l_b == -inf exactly where b > 0 and lp == -inf: such a chain has no drift, as in mala.hip.  A transition is the one
// ment_langevin.h states (fp32 operation order, acceptance rule, conventions) with l -> l_b and g -> gb.  It is spelt out in the
// kernel below and does not go through langevin_step: on a tempered target that form compiled to one VGPR more in the <true>
// instantiation (106 against 105).  A change to the rule is made there AND here; tests/_mala_fp64.py judges both with one verifier.
//
// Per temperature k = temp_offset + 1 .. temp_offset + ntemps, with b_k = betas[k]:
//   weight:  logw += b_k == b_{k-1} ? 0 : (lp > -inf ? (b_k - b_{k-1}) * (lp - lq) : -inf)     (fp32 increment, fp64 sum)
//   move:    steps_per_temp transitions on l_{b_k}.
// The increment is never NaN (a NaN lp counts as outside), so logw may reach -inf and never NaN.  lp, g and lq are recomputed
// from x at entry: nothing but x and logw crosses a launch, nothing in a chain depends on another chain or on where the ladder is
// cut, and a ladder cut into several launches gives the bits of one launch.  No atomics.
#include "ment_langevin.h"

namespace mf {

// The ChainArgs fields (chain_args fills them, chain_noise and chain_keep read them) and what the ladder adds.
struct AisArgs {
    const float* noise;     // [ntemps * steps_per_temp][d + 1][chains]
    const float* scale;     // [d] proposal scale per axis
    float* out;             // [total transitions][chains][d] or null: the state after every transition (row = global index)
    float* logp;            // [chains] or null: logp of the final states
    int64_t steps;          // ntemps * steps_per_temp
    int64_t keep_t;         // as in ChainArgs
    int64_t keep_row;
    int64_t keep_every;
    int chains;
    int d;
    float drift_clip;
    const float* betas;     // the ladder; this launch reads betas[temp_offset .. temp_offset + ntemps]
    double* logw;           // [chains], in and out
    int64_t ntemps;
    int64_t temp_offset;
    int steps_per_temp;
    float c0;
    float mean[MENT_DMAX];
    float inv_b[MENT_DMAX];
};

// lq at v, and t_j = (v_j - m_j) * ib_j for the gradient
__device__ __forceinline__ float ais_base(const float (&v)[MENT_DMAX], const AisArgs& aa, float (&t)[MENT_DMAX]) {
#pragma clang fp contract(off)
    float q = 0.0f;
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j) {
        t[j] = 0.0f;
        if (j < aa.d) {
            t[j] = (v[j] - aa.mean[j]) * aa.inv_b[j];
            const float tt = t[j] * t[j];
            q = q + tt;
        }
    }
    const float h = 0.5f * q;
    return aa.c0 - h;
}

__device__ __forceinline__ float ais_temper(float beta, float lp, float lq) {
#pragma clang fp contract(off)
    if (!(beta > 0.0f)) return lq;
    const float w = beta * (lp - lq);
    return lq + w;
}

// gb_j from t_j of ais_base, g_j of logp_point and l_b of ais_temper
__device__ __forceinline__ float ais_grad(float beta, float lb, float g, float t, float ib) {
#pragma clang fp contract(off)
    const float gq = -(t * ib);
    if (lb == -INFINITY) return 0.0f;
    if (!(beta > 0.0f)) return gq;
    const float w = beta * (g - gq);
    return gq + w;
}

template <bool TAB_LDS>
__global__ __launch_bounds__(MENT_BLOCK) void ais_ment_steps_kernel(float* __restrict__ x, AisArgs aa, SlotArgs sa,
                                                                    int* __restrict__ accepted) {
    MF_DYN_SMEM(float, lds);
    float* desc;
    int* meta;
    const float* tab = stage_slots<TAB_LDS>(sa, lds, desc, meta);
    const int c = blockIdx.x * MENT_BLOCK + threadIdx.x;
    if (c >= aa.chains) return;                       // after the barrier of stage_slots
    const int d = aa.d;
    const float clip = aa.drift_clip;
    const float inv_a2 = prior_inv_a2(sa);
    float xv[MENT_DMAX], sc[MENT_DMAX], g[MENT_DMAX], tx[MENT_DMAX];
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j) {
        xv[j] = (j < d) ? x[(int64_t)c * d + j] : 0.0f;
        sc[j] = (j < d) ? aa.scale[j] : 0.0f;
    }
    float lp = logp_point<true>(xv, d, desc, meta, tab, sa, inv_a2, g);
    float lq = ais_base(xv, aa, tx);
    double lw = aa.logw[c];
    int acc = 0;
    const int64_t row = aa.chains;                     // floats per noise row
    int64_t keep_t = aa.keep_t, keep_row = aa.keep_row;
    int64_t t = 0;
    float beta_prev = aa.betas[aa.temp_offset];
    for (int64_t k = 1; k <= aa.ntemps; ++k) {
        const float beta = aa.betas[aa.temp_offset + k];
        if (beta != beta_prev) {
            const float inc = lp > -INFINITY ? (beta - beta_prev) * (lp - lq) : -INFINITY;
            lw += (double)inc;
        }
        beta_prev = beta;
        for (int i = 0; i < aa.steps_per_temp; ++i, ++t) {
            const float* nz = chain_noise(aa, t, c);
            const float lb = ais_temper(beta, lp, lq);
            float yv[MENT_DMAX], gy[MENT_DMAX], ty[MENT_DMAX];
            float zz = 0.0f;
#pragma unroll
            for (int j = 0; j < MENT_DMAX; ++j) {
                yv[j] = 0.0f;
                if (j < d) {
                    const float z = nz[j * row];
                    const float gb = ais_grad(beta, lb, g[j], tx[j], aa.inv_b[j]);
                    yv[j] = fmaf(sc[j], z, xv[j] + langevin_drift(gb, sc[j], clip));
                    zz = fmaf(z, z, zz);
                }
            }
            const float u = nz[d * row];
            const float lp_new = logp_point<true>(yv, d, desc, meta, tab, sa, inv_a2, gy);
            const float lq_new = ais_base(yv, aa, ty);
            const float lb_new = ais_temper(beta, lp_new, lq_new);
            float rr = 0.0f;
#pragma unroll
            for (int j = 0; j < MENT_DMAX; ++j) {
                if (j < d) {
                    const float gb = ais_grad(beta, lb_new, gy[j], ty[j], aa.inv_b[j]);
                    const float r = ((xv[j] - yv[j]) - langevin_drift(gb, sc[j], clip)) / sc[j];
                    rr = fmaf(r, r, rr);
                }
            }
            const float delta = (lb_new - lb) + 0.5f * (zz - rr);
            bool accept = lb_new > -INFINITY ? (lb == -INFINITY || logf(u) < delta) : (lb_new == -INFINITY && lb == -INFINITY);
            accept = accept && u == u && zz == zz;     // NaN noise never moves a chain, wherever the chain is
#pragma unroll
            for (int j = 0; j < MENT_DMAX; ++j) {
                xv[j] = accept ? yv[j] : xv[j];
                g[j] = accept ? gy[j] : g[j];
                tx[j] = accept ? ty[j] : tx[j];
            }
            lp = accept ? lp_new : lp;
            lq = accept ? lq_new : lq;
            acc += accept ? 1 : 0;
            chain_keep(aa, t, c, xv, keep_t, keep_row);
        }
    }
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j)
        if (j < d) x[(int64_t)c * d + j] = xv[j];
    aa.logw[c] = lw;
    accepted[c] += acc;
    if (aa.logp != nullptr) aa.logp[c] = lp;
}

}  // namespace mf

using namespace mf;

extern "C" int mf_ais_ment_steps(float* x, int64_t chains, int d, int nslot, const float* desc, const int32_t* meta,
                                 const float* tables, int64_t table_floats, int prior_kind, float prior_a, float prior_lognorm,
                                 const float* noise, const float* betas, int64_t nbetas, int64_t ntemps, int64_t temp_offset,
                                 int64_t steps_per_temp, const float* scale, float drift_clip, const float* base_mean,
                                 const float* base_scale, double* logw, float* out, int32_t* accepted, float* logp,
                                 void* stream) {
    size_t smem;
    bool tl;
    if (slot_geometry(d, nslot, table_floats, prior_kind, &smem, &tl)) return 1;
    const int64_t lim = (int64_t)1 << 20;              // ntemps * steps_per_temp stays within chain_args' 2^40
    if (ntemps < 0 || temp_offset < 0 || ntemps > lim || temp_offset > lim)
        return fail("ais: 0 <= ntemps, temp_offset <= 2^20 expected (got %lld, %lld)", (long long)ntemps, (long long)temp_offset);
    if (steps_per_temp < 0 || steps_per_temp > lim)
        return fail("ais: 0 <= steps_per_temp <= 2^20 expected (got %lld)", (long long)steps_per_temp);
    if (temp_offset + ntemps + 1 > nbetas)
        return fail("ais: temperatures %lld .. %lld lie beyond the ladder's %lld entries", (long long)temp_offset,
                    (long long)(temp_offset + ntemps), (long long)nbetas);
    AisArgs aa;
    if (chain_args("ais", chains, d, noise, ntemps * steps_per_temp, temp_offset * steps_per_temp, scale, 0, 1, out, &aa))
        return 1;
    if (!(drift_clip >= 0.0f)) return fail("ais: drift_clip must be >= 0 (got %g)", (double)drift_clip);
    if (logw == nullptr && chains > 0) return fail("ais: logw must not be null");
    if (base_mean == nullptr || base_scale == nullptr) return fail("ais: base_mean and base_scale must not be null");
    double c0 = -0.5 * d * 1.8378770664093453;         // log 2 pi
    for (int j = 0; j < MENT_DMAX; ++j) {
        aa.mean[j] = 0.0f;
        aa.inv_b[j] = 0.0f;
        if (j >= d) continue;
        if (!(base_scale[j] > 0.0f) || !(base_scale[j] <= 3.0e38f) || !(base_mean[j] == base_mean[j]))
            return fail("ais: base_scale must be > 0 and finite, base_mean not NaN (axis %d: %g, %g)", j, (double)base_scale[j],
                        (double)base_mean[j]);
        aa.mean[j] = base_mean[j];
        aa.inv_b[j] = 1.0f / base_scale[j];
        c0 -= std::log((double)base_scale[j]);
    }
    if (chains == 0 || ntemps == 0) return 0;
    const SlotArgs sa = slot_args(nslot, desc, meta, tables, table_floats, prior_kind, prior_a, prior_lognorm);
    aa.logp = logp;
    aa.drift_clip = drift_clip;
    aa.betas = betas;
    aa.logw = logw;
    aa.ntemps = ntemps;
    aa.temp_offset = temp_offset;
    aa.steps_per_temp = (int)steps_per_temp;
    aa.c0 = (float)c0;
    const int G = (int)((chains + MENT_BLOCK - 1) / MENT_BLOCK);
    MF_LAUNCH_TAB(tl, ais_ment_steps_kernel<true>, ais_ment_steps_kernel<false>, G, MENT_BLOCK, smem, stream, x, aa, sa,
                  accepted);
    return check_launch("mf_ais_ment_steps");
}
