/* mentflow_hip.h — C ABI of libmentflow_hip.so, the MI355X (gfx950) implementation of the MENT-Flow hot path.
 *
 * The reference (austin-hoover/ment-flow) is pure Python: it has no FFI of its own.  Each entry point below
 * replaces the chain of eager PyTorch ops cited next to it (paths relative to the reference repository);
 * INTEGRATION.md shows the ctypes stub a maintainer would add on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless stated otherwise; float = IEEE binary32; row-major.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises.
 *   - return value: 0 on success, non-zero on error (mf_last_error() gives the message, thread-local).
 *   - no entry point allocates: scratch is passed in by the caller (sizes from the *_floats helpers).
 */
#ifndef MENTFLOW_HIP_H
#define MENTFLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MF_ABI_VERSION 5
#define MF_ENTROPY_SCRATCH_DOUBLES 2048

int mf_abi_version(void);
const char* mf_last_error(void);
/* 0 for the gfx950 library.  (1 only for the host-emulated kernel build under tests/emu, which is test
 * infrastructure and is never loaded by the product package.)                                               */
int mf_is_emulation(void);

/* Per-kernel timing for bench.py: while enabled, every launch of the kernels listed below is bracketed by HIP
 * events recorded on its own stream.  mf_prof_report(id) synchronises those events and returns the summed
 * duration (ms) and the number of launches.  ids: 0 flow layer fwd, 1 flow layer bwd, 2 parameter-gradient
 * contraction (outer_accum), 3 kde1d fwd, 4 kde1d bwd, 5 kde2d fwd, 6 kde2d bwd.                              */
int mf_prof_enable(int enable);
int mf_prof_report(int kernel_id, double* total_ms, int64_t* launches);

/* ------------------------------------------------------------------------------------------------------------
 * Generic index gather (weight packing / gradient unpacking for the flow kernels).
 *   dst[j] = idx[j] >= 0 ? src[idx[j]] : 0        (accumulate != 0:  dst[j] += ...)
 * Replaces `mask * weight` in zuko.nn.MaskedLinear.forward (masked-out entries have idx = -1) and the
 * reshape/permute of conditioner outputs (zuko MaskedAutoregressiveTransform.meta).                          */
int mf_gather_f32(const float* src, const int32_t* idx, float* dst, int64_t n, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Autoregressive rational-quadratic-spline flow layer  (zuko NSF layer as inverted by
 * mentflow/generate/build.py:42-43; sampling direction of mentflow/generate/flows/zuko.py:24-29).
 *
 * `image` is the packed per-layer weight image (mf_flow_image_floats floats), laid out exactly as it sits in
 * LDS: [W0 64 x S0][b0 64]{[W_l 64 x 65][b_l 64]}(hidden_layers-1)[W_out d x 64 x 65][b_out d x 64];
 * see mentflow_amd/generate/packing.py for the row permutation of W_out.  hidden width is 64.
 *
 * fwd:  y[n,d] = RQS(x; MLP(x)),   logp_out[n] = (init_logp ? logN(x) : logp_in[n]) - sum_i ladj_i
 *       (logN(x) = -1/2 |x|^2 - d/2 log 2pi: zuko DiagNormal.log_prob of the base draw, first layer only).
 * order: HOST pointer to the d autoregressive orders of this layer (zuko `order` buffer), or NULL.  With it the kernels
 *       skip the MFMA k-steps that only multiply masked-out (zero) weights — the image must then hold the hidden
 *       units sorted by dependency class as packing.py lays them out; NULL = dense products (any image).
 * bwd:  given gy[n,d] = dL/dy and glogp[n] = dL/dlogp, writes gx[n,d] = dL/dx (NULL for the first layer: the
 *       base draw needs no gradient) and the parameter gradients dL/d(image) as PARTIAL SUMS, one per workgroup, into
 *       the rows of gslab[slab_rows][mf_flow_image_floats] (image layout per row) with plain stores — no float
 *       atomics, so the result is bitwise reproducible.  slab_rows must equal mf_flow_bwd_slab_rows(n, ...) (the
 *       number of workgroup columns this call launches).  accumulate = 0: every row is overwritten (first chunk of a
 *       backward pass: no zeroing needed); accumulate != 0: each workgroup adds to its own row (later chunks of the
 *       same size class).  mf_flow_grad_reduce sums the rows in a fixed order into the flat parameter gradient.
 *       `scratch` needs mf_flow_bwd_scratch_floats(n,...,order) floats: 0 when the call takes the fused kernel
 *       (parameter gradients inside the backward kernel: large batches with `order`), else (2 hidden_layers + d) * 64
 *       floats per particle for the hand-off to the parameter-gradient kernel (callers then process the batch in
 *       chunks to bound it).                                                                                    */
int64_t mf_flow_image_floats(int d, int hidden_layers);
/* Spline bins: 20 (the reference's value, experiments/setup.py:119-121) and 8 (zuko's default) are compile-time instances;
 * every other 2 <= bins <= 21 runs through a run-time instance whose last-layer block is laid out for 21 bins.  Returns the
 * slot (0..31) of a lane half's first derivative logit in the packed block — `bins` for the compile-time instances, 21
 * for the run-time one — or -1 if there is no kernel for that number of bins (the packer needs it: packing.py).        */
int mf_flow_rqs_deriv_slot(int bins);
/* Backward variant of the flow layers: -1 = default (environment variable MENTFLOW_BWD_FUSED, read once; unset = fused),
 * 0 = two-kernel path (backward + parameter-gradient contraction through an HBM scratch), 1 = fused kernel.  Process-wide;
 * tests use it to run both variants in one process.                                                                */
int mf_flow_set_bwd_variant(int variant);
int64_t mf_flow_bwd_scratch_floats(int64_t n, int d, int hidden_layers, const int32_t* order);
int mf_flow_rqs_layer_fwd(const float* image, int d, int hidden_layers, int bins, const int32_t* order,
                          const float* x, int64_t n, float* y, const float* logp_in, float* logp_out, int init_logp,
                          void* stream);
int mf_flow_bwd_slab_rows(int64_t n, int d, int hidden_layers, const int32_t* order);
int mf_flow_rqs_layer_bwd(const float* image, int d, int hidden_layers, int bins, const int32_t* order,
                          const float* x, int64_t n, const float* gy, const float* glogp, float* gx, float* gslab,
                          int slab_rows, int accumulate, float* scratch, int64_t scratch_floats, void* stream);

/* Activation hand-off from the training forward to the fused backward (ABI 4).  The eager reference keeps every activation
 * of zuko's conditioner for autograd (reached from mentflow/generate/flows/zuko.py:24-26).  mf_flow_rqs_layer_fwd saves nothing
 * (evaluation / no-grad; its backward mf_flow_rqs_layer_bwd recomputes the conditioner); mf_flow_rqs_layer_fwd_save is the same
 * forward that ALSO writes, per 32-particle tile, conditioner activations into `act` in the register layout of the fused
 * backward kernel:
 *   level 1: the post-ReLU hidden tiles of levels 1 .. hidden_layers-1 (level 0 is 8 MFMAs from the layer input: recomputed)
 *            64 floats per particle and level:                                                  512 B at hidden_layers = 3
 *   level 2: level 1 + the conditioner outputs (spline logits) of the d-1 features that have a conditioner, the 3 bins / 2
 *            slots per lane half the spline reads:                            + 240 (d-1) B at 20 bins: 1 712 B at d = 6
 * and mf_flow_rqs_layer_bwd_saved is the fused backward that loads them instead of re-running the conditioner's forward
 * chains (a quarter of that MFMA-bound kernel).  `act` holds mf_flow_rqs_act_floats(n, d, hidden_layers, bins, level) floats
 * per layer and belongs to ONE (layer, batch) pair: forward writes it, the backward of the same layer and particles reads it.
 * mf_flow_rqs_act_level(...) = highest level the built kernels take for the configuration under the current backward variant:
 * 2 with `order`, d <= 6 and bins in {20, 8}; 0 otherwise (two-kernel backward, run-time-bins instance) — callers then use
 * mf_flow_rqs_layer_fwd / _bwd.  Gradients are bitwise identical at every level (same arithmetic on the same values).      */
int mf_flow_rqs_act_level(int d, int hidden_layers, int bins, const int32_t* order);
int64_t mf_flow_rqs_act_floats(int64_t n, int d, int hidden_layers, int bins, int level);
int mf_flow_rqs_layer_fwd_save(const float* image, int d, int hidden_layers, int bins, const int32_t* order,
                               const float* x, int64_t n, float* y, const float* logp_in, float* logp_out, int init_logp,
                               float* act, int64_t act_floats, int level, void* stream);
int mf_flow_rqs_layer_bwd_saved(const float* image, int d, int hidden_layers, int bins, const int32_t* order,
                                const float* x, int64_t n, const float* gy, const float* glogp, float* gx, float* gslab,
                                int slab_rows, int accumulate, const float* act, int64_t act_floats, int level, void* stream);

/* Sum of the slab rows, all layers in one launch: gslab[layers][rows][image_floats] ->
 * gflat[j] = sum_{r < rows} gslab[t][r][pos] with grad_index[j] = t * image_floats + pos (-1: parameter without an
 * image slot -> 0).  Fixed summation order, fp64 accumulator: replaces the autograd accumulation of
 * d(mask * W)/dW of zuko's MaskedLinear (reached from mentflow/generate/flows/zuko.py:24-26).                       */
int mf_flow_grad_reduce(const float* gslab, int layers, int rows, int64_t image_floats, const int32_t* grad_index,
                        float* gflat, int64_t numel, void* stream);

/* Inverse of one layer, x = T^-1(y): the d autoregressive passes of zuko AutoregressiveTransform._inverse
 * (mentflow/generate/flows/zuko.py:21-22,31-32 -> log_prob / inverse of an arbitrary point).  `order` is required. */
int mf_flow_rqs_layer_inv(const float* image, int d, int hidden_layers, int bins, const int32_t* order,
                          const float* y, int64_t n, float* x, void* stream);

/* Affine (MAF) variant: zuko MonotonicAffineTransform, y = x*exp(s~)+t, s~ = s/(1+|s/log(1e-3)|), ladj = s~
 * (mentflow/generate/build.py:28 "maf"; BASELINE config C1).  Same image layout with ONE output block whose slot i of
 * lane half 0 is shift_i and of half 1 is scale_i.                                                             */
int64_t mf_flow_affine_image_floats(int d, int hidden_layers);
int64_t mf_flow_affine_bwd_scratch_floats(int64_t n, int hidden_layers);
int mf_flow_affine_layer_fwd(const float* image, int d, int hidden_layers, const int32_t* order, const float* x,
                             int64_t n, float* y, const float* logp_in, float* logp_out, int init_logp, void* stream);
int mf_flow_affine_bwd_slab_rows(int64_t n);
int mf_flow_affine_layer_bwd(const float* image, int d, int hidden_layers, const int32_t* order, const float* x,
                             int64_t n, const float* gy, const float* glogp, float* gx, float* gslab, int slab_rows,
                             int accumulate, float* scratch, int64_t scratch_floats, void* stream);
int mf_flow_affine_layer_inv(const float* image, int d, int hidden_layers, const int32_t* order, const float* y,
                             int64_t n, float* x, void* stream);

/* Wide conditioners (ABI 5): the same layers for hidden widths up to 128 units and / or up to 16 features — shapes whose weights
 * do not fit the 160 KiB of LDS the 64-wide entry points above keep them in (mentflow/generate/build.py:36-38 takes hidden_units
 * and hidden_layers from the config; zuko accepts any).  One family for both transforms: bins = 0 selects the affine (MAF)
 * transform, 2 <= bins <= 21 the rational-quadratic spline.  Differences to the entry points above:
 *   - `image` (mf_flow_wide_image_floats(hidden_layers, nblk) floats, nblk = d for the spline, 1 for affine) holds every weight
 *     matrix twice, as forward and as transposed 32 x 32 MFMA FRAGMENT blocks, and stays in global memory (L2-resident); its layout
 *     is documented in mentflow_amd/csrc/flow_wide.hip and produced by mentflow_amd/generate/packing.py (wide_image_index);
 *   - gslab rows have mf_flow_wide_grad_floats(hidden_layers, nblk) floats in NATURAL order (padded physical rows / columns);
 *     pass that number as `image_floats` to mf_flow_grad_reduce;
 *   - `hidden` = hidden units (1 .. 128; all hidden layers share it), hidden_layers 1 .. 4, d 1 .. 16 (mf_flow_wide_limits);
 *   - the backward is always the two-kernel form: `scratch` needs mf_flow_wide_bwd_scratch_floats floats.                        */
int mf_flow_wide_limits(int* max_features, int* max_hidden, int* max_hidden_layers);
int64_t mf_flow_wide_image_floats(int hidden_layers, int nblk);
int64_t mf_flow_wide_grad_floats(int hidden_layers, int nblk);
int mf_flow_wide_layer_fwd(const float* image, int d, int hidden, int hidden_layers, int bins, const int32_t* order,
                           const float* x, int64_t n, float* y, const float* logp_in, float* logp_out, int init_logp,
                           void* stream);
int64_t mf_flow_wide_bwd_scratch_floats(int64_t n, int d, int hidden_layers, int bins);
int mf_flow_wide_bwd_slab_rows(int64_t n);
int mf_flow_wide_layer_bwd(const float* image, int d, int hidden, int hidden_layers, int bins, const int32_t* order,
                           const float* x, int64_t n, const float* gy, const float* glogp, float* gx, float* gslab,
                           int slab_rows, int accumulate, float* scratch, int64_t scratch_floats, void* stream);
int mf_flow_wide_layer_inv(const float* image, int d, int hidden, int hidden_layers, int bins, const int32_t* order,
                           const float* y, int64_t n, float* x, void* stream);
/* Activation hand-off of the wide family (the counterpart of mf_flow_rqs_layer_fwd_save / _bwd_saved above): a training forward
 * stores every hidden level (in the layout of the backward's scratch tiles, so that the parameter-gradient contraction reads them in
 * place) and every output block's conditioner outputs into `act` (mf_flow_wide_act_floats(n, d, hidden_layers, bins) floats per layer
 * and batch: 3 KB per particle at 128 units, d = 6, three hidden layers); mf_flow_wide_layer_bwd_saved then neither recomputes the
 * conditioner nor re-writes its activations (half of the backward's MFMAs and a third of its scratch traffic).  The whole batch in one
 * call: `x`, `act` and the scratch must cover the same n particles.  Same results as mf_flow_wide_layer_fwd / _bwd.                 */
int64_t mf_flow_wide_act_floats(int64_t n, int d, int hidden_layers, int bins);
int mf_flow_wide_layer_fwd_save(const float* image, int d, int hidden, int hidden_layers, int bins, const int32_t* order,
                                const float* x, int64_t n, float* y, const float* logp_in, float* logp_out, int init_logp,
                                float* act, int64_t act_floats, void* stream);
int mf_flow_wide_layer_bwd_saved(const float* image, int d, int hidden, int hidden_layers, int bins, const int32_t* order,
                                 const float* x, int64_t n, const float* gy, const float* glogp, float* gx, float* gslab,
                                 int slab_rows, int accumulate, float* scratch, int64_t scratch_floats, const float* act,
                                 int64_t act_floats, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fused linear projection + 1-D Gaussian-KDE histogram over P projections.
 * Replaces, for all P transforms at once: `x.clone() @ M.T` (mentflow/simulate/transform.py:67-68, only the
 * consumed output row V_p of each matrix), Histogram1D.project (mentflow/diagnostics/diagnostics.py:116-122) and the
 * residuals/exp/mean of marginal_pdf (mentflow/diagnostics/histogram.py:37-39).
 *   S[p,k] = sum_n exp(-1/2 ((x_n . V_p - coords[k]) / sigma)^2)        (raw sums: the 1/N and the
 *   normalisation of histogram.py:39-43 happen in mf_hist_norm_discrepancy_fwd, after any cross-GPU sum)
 * Only the 2*radius+1 bins around each projected particle are visited (dropped kernel values are below
 * exp(-(radius+1/2)^2 delta^2 / (2 sigma^2)), 3e-18 for the reference's sigma = delta/2 and radius 4); pass
 * radius >= B for the dense sum.  radius and sigma are independent arguments: every pair is evaluated correctly.
 * (radius = 4 with delta / sigma in [2, 2.6] — the reference's bandwidths 0.39 .. 0.5 bins — takes a specialised window
 * with factorised tail weights and, in 2-D, without the 12 corner cells whose weight is below the 2^-50 quantum for
 * every position of the particle; the kernels test the ratio themselves and run the plain loop otherwise.)       */
/* ws: mf_proj_kde_ws_bytes(P, bins) bytes of scratch: one 64-bit INTEGER accumulator per bin.
 * Weights are summed as fixed-point integers at every level (2^-50 units with 64-bit LDS atomics inside a workgroup,
 * one 64-bit integer global atomic per bin and workgroup in 2^(s-50) units, s = max(0, ceil(log2 n) - 13): exact up to
 * 8192 particles per call): order independent, bitwise reproducible.                                            */
int64_t mf_proj_kde_ws_bytes(int P, int bins);
int mf_proj_kde1d_fwd(const float* x, int64_t n, int d, const float* V, int P, const float* coords, int B,
                      float sigma, int radius, float* S, void* ws, void* stream);
/* gx[n,d] (+)= sum_p V_p * sum_k gS[p,k] * K_npk * (-(u_np - c_k)/sigma^2)             */
int mf_proj_kde1d_bwd(const float* x, int64_t n, int d, const float* V, int P, const float* coords, int B,
                      float sigma, int radius, const float* gS, float* gx, int accumulate, void* stream);

/* 2-D variant: two projection vectors per transform (rows `axis[0]`, `axis[1]` of the matrix); replaces
 * Histogram2D.project + marginal_pdf x2 + joint_pdf's Kx^T Ky (histogram.py:47-74,89-101).
 *   S[p,a,b] = sum_n Kx_na Ky_nb   (no 1/N, as the reference)                                                */
int mf_proj_kde2d_fwd(const float* x, int64_t n, int d, const float* V0, const float* V1, int P,
                      const float* coords_x, int Bx, float sigma_x, int radius_x, const float* coords_y, int By,
                      float sigma_y, int radius_y, float* S, void* ws, void* stream);
int mf_proj_kde2d_bwd(const float* x, int64_t n, int d, const float* V0, const float* V1, int P,
                      const float* coords_x, int Bx, float sigma_x, int radius_x, const float* coords_y, int By,
                      float sigma_y, int radius_y, const float* gS, float* gx, int accumulate, void* stream);

/* The launch shape one of the four entry points above takes for a call of these sizes in THIS process (the MENTFLOW_KDE*
 * tuning variables, read once, included): `kernel` 0 = mf_proj_kde1d_fwd, 1 = mf_proj_kde1d_bwd, 2 = mf_proj_kde2d_fwd,
 * 3 = mf_proj_kde2d_bwd; 1-D: Bx = bins, radius_x = radius, By and radius_y are ignored.  Fills out[MF_KDE_PLAN_FIELDS]
 * (a HOST array).  Returns 1, with the reason in mf_last_error(), where the entry point would refuse the sizes or a tuning
 * variable.  Pure host arithmetic: no HIP call, nothing enqueued.  Tests pin the launch path of each case with it and
 * tools/kde_sweep.py records the shape it timed.  A purely additive entry point: MF_ABI_VERSION stays 5.                */
#define MF_KDE_PLAN_WINDOW 0    /* kernel instance: 4 = factorised radius-4 window, 0 = run-time radius                  */
#define MF_KDE_PLAN_BLOCK 1     /* threads per workgroup: 256, 512 or 1024                                               */
#define MF_KDE_PLAN_PG 2        /* projections whose images one workgroup holds in LDS                                   */
#define MF_KDE_PLAN_GROUPS 3    /* ceil(P / PG): grid.y of a forward, passes of a backward                               */
#define MF_KDE_PLAN_PER_WG 4    /* particles per workgroup                                                               */
#define MF_KDE_PLAN_SPLIT 5     /* 1-D backward: lanes per particle (CH); 2-D backward: particles per thread (NPT); else 0 */
#define MF_KDE_PLAN_GRID_X 6    /* workgroups along the particles                                                        */
#define MF_KDE_PLAN_LDS_BYTES 7 /* dynamic LDS of a workgroup                                                            */
#define MF_KDE_PLAN_SHIFT 8     /* forwards: s of the 2^(s-50) accumulator units above; backwards: 0                     */
#define MF_KDE_PLAN_FIELDS 9
int mf_proj_kde_plan(int kernel, int64_t n, int P, int Bx, int By, int radius_x, int radius_y, int64_t* out);

/* Thin multipole kick ahead of a linear map (the non-linear transport of experiments/rec_2d/nonlinear:
 * mentflow/simulate/transform.py:78-146, orders 3..5, k = strength / (order-1)!): u = kick(x), and its adjoint.   */
int mf_multipole_kick_fwd(const float* x, int64_t n, int d, int order, float k, int skew, float* u, void* stream);
int mf_multipole_kick_bwd(const float* x, int64_t n, int d, int order, float k, int skew, const float* gu, float* gx,
                          void* stream);

/* Hard-binned projection histograms (measurement generation / eval): counts[p,k] of u = x.V_p in uniform bins
 * [lo, lo + B*delta], out-of-range ignored, last bin right-inclusive: torch.histogram semantics
 * (mentflow/diagnostics/diagnostics.py:128-131); density/renormalisation is done by the caller.                */
int mf_proj_hist1d_counts(const float* x, int64_t n, int d, const float* V, int P, const float* edges, int B,
                          int32_t* counts, void* stream);
int mf_proj_hist2d_counts(const float* x, int64_t n, int d, const float* V0, const float* V1, int P,
                          const float* edges_x, int Bx, const float* edges_y, int By, int32_t* counts,
                          void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Weighted projection histograms (mentflow_amd/csrc/wproj.hip): the entry points above for particles with a weight each.
 *   w[n]:    one fp32 weight per row.  A weight that is not finite and positive (0, negative, NaN, +-inf) contributes
 *            nothing to S or sums and gets gx = 0.
 *   wmax[1]: DEVICE scalar, the largest valid weight (0 if there is none: S is then all zero).  The forwards accumulate
 *            (w_n / wmax) K in the 2^-50 fixed point of the unweighted kernels and multiply wmax back in at the end, so a
 *            contribution below 2^-50 * wmax rounds to zero.  Sums stay exact integers: order independent, bitwise
 *            reproducible; all weights 1 give the unweighted result bit for bit.
 *   S[p,k]   = sum_n w_n K_npk                    ws: mf_proj_kde_ws_bytes(P, bins) bytes, as above
 *   gx[n,d] (+)= w_n * (gx of the unweighted backward);   gw[n] (+)= sum_p sum_k gS[p,k] K_npk for a weight that is valid
 *            or zero, 0 for a negative, NaN or infinite one.  Either of gx, gw may be NULL (not wanted), not both.
 *   sums[p,k] = sum of w_n over the rows whose projection lies in bin k: torch.histogram(weight=...) semantics, bins as
 *            mf_proj_hist{1,2}d_counts (out of range ignored, last bin right-inclusive); fp32, ws as for the KDE forwards.
 * Launch shapes are those of the unweighted entry point of the same sizes (mf_proj_kde_plan).  Every entry point refuses
 * null pointers, d outside 1..8, fewer than 2 bins, P < 1, P * bins >= 2^31, a sigma that is not finite and positive and
 * a 2-D radius outside 0..5, with the reason in mf_last_error().  Purely additive: MF_ABI_VERSION stays 5.            */
int mf_proj_wkde1d_fwd(const float* x, const float* w, const float* wmax, int64_t n, int d, const float* V, int P,
                       const float* coords, int B, float sigma, int radius, float* S, void* ws, void* stream);
int mf_proj_wkde1d_bwd(const float* x, const float* w, int64_t n, int d, const float* V, int P, const float* coords, int B,
                       float sigma, int radius, const float* gS, float* gx, float* gw, int accumulate, void* stream);
int mf_proj_wkde2d_fwd(const float* x, const float* w, const float* wmax, int64_t n, int d, const float* V0,
                       const float* V1, int P, const float* coords_x, int Bx, float sigma_x, int radius_x,
                       const float* coords_y, int By, float sigma_y, int radius_y, float* S, void* ws, void* stream);
int mf_proj_wkde2d_bwd(const float* x, const float* w, int64_t n, int d, const float* V0, const float* V1, int P,
                       const float* coords_x, int Bx, float sigma_x, int radius_x, const float* coords_y, int By,
                       float sigma_y, int radius_y, const float* gS, float* gx, float* gw, int accumulate, void* stream);
int mf_proj_whist1d_sums(const float* x, const float* w, const float* wmax, int64_t n, int d, const float* V, int P,
                         const float* edges, int B, float* sums, void* ws, void* stream);
int mf_proj_whist2d_sums(const float* x, const float* w, const float* wmax, int64_t n, int d, const float* V0,
                         const float* V1, int P, const float* edges_x, int Bx, const float* edges_y, int By, float* sums,
                         void* ws, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Histogram normalisation + discrepancy for P projections (tiny: P*bins elements; one workgroup per projection).
 *   normalize != 0:  prob = S * pre_scale   (1-D: pre_scale = 1/N_total, histogram.py:39;  2-D: 1, histogram.py:69)
 *                    ghat = prob / (sum(prob) * cell + eps)                        (histogram.py:40-43,70-73)
 *   normalize == 0:  ghat = S  (S already is a prediction; the standalone discrepancy functions)
 *   meas != NULL:    kind 0 (kld): D_p = sum[xlogy(m,m) - m*log(ghat+pad)] / batch_div     (mentflow/loss.py:15-17;
 *                                  batch_div = pred.shape[0] = B for 1-D, Bx for 2-D predictions)
 *                    kind 1 (mae): D_p = sum|ghat-m| / batch_div  (loss.py:7-8, batch_div = number of bins)
 *                    kind 2 (mse): D_p = sum(ghat-m)^2 / batch_div (loss.py:11-12)
 *   ghat may be NULL (not wanted), meas/D may be NULL (normalisation only).
 * bwd: gS[p,k] = dL/dS from gD[p] = dL/dD_p (may be NULL) and/or gghat[p,k] = dL/dghat (may be NULL);
 *      closed form of SURVEY.md Appendix B.                                                                  */
int mf_hist_norm_discrepancy_fwd(const float* S, int P, int bins, int normalize, float pre_scale, float cell,
                                 float eps, const float* meas, int kind, float pad, float batch_div, float* ghat,
                                 float* D, void* stream);
int mf_hist_norm_discrepancy_bwd(const float* S, int P, int bins, int normalize, float pre_scale, float cell,
                                 float eps, const float* meas, int kind, float pad, float batch_div, const float* gD,
                                 const float* gghat, float* gS, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Monte-Carlo entropy sums  (mentflow/entropy.py:58-62 + mentflow/prior.py:25-26):
 *   out[0] = sum_n logp[n],  out[1] = sum_n |x_n|^2      (means / prior constants applied by the caller after
 *   any cross-GPU sum; scratch2 = MF_ENTROPY_SCRATCH_DOUBLES doubles of device scratch: per-workgroup fp64 partials,
 *   summed in a fixed order — no atomics, bitwise reproducible).
 *   mf_scale_rows: gx[n,:] (+)= coef[0] * cscale * x[n,:]  — the adjoint of the |x|^2 term; coef is a DEVICE
 *   scalar (the upstream gradient) so that no host synchronisation is needed.                                 */
int mf_mc_entropy_sums(const float* x, const float* logp, int64_t n, int d, float* out2, double* scratch2,
                       void* stream);
int mf_scale_rows(const float* x, int64_t n, int d, const float* coef, float cscale, float* gx, int accumulate,
                  void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Classical MENT  (mentflow/ment.py:20-52,225-318; mentflow/sample.py:26-113).  Added at ABI version 5: the entry points
 * below are purely additive (no existing signature or behaviour changed), so MF_ABI_VERSION stays 5.
 *
 * Slots: `nslot` (transform, diagnostic) pairs, each a DEVICE float descriptor of 24 floats
 *   [0:8) row r0, [8:16) row r1 (2-D slots; zero-padded beyond d), [16] c0_x, [17] c_last_x, [18] 1/delta_x,
 *   [19] c0_y, [20] c_last_y, [21] 1/delta_y, [22:24) unused
 * and a DEVICE int32 meta row of 4: [ndim (1|2), Bx, By, offset of the slot's table in `tables`].  Tables are the
 * Lagrange-function values at the bin centres, [Bx] or [Bx, By] row-major, concatenated (fp32).
 *   h_s(x) = linear / bilinear interpolation of the table at u = (r0.x[, r1.x]); 0 outside [c0, c_last] on either axis;
 *            NaN for a NaN coordinate; clamped to [0, 1e10].
 *   prob(x) = prod_s h_s(x) * prior(x);  prior_kind 0: 1, 1: exp(prior_lognorm - |x|^2 / (2 prior_a^2)) (prior.Gaussian),
 *            2: exp(prior_lognorm) on [-prior_a, prior_a]^d, else 0.
 * 1 <= d <= 8, 0 <= nslot <= 512.  Sums are fp64 in a fixed order, no float atomics: outputs are bitwise reproducible.
 *
 * mf_ment_prob:       out[p] = prob(x[p])   (multiply != 0: out[p] *= prob(x[p]), for chains of pre-transforms).
 * mf_ment_prob_grid:  the same on the implicit tensor grid of ncells = prod(shape) < 2^31 cells, cell q (ij order, last
 *                     axis fastest) at (coords_0[i_0], ..., coords_{d-1}[i_{d-1}]) (`coords` concatenated per axis;
 *                     `shape` is a HOST array of d), prob[q] written, and block_sums[b] = fp64 sum of (prob[q] + 1e-15f)
 *                     over the cells of block b (mf_ment_blocks(ncells) blocks of 1024 consecutive cells).
 * mf_ment_block_sums: those block sums for a given buffer prob[ncells].
 * mf_ment_sample:     inverse-CDF draws from the cells of prob[shape] with weights prob + 1e-15 (sample_hist_bins):
 *                     rnd[size, 1 + 2d] uniforms in [0, 1) (column 0 picks the cell, 1..d place the point uniformly in it,
 *                     d+1..2d add 0.5 U(-delta, delta) per axis when noise != 0); `edges` = per-axis edge arrays (shape_j + 1
 *                     each) concatenated; prefix = mf_ment_blocks(ncells) + 1 doubles of scratch; x[size, d] written.
 * mf_ment_integrate:  pred[b] = sum_t prob(Minv u_bt) of one slot's line / plane integral: `coords` = per-axis u
 *                     coordinates concatenated (counts[d] HOST), the nmeas measured axes meas_axes (HOST) index the bins in
 *                     ij order in the order given, the other axes (ascending, ij order) the integration points t; minv is a
 *                     HOST [d, d] array.  partial = mf_ment_integrate_ws_doubles(nbins, npoints) doubles of scratch.      */
int64_t mf_ment_blocks(int64_t ncells);
int64_t mf_ment_integrate_ws_doubles(int64_t nbins, int64_t npoints);
int mf_ment_prob(const float* x, int64_t n, int d, int nslot, const float* desc, const int32_t* meta, const float* tables,
                 int64_t table_floats, int prior_kind, float prior_a, float prior_lognorm, int multiply, float* out,
                 void* stream);
int mf_ment_prob_grid(const float* coords, const int64_t* shape, int d, int nslot, const float* desc, const int32_t* meta,
                      const float* tables, int64_t table_floats, int prior_kind, float prior_a, float prior_lognorm,
                      float* prob, double* block_sums, void* stream);
int mf_ment_block_sums(const float* prob, int64_t ncells, double* block_sums, void* stream);
int mf_ment_sample(const float* prob, const int64_t* shape, int d, const double* block_sums, double* prefix,
                   const float* edges, const float* rnd, int64_t size, int noise, float* x, void* stream);
int mf_ment_integrate(int d, const float* minv, const float* coords, const int64_t* counts, int nmeas,
                      const int32_t* meas_axes, int nslot, const float* desc, const int32_t* meta, const float* tables,
                      int64_t table_floats, int prior_kind, float prior_a, float prior_lognorm, double* partial,
                      float* pred, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Metropolis-Hastings chains on the density of classical MENT (no counterpart in the reference).  A purely additive entry
 * point: MF_ABI_VERSION stays 5.  Slot arguments (nslot .. prior_lognorm) exactly as mf_ment_prob takes them.
 *
 * mf_mcmc_ment_steps: `chains` independent random-walk chains, one GPU lane each, advance `steps` steps from x[chains, d]
 *                     (in / out).  Step t of the call has the global index g = step_offset + t:
 *                       y = fma(scale[a], noise[t][a][c], x[a]) for a < d,  p_new = prob(y) (the bits mf_ment_prob returns),
 *                       u = noise[t][d][c];  accept iff  p_new > 0 ? u * p < p_new : (p_new == 0 && p == 0),
 *                     so a chain never leaves the support once inside, random-walks while outside it, and rejects a NaN
 *                     p_new or u.  p = prob(x) is recomputed at entry.  noise[steps][d + 1][chains] (chain fastest; the caller
 *                     draws normal rows 0..d-1 and a uniform [0, 1) row d), scale[d] on the DEVICE.  If g >= keep_from and
 *                     (g - keep_from) % keep_every == 0 the state after step g is written to
 *                     out[(g - keep_from) / keep_every][c][0..d); out may be NULL (nothing kept).  accepted[c] (int32) is
 *                     incremented by the chain's accepted proposals.  No atomics; chains do not interact; the outputs are
 *                     bitwise reproducible and do not depend on how a run is cut into calls (step_offset advanced).
 *                     keep_every >= 1; steps, step_offset, keep_from, keep_every <= 2^40.                                    */
int mf_mcmc_ment_steps(float* x, int64_t chains, int d, int nslot, const float* desc, const int32_t* meta, const float* tables,
                       int64_t table_floats, int prior_kind, float prior_a, float prior_lognorm, const float* noise,
                       int64_t steps, int64_t step_offset, const float* scale, int64_t keep_from, int64_t keep_every,
                       float* out, int32_t* accepted, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Metropolis-adjusted Langevin chains on the density of classical MENT (no counterpart in the reference).  A purely additive
 * entry point: MF_ABI_VERSION stays 5.  Slot arguments (nslot .. prior_lognorm) exactly as mf_ment_prob takes them; x, noise,
 * steps, step_offset, scale, keep_from, keep_every, out and accepted exactly as mf_mcmc_ment_steps takes them.
 *
 * mf_mala_ment_steps: `chains` independent chains, one GPU lane each, advance `steps` steps from x[chains, d] (in / out).  With
 *                     l = logp(x) and g = d logp / dx as mf_ment_logprob returns them (the same device function: the same
 *                     bits), s = scale[a], z = noise[t][a][c], u = noise[t][d][c], all in fp32:
 *                       drift_a(x) = min(max(0.5 s^2 g_a(x), -drift_clip s), drift_clip s)
 *                       y_a = fma(s, z, x_a + drift_a(x)),   r_a = ((x_a - y_a) - drift_a(y)) / s,
 *                       D = (logp(y) - l) + 0.5 (sum_a z^2 - sum_a r_a^2),
 *                       accept iff  logp(y) > -inf ? (l == -inf || log u < D) : (logp(y) == -inf && l == -inf),
 *                     and never when logp(y), u or a z is NaN.  So a chain never leaves the support once inside; outside it
 *                     (l == -inf, g == 0: no drift) it random-walks and takes the first point inside; a state never turns NaN;
 *                     u == 0 accepts whenever D > -inf.  The test is made on logarithms: it stays the Metropolis rule where
 *                     the fp32 product of mf_ment_prob under- or overflows.  drift_clip >= 0 (0: a driftless walk) bounds the
 *                     drift per axis in proposal standard deviations; the truncated drift is a function of the state alone,
 *                     so the correction is exact.  l and g are recomputed at entry.  logp (may be NULL) [chains] receives
 *                     logp of the final states.  No atomics; chains do not interact; the outputs are bitwise reproducible and
 *                     do not depend on how a run is cut into calls (step_offset advanced).  keep_every >= 1; steps,
 *                     step_offset, keep_from, keep_every <= 2^40.                                                          */
int mf_mala_ment_steps(float* x, int64_t chains, int d, int nslot, const float* desc, const int32_t* meta, const float* tables,
                       int64_t table_floats, int prior_kind, float prior_a, float prior_lognorm, const float* noise,
                       int64_t steps, int64_t step_offset, const float* scale, float drift_clip, int64_t keep_from,
                       int64_t keep_every, float* out, int32_t* accepted, float* logp, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Annealed importance sampling on the density of classical MENT (no counterpart in the reference): log-weights whose mean
 * estimates the normaliser of the density.  A purely additive entry point: MF_ABI_VERSION stays 5.  Slot arguments (nslot ..
 * prior_lognorm) exactly as mf_ment_prob takes them; x, scale, drift_clip, accepted and logp exactly as mf_mala_ment_steps.
 *
 * mf_ais_ment_steps: `chains` independent chains, one GPU lane each, walk the temperatures k = temp_offset + 1 .. temp_offset +
 *                    ntemps of the ladder betas[nbetas] (device, non-decreasing in [0, 1]; temp_offset + ntemps < nbetas) from
 *                    x[chains, d] (in / out).  lp = logp(x) and g its gradient as mf_ment_logprob returns them (the same
 *                    device function: the same bits).  The base q0 = N(base_mean, diag base_scale^2) (HOST arrays [d],
 *                    base_scale > 0) has lq(x) = c0 - 0.5 sum t_j^2, t_j = (x_j - m_j) * (1 / b_j), c0 = -sum log b_j -
 *                    (d / 2) log 2 pi formed in fp64, and gradient gq_j = -(t_j * (1 / b_j)).  The tempered density is
 *                    l_b = b > 0 ? lq + b * (lp - lq) : lq with gradient gb = gq + b * (g - gq) (b == 0: gq; 0 where
 *                    l_b == -inf), all in fp32, one rounding per operation.  Per temperature k:
 *                      logw[c] += betas[k] == betas[k-1] ? 0 : (lp > -inf ? (betas[k] - betas[k-1]) * (lp - lq) : -inf)
 *                    (fp32 increment, fp64 sum: logw double[chains], in / out, may reach -inf, never NaN), then
 *                    steps_per_temp >= 0 transitions of mf_mala_ment_steps with l -> l_b and g -> gb at b = betas[k]: same
 *                    proposal, truncated drift, acceptance rule and NaN conventions.  noise[ntemps * steps_per_temp][d + 1]
 *                    [chains] holds this call's transitions in order.  out (may be NULL) [total transitions][chains][d]
 *                    receives the state after every transition, at row temp_offset * steps_per_temp + its index in this
 *                    call.  logp (may be NULL) [chains] receives logp of the final states.  lp, g and lq are recomputed at
 *                    entry: nothing but x and logw crosses a call, and a ladder cut into several calls (temp_offset advanced)
 *                    gives the bits of one call.  No atomics; chains do not interact; outputs are bitwise reproducible.
 *                    chains == 0 and ntemps == 0 do nothing.  ntemps, temp_offset, steps_per_temp <= 2^20.                 */
int mf_ais_ment_steps(float* x, int64_t chains, int d, int nslot, const float* desc, const int32_t* meta, const float* tables,
                      int64_t table_floats, int prior_kind, float prior_a, float prior_lognorm, const float* noise,
                      const float* betas, int64_t nbetas, int64_t ntemps, int64_t temp_offset, int64_t steps_per_temp,
                      const float* scale, float drift_clip, const float* base_mean, const float* base_scale, double* logw,
                      float* out, int32_t* accepted, float* logp, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The resampling stage of a sequential Monte Carlo sampler on the density of classical MENT (no counterpart in the reference):
 * between two calls of mf_ais_ment_steps, which moves the chains and carries their log-weights.  A purely additive entry
 * point: MF_ABI_VERSION stays 5.
 *
 * mf_smc_resample: systematic resampling of the `chains` weighted states x[chains, d] (1 <= d <= 8), split into `groups`
 *                  islands of S = chains / groups consecutive chains (chains % groups == 0); every island is independent of
 *                  every other.  Per island g, with m = max logw over it and w_i = exp(logw_i - m) in fp64 (a logw that is
 *                  NaN or infinite counts as weight 0): S1 = sum w, S2 = sum w^2, ess = S1^2 / S2 (0 if S1 == 0), log mean
 *                  weight = m + log(S1 / S) (-inf if S1 == 0); stats double[groups][4] receives log mean weight, ess,
 *                  resampled (0 or 1) and m.  The island resamples iff S1 > 0 and ess < (double)ess_threshold * S (never
 *                  with a NaN threshold).  If not: its rows of x_out are copies of x, its ancestors are the identity and
 *                  its logw is untouched, bit for bit.  If so: with the inclusive prefix sums P_i of w (scratch double[chains]),
 *                  c = S1 / S and u[g] (device, double; clamped into [0, 1 - 2^-53], NaN -> 0), the parent of row j = 0 ..
 *                  S - 1 is the first i with fma(-j, c, P_i) > u[g] c, that is P_i > (u[g] + j) c, searchsorted from the
 *                  right, without the rounding of u + j (equal weights give the identity for every u); where rounding
 *                  leaves none it is the first i with P_i == S1, the last state whose weight moved the prefix.  A state of
 *                  weight 0 is never a parent; parents do not decrease within an island.  x_out[j] = x[parent] bitwise,
 *                  ancestors int32[chains] holds the global index of each row's parent, and every logw of the island
 *                  becomes its log mean weight, so logsumexp(logw) - log S is kept.  Every sum is taken in a fixed order
 *                  (thread segments, then the segment totals in order); no atomics; outputs are bitwise reproducible and
 *                  island g's depend on nothing but its own rows and u[g].  x_out must not be x.  chains == 0 does nothing. */
int mf_smc_resample(const float* x, float* x_out, int64_t chains, int d, int64_t groups, double* logw, const double* u,
                    float ess_threshold, int32_t* ancestors, double* stats, double* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Differentiable log-density of classical MENT (no counterpart in the reference, whose interpolators are scipy on the host).
 * A purely additive entry point: MF_ABI_VERSION stays 5.  Slot arguments (nslot .. prior_lognorm) and limits exactly as
 * mf_ment_prob takes them; n = 0 and nslot = 0 are valid.
 *
 * mf_ment_logprob: logp[i] = sum_s log clamp(h_s(x_i), 0, 1e10) + log prior(x_i)  (prior_kind 0: + 0; 1: + prior_lognorm -
 *                  |x|^2 / (2 prior_a^2); 2: + prior_lognorm inside [-prior_a, prior_a]^d, -inf outside).  Projections and
 *                  cells are those of mf_ment_prob bit for bit, slot order and early exit included: logp = -inf exactly where
 *                  that product meets a zero factor first, NaN where it meets a NaN factor first; where the fp32 product would
 *                  merely underflow or overflow, logp stays finite and accurate (the factors' exponents are summed apart).
 *                  grad (may be NULL) [n, d] = d logp / dx = sum_s (h_s' / h_s) rows_s + d log prior / dx, with the derivative
 *                  of the cell that holds the point (the right derivative at an interior bin centre, the left one at the last
 *                  centre); a slot with h_s >= 1e10 (on the clamp) contributes nothing; a row with logp = -inf gets 0, a row
 *                  with logp = NaN gets NaN.  Tables are constants.  No atomics; rows are independent; bitwise reproducible. */
int mf_ment_logprob(const float* x, int64_t n, int d, int nslot, const float* desc, const int32_t* meta, const float* tables,
                    int64_t table_floats, int prior_kind, float prior_a, float prior_lognorm, float* logp, float* grad,
                    void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Gradient of the log-density of classical MENT with respect to its Lagrange tables: the adjoint of mf_ment_logprob in
 * `tables` (no counterpart in the reference).  A purely additive entry point: MF_ABI_VERSION stays 5.  x, n, d and the slot
 * arguments (nslot .. table_floats) and their limits exactly as mf_ment_logprob takes them (the prior does not depend on the
 * tables and is not passed); n = 0 zeroes the outputs and returns 0.
 *
 * mf_ment_logprob_tables_bwd:  grad_log[e] = sum_i weight[i] rho_e(x_i) = dL / d log tables[e] for L = sum_i weight[i] logp[i],
 *                  grad_tab[e] (may be NULL) = grad_log[e] / tables[e] = dL / d tables[e] where tables[e] > 0, else 0: a zero
 *                  entry is outside MENT's support and stays there, as under the multiplicative update (the one-sided
 *                  derivative there is not returned).  logp[n] is what mf_ment_logprob returned for the same arguments, weight[n]
 *                  the upstream dL / dlogp.  A row takes part iff logp[i] is finite and weight[i] != 0; a row with logp = -inf
 *                  contributes nothing whatever its weight (NaN included).  Projections and cells (i, w) are those of
 *                  mf_ment_logprob bit for bit.  Per slot and node e of the cell, rho_e = node weight * tables[e] / h clamped to
 *                  [0, 1]: for a 1-D slot with h = a (1 - w) + b w the pair a (1 - w) / h, b w / h, for a 2-D slot the four
 *                  bilinear terms; the clamp is a no-op up to rounding for non-negative tables, and for tables with negative
 *                  entries the result is only promised finite.  A slot with h >= 1e10 (on the upper clamp: a constant)
 *                  contributes nothing, nor does a slot with h <= 0 or NaN on a row the caller declared live.
 *                  Fixed point: wmax is a DEVICE scalar >= 0, the maximum of |weight| over the rows with finite logp;
 *                  P = 2^ceil(log2 wmax), F = min(50, 62 - ceil(log2 max(n, 2))); each contribution is
 *                  round((weight / P) rho 2^F) (|weight| / P is clamped to 1 should wmax be too small), added as a signed
 *                  64-bit integer in two's complement, which cannot overflow; acc[table_floats] is workspace the call zeroes
 *                  first; a finishing pass writes acc * P * 2^-F, formed in fp64 and rounded once.  wmax == 0 gives all zeros.
 *                  Integer atomics only (64-bit, in LDS while descriptors + tables fit the budget of mf_ment_logprob's
 *                  tables-in-LDS instance, else straight into acc): bitwise reproducible, independent of the order of the rows.
 *                  Poison: status[0] (DEVICE, int32) is set to 0 and then to non-zero if wmax is NaN or inf, if a row has NaN
 *                  logp and weight != 0 (NaN counts), or if a row has finite logp and a non-finite weight; such rows add
 *                  nothing, the outputs stay finite, and the caller decides (ops.ment_logprob_table_grad returns NaN). */
int mf_ment_logprob_tables_bwd(const float* x, int64_t n, int d, int nslot, const float* desc, const int32_t* meta,
                               const float* tables, int64_t table_floats, const float* logp, const float* weight,
                               const float* wmax, unsigned long long* acc, float* grad_log, float* grad_tab, int32_t* status,
                               void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Sliced Wasserstein distance  (mentflow/loss.py:20-42, where the 1-D transport cost is POT's ot.lp.wasserstein_1d on the
 * host).  Purely additive entry points: MF_ABI_VERSION stays 5.  No float atomics, fp64 sums in a fixed order: every output
 * is bitwise reproducible.  All sizes obey P * n < 2^31.
 *
 * mf_swd_project:        u[p, i] = sum_k x[i, k] * dir[k, p] for x[n, d] (1 <= d <= 8) and dir[d, P]; u is projection-major
 *                        [P, n] so that each projection is one contiguous segment.
 * mf_segsort_f32:        out[s, :] = keys[s, :] in ascending order for each of the P segments of n fp32 keys (keys only, no
 *                        payload).  Order of torch.sort: NaN last (written back as a quiet NaN), -0.0 and +0.0 compare equal.
 *                        Tiles of 2^tile_log2 keys are sorted in LDS, then merged pairwise in ceil(log2(tiles)) passes between
 *                        `out` and the workspace; tile_log2 = 0 selects the built-in tile (2^12), 4..12 are accepted.
 *                        `ws` = mf_segsort_workspace_bytes(P, n, tile_log2) bytes of device scratch (0: none needed, ws may be
 *                        NULL; -1: bad arguments).  `out` may be `keys`.
 * mf_swd_quantile_cost:  u[P, n1], v[P, n2] sorted per row ->
 *                          wpp[s] = int_0^1 |F_u^-1(q) - F_v^-1(q)|^p dq   (fp64)
 *                        for the uniform-weight empirical measures of row s: mean_i |u_i - v_i|^p for n1 == n2, else the sum
 *                        over the merged quantile breakpoints with weights formed exactly in int64 (n1 * n2 < 2^63), and
 *                          dist[0] = (sum_s wpp[s] / P)^(1/p)   (fp32).
 *                        p >= 1 real (fast paths for 1 and 2).  A NaN anywhere in a row makes that wpp and dist NaN.
 *                        partial = mf_swd_cost_ws_doubles(P, n1, n2) doubles of scratch.
 *
 * The adjoint (gradient of dist with respect to either point cloud; the directions are constants):
 *
 * mf_segsort_pairs_f32:  the same sort carrying each key's position: out[s, r] is bitwise what mf_segsort_f32 writes and
 *                        perm[s, r] in [0, n) is the position in segment s of the key that ended up at rank r; perm[s, :] is
 *                        always a permutation of 0..n-1 (also for rows of NaN, +-inf, +-0).  Order: ascending in the mapped
 *                        key (-0.0 in front of +0.0, every NaN last), equal mapped keys by ascending position, i.e.
 *                        torch.sort(stable=True) except that torch leaves mixed signed zeros in input order.  The unique
 *                        64-bit composites (mapped key << 32 | position) are sorted, so the result does not depend on the
 *                        network or merge order.  tile_log2 as above (0: the built-in pair tile, 2^12).
 *                        `ws` = mf_segsort_pairs_workspace_bytes(P, n, tile_log2) bytes (0: none, -1: bad arguments), 8-byte
 *                        aligned.  `out` may be `keys`.
 * mf_swd_quantile_cost_bwd:  u[P, n1], v[P, n2] sorted per row and wpp[P] as mf_swd_quantile_cost left them, gdist[1] the
 *                        gradient arriving at dist (device scalar; no device-to-host copy, no host synchronisation) ->
 *                        gu[P, n1], gv[P, n2] = gdist * d dist / d u, d v.  With M = sum_s wpp[s] / P (the forward's order),
 *                          coef = gdist (1/p) M^(1/p - 1) / P   (p = 1: gdist / P;  M == 0: coef = 0;  M NaN: all NaN),
 *                        t = a - b one fp32 subtraction, then fp64: phi'(t) = sign(t) (p = 1), 2 t (p = 2), else
 *                        p |t|^(p-1) sign(t); sign(0) = 0.  Equal sizes: g[r] = coef phi'(u_r - v_r) / n for u, the negative
 *                        for v.  Unequal sizes: the sum over the quantile pieces an element takes part in, with the forward's
 *                        int64 weights, divided by n1 n2 in fp64 and rounded once to fp32 (an element of the smaller set
 *                        meets a contiguous range of the larger one, summed by a lane group in a fixed-shape fp64 tree: no
 *                        atomics).  M == 0 (identical clouds) gives zero gradients by definition, where differentiating
 *                        the composed formula gives 0 * inf = NaN for p > 1.  gu or gv may be NULL: that side is skipped.
 *                        perm_u / perm_v (from mf_segsort_pairs_f32) != NULL: the value of rank r is stored at position
 *                        perm[s, r] (the un-sort fused into the store); NULL: at r.
 * mf_swd_project_bwd:    gx[i, k] (+)= sum_p dir[k, p] * g[p, i] for g[P, n], gx[n, d]: an fmaf chain over ascending p per
 *                        output, no atomics; accumulate != 0 adds onto gx.  Limits of mf_swd_project.                        */
int mf_swd_project(const float* x, int64_t n, int d, const float* dir, int P, float* u, void* stream);
int64_t mf_segsort_workspace_bytes(int P, int64_t n, int tile_log2);
int mf_segsort_f32(const float* keys, int P, int64_t n, int tile_log2, float* out, void* ws, void* stream);
int64_t mf_swd_cost_ws_doubles(int P, int64_t n1, int64_t n2);
int mf_swd_quantile_cost(const float* u, int64_t n1, const float* v, int64_t n2, int P, float p, double* partial, double* wpp,
                         float* dist, void* stream);
int64_t mf_segsort_pairs_workspace_bytes(int P, int64_t n, int tile_log2);
int mf_segsort_pairs_f32(const float* keys, int P, int64_t n, int tile_log2, float* out, int32_t* perm, void* ws, void* stream);
int mf_swd_quantile_cost_bwd(const float* u, int64_t n1, const int32_t* perm_u, const float* v, int64_t n2,
                             const int32_t* perm_v, int P, float p, const double* wpp, const float* gdist, float* gu, float* gv,
                             void* stream);
int mf_swd_project_bwd(const float* g, int64_t n, int d, const float* dir, int P, float* gx, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Sample-based entropy estimators  (mentflow/entropy.py:27-50).  Purely additive entry points: MF_ABI_VERSION stays 5.  Both
 * return the NEGATIVE entropy H as one fp32 device scalar; no float atomics, fp64 sums in a fixed order: every output is
 * bitwise reproducible.  x[n, d] fp32, 1 <= d <= 16.
 *
 * mf_knn_entropy_fwd:  Kozachenko-Leonenko estimate with the k-th nearest other point, 1 <= k <= 16, n > k:
 *                        H = -[psi(n) - psi(k) + ln c_d + (d / n) sum_i ln rho_k(i)],   c_d = pi^(d/2) / Gamma(d/2 + 1).
 *                      rho^2 from direct fp32 differences; neighbours ordered by (rho^2, index); ln rho = 0.5 ln max(rho^2,
 *                      FLT_MIN).  Outputs: H[1], sum_ln_rho[1] (fp64), idx[n] (the k-th neighbour j(i), always in [0, n)) and
 *                      rho2[n].  A point with fewer than k candidates at finite distance (NaN / inf coordinates) gets
 *                      rho2 = +inf and idx = i, which makes H non-finite.  `chunks` cuts the candidate range over the grid
 *                      (0: built-in choice, else 1..65535); idx and rho2 do not depend on it.
 *                      ws = mf_knn_entropy_ws_bytes(n, d, k, chunks) bytes of device scratch (-1: bad arguments).
 * mf_knn_entropy_bwd:  gx[i] = coef[0] * cscale * d(sum ln rho)/dx_i
 *                            = coef[0] * cscale * [ w_i (x_i - x_j(i)) + sum_{i': j(i') = i} w_i' (x_i - x_i') ],
 *                      w = 1 / rho2 where FLT_MIN < rho2 < inf, else 0; the reverse-neighbour sum runs in ascending i'.  coef is
 *                      a DEVICE scalar (the upstream gradient); the caller passes cscale = -d / n.
 * mf_cov_entropy_fwd:  eps = sqrt(det(cov(x))) (divisor n - 1), H = -3 ln(2 pi e) - ln(eps + pad): the reference's formula as it
 *                      stands (its constant is the 6-D one whatever d).  aux[d + d * d] (fp64) receives the mean and the matrix
 *                      A = -eps / (eps + pad) / (n - 1) * cov^-1 of the adjoint (zero where det is not positive and finite).
 *                      ws = mf_cov_entropy_ws_doubles(n, d) doubles of device scratch (-1: bad arguments).
 * mf_cov_entropy_bwd:  gx[i] = coef[0] * A (x_i - mean), evaluated in fp64 and rounded once.                              */
int64_t mf_knn_entropy_ws_bytes(int64_t n, int d, int k, int chunks);
int mf_knn_entropy_fwd(const float* x, int64_t n, int d, int k, int chunks, float* H, double* sum_ln_rho, int32_t* idx,
                       float* rho2, void* ws, void* stream);
int mf_knn_entropy_bwd(const float* x, int64_t n, int d, const int32_t* idx, const float* rho2, const float* coef,
                       float cscale, float* gx, void* stream);
int64_t mf_cov_entropy_ws_doubles(int64_t n, int d);
int mf_cov_entropy_fwd(const float* x, int64_t n, int d, double pad, float* H, double* aux, double* ws, void* stream);
int mf_cov_entropy_bwd(const float* x, int64_t n, int d, const double* aux, const float* coef, float* gx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MENTFLOW_HIP_H */
