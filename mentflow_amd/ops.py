"""torch.autograd wrappers over the C ABI of libmentflow_hip.so (include/mentflow_hip.h).

Each Function's forward AND backward is a hand-written gfx950 kernel; torch supplies device memory, the current
stream and the autograd graph between ops, nothing else.  All tensors must live on the GPU (mentflow_amd._lib.ptr
raises otherwise): there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import List, Optional, Tuple

import torch

from . import _lib
from ._lib import call, ptr, stream_ptr

_F32 = torch.float32
_ENV_ACT_LEVEL = int(os.environ["MENTFLOW_ACT_LEVEL"]) if os.environ.get("MENTFLOW_ACT_LEVEL", "") != "" else None


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != _F32:
        raise RuntimeError(f"mentflow_amd kernels compute in float32 (got {t.dtype})")
    return t.contiguous()


def kde_radius(bandwidth_in_bins: float) -> int:
    """Truncation radius (bins) of the Gaussian KDE: weights beyond (R + 1/2) bins are < exp(-40.5) = 2.6e-18."""
    return max(1, int(math.ceil(9.0 * float(bandwidth_in_bins) - 0.5)))


# ------------------------------------------------------------------------------------------------ flow
# One class per kernel family (include/mentflow_hip.h): its entry points and size queries.  FlowSpec picks the family once;
# the layer loops below call through it.  `shape` = the arguments between `image` and `order`; fwd / bwd return the entry point
# of a hand-off level and the arguments that follow `init_logp` / `accumulate`.
class _NarrowRqs:
    """mf_flow_rqs_*: the 64-wide spline kernels (weights in LDS).  Fused backward where the layer's mask structure and LDS
    budget allow (mf_flow_set_bwd_variant can force the two-kernel path); hand-off levels 1 and 2."""
    inv = "mf_flow_rqs_layer_inv"
    saved_whole = False     # the saved-activation backward is the fused kernel: no scratch, one chunk anyway

    def __init__(self, s: "FlowSpec"):
        self.s, self.shape = s, (s.d, s.L, s.bins)

    def fwd(self, act, level):
        return ("mf_flow_rqs_layer_fwd_save", (ptr(act), act.numel(), level)) if level > 0 else ("mf_flow_rqs_layer_fwd", ())

    def bwd(self, scratch, act, level):
        return (("mf_flow_rqs_layer_bwd_saved", (ptr(act), act.numel(), level)) if level > 0 else
                ("mf_flow_rqs_layer_bwd", (ptr(scratch), scratch.numel())))

    def scratch_floats(self, n):
        return max(_lib.get_lib().mf_flow_bwd_scratch_floats(n, self.s.d, self.s.L, o) for o in self.s.orders)

    def slab_rows(self, n):
        r = {_lib.get_lib().mf_flow_bwd_slab_rows(n, self.s.d, self.s.L, o) for o in self.s.orders}
        if len(r) != 1:
            raise RuntimeError("layers of one flow disagree on the backward variant")
        return r.pop()

    def act_floats(self, n, level):
        return _lib.get_lib().mf_flow_rqs_act_floats(n, self.s.d, self.s.L, self.s.bins, level)

    def top_level(self):    # under the CURRENT backward variant (0 for the two-kernel path)
        return min(_lib.get_lib().mf_flow_rqs_act_level(self.s.d, self.s.L, self.s.bins, o) for o in self.s.orders)


class _NarrowAffine:
    """mf_flow_affine_*: the 64-wide affine kernels (weights in LDS); no activation hand-off."""
    inv = "mf_flow_affine_layer_inv"
    saved_whole = False

    def __init__(self, s: "FlowSpec"):
        self.s, self.shape = s, (s.d, s.L)

    def fwd(self, act, level):
        return "mf_flow_affine_layer_fwd", ()

    def bwd(self, scratch, act, level):
        return "mf_flow_affine_layer_bwd", (ptr(scratch), scratch.numel())

    def scratch_floats(self, n):
        return _lib.get_lib().mf_flow_affine_bwd_scratch_floats(n, self.s.L)

    def slab_rows(self, n):
        return _lib.get_lib().mf_flow_affine_bwd_slab_rows(n)

    def act_floats(self, n, level):
        return 0

    def top_level(self):
        return 0


class _Wide:
    """mf_flow_wide_*: hidden_units 65 .. 128 and / or 8 .. 16 features.  Weights in global memory as MFMA fragments, two-kernel
    backward, gradient slabs in natural order; one hand-off level (hidden tiles + conditioner outputs)."""
    inv = "mf_flow_wide_layer_inv"
    saved_whole = True      # the saved activations cover the batch as one tile sequence: one chunk whatever the scratch costs

    def __init__(self, s: "FlowSpec"):
        self.s, self.bins = s, (s.bins if s.kind == "rqs" else 0)
        self.shape = (s.d, s.hidden, s.L, self.bins)

    def fwd(self, act, level):
        return ("mf_flow_wide_layer_fwd_save", (ptr(act), act.numel())) if level > 0 else ("mf_flow_wide_layer_fwd", ())

    def bwd(self, scratch, act, level):
        tail = (ptr(scratch), scratch.numel())
        return ("mf_flow_wide_layer_bwd_saved", tail + (ptr(act), act.numel())) if level > 0 else ("mf_flow_wide_layer_bwd", tail)

    def scratch_floats(self, n):
        return _lib.get_lib().mf_flow_wide_bwd_scratch_floats(n, self.s.d, self.s.L, self.bins)

    def slab_rows(self, n):
        return _lib.get_lib().mf_flow_wide_bwd_slab_rows(n)

    def act_floats(self, n, level):
        return _lib.get_lib().mf_flow_wide_act_floats(n, self.s.d, self.s.L, self.bins)

    def top_level(self):
        return 1


class FlowSpec:
    """Static description of a packed flow (shared by every call): geometry, kernel family + device index maps."""

    def __init__(self, d: int, hidden_layers: int, transforms: int, kind: str, bins: int, image_floats: int,
                 image_index: torch.Tensor, grad_index: torch.Tensor, orders, wide: bool = False, hidden: int = 64,
                 grad_floats: Optional[int] = None):
        self.d, self.L, self.T, self.kind, self.bins, self.hidden = d, hidden_layers, transforms, kind, bins, int(hidden)
        self.grad_floats = int(image_floats if grad_floats is None else grad_floats)
        # per layer: host int32 array of the autoregressive order (lets the kernels skip masked-out MFMA k-steps)
        self.orders = [(C.c_int32 * d)(*[int(v) for v in o]) for o in orders]
        self.family = _Wide(self) if wide else (_NarrowRqs(self) if kind == "rqs" else _NarrowAffine(self))
        self.image_floats = image_floats
        self.image_index = image_index      # int32 [T * image_floats]  -> flat parameter index or -1
        self.grad_index = grad_index        # int32 [numel]             -> position in the image stack or -1
        self.bwd_chunk = 1 << 20            # particles per backward chunk (3 KiB of scratch each at d=6)
        # Activation hand-off from the training forward to the backward through HBM (mf_flow_rqs_layer_fwd_save): None = the
        # highest level (2: hidden tiles + conditioner outputs, 1: hidden tiles, 0: recompute everything) that the family's
        # kernels take for this flow AND whose buffers (T layers x 1 712 / 512 B per particle at d = 6, L = 3, 20 bins) fit
        # `act_budget_bytes`; an int pins the level (tests, A/B runs).  Environment: MENTFLOW_ACT_LEVEL.
        self.act_level: Optional[int] = _ENV_ACT_LEVEL
        self.act_budget_bytes: Optional[int] = None     # None: 60 % of the device's memory (173 GB on an MI355X)

    def resolve_act_level(self, n: int, device: torch.device) -> int:
        """The wanted level (act_level, capped by the family's highest), stepped down while T layers of buffers exceed the
        budget."""
        if n <= 0:
            return 0
        top = self.family.top_level()
        level = top if self.act_level is None else min(int(self.act_level), top)
        if level <= 0:
            return 0
        budget = self.act_budget_bytes
        if budget is None:
            budget = int(0.6 * torch.cuda.get_device_properties(device).total_memory) if device.type == "cuda" else 1 << 62
        while level > 0 and 4 * self.T * self.family.act_floats(n, level) > budget:
            level -= 1
        return level


def _layer_fwd(spec: FlowSpec, t: int, image: torch.Tensor, x: torch.Tensor, y: torch.Tensor,
               logp_in: Optional[torch.Tensor], logp_out: torch.Tensor, init: bool, act: Optional[torch.Tensor] = None,
               act_level: int = 0) -> None:
    name, tail = spec.family.fwd(act, act_level)
    call(name, ptr(image), *spec.family.shape, spec.orders[t], ptr(x), x.shape[0], ptr(y), ptr(logp_in), ptr(logp_out),
         int(init), *tail, stream_ptr(x))


def _layer_bwd(spec: FlowSpec, t: int, image, x, gy, glogp, gx, gslab, accumulate: bool, scratch, act=None,
               act_level: int = 0) -> None:
    name, tail = spec.family.bwd(scratch, act, act_level)
    call(name, ptr(image), *spec.family.shape, spec.orders[t], ptr(x), x.shape[0], ptr(gy), ptr(glogp), ptr(gx), ptr(gslab),
         gslab.shape[0], int(accumulate), *tail, stream_ptr(x))


def _bwd_plan(spec: FlowSpec, n: int, level: int):
    """(chunk, scratch_floats) of a backward pass over n particles: the fused kernels need no scratch and take the whole
    batch in one launch per layer; the two-kernel path is chunked to bound its hand-off scratch.  Every chunk of a pass must
    write the same number of slab rows (each workgroup accumulates into its own row), so a ragged last chunk is only allowed
    when it does."""
    fam = spec.family
    chunk = n if (fam.scratch_floats(n) == 0 or (level > 0 and fam.saved_whole)) else min(n, spec.bwd_chunk)
    return chunk, fam.scratch_floats(chunk)


def pack_images(spec: FlowSpec, flat: torch.Tensor) -> torch.Tensor:
    images = torch.empty(spec.T * spec.image_floats, dtype=_F32, device=flat.device)
    call("mf_gather_f32", ptr(flat), ptr(spec.image_index), ptr(images), images.numel(), 0, stream_ptr(flat))
    return images.view(spec.T, spec.image_floats)


class FlowSampleFn(torch.autograd.Function):
    """(z[N,d], flat parameters) -> (x[N,d], log_prob[N]) through all T autoregressive layers.

    Replaces zuko ``NormalizingFlow.rsample_and_log_prob`` as called by
    mentflow/generate/flows/zuko.py:24-26 (base draw z injected) and its autograd backward.
    Saved for backward: the T layer inputs (N x d each), the packed images and — FlowSpec.act_level — the conditioner's
    hidden tiles / outputs of every layer, written by the forward kernels in the register layout of the fused backward
    (the eager reference keeps every activation for autograd; level 0 recomputes them in the backward instead).

    Two ways to receive the parameter gradient: (a) ``flat`` is an autograd tensor (e.g. ``torch.cat`` of the parameters):
    its gradient is returned to autograd; (b) ``flat`` is a plain buffer, ``trigger`` a leaf that requires grad (so that
    autograd calls this backward) and ``grad_sink(gflat)`` deposits the gradient (AutoregressiveFlow: one flat copy
    into the parameters' .grad views instead of one accumulation kernel per parameter).  In form (b) the parameters are
    NOT part of the autograd graph (see the AutoregressiveFlow docstring for what that implies).  dL/dz is returned when
    ``z`` requires grad (one more layer-0 input gradient + the base-density term -z dL/dlog_prob)."""

    @staticmethod
    def forward(ctx, z: torch.Tensor, flat: torch.Tensor, spec: FlowSpec, grad_reduce=None, trigger=None, grad_sink=None):
        z = _f32c(z)
        flat = _f32c(flat.detach())
        n = z.shape[0]
        images = pack_images(spec, flat)
        logp = torch.empty(n, dtype=_F32, device=z.device)
        level = spec.resolve_act_level(n, z.device)
        act = torch.empty(spec.T, spec.family.act_floats(n, level), dtype=_F32, device=z.device) if level > 0 else None
        xs = [z]
        for t in range(spec.T):
            y = torch.empty_like(z)
            _layer_fwd(spec, t, images[t], xs[-1], y, logp, logp, t == 0, None if act is None else act[t], level)
            xs.append(y)
        ctx.spec = spec
        ctx.grad_reduce = grad_reduce
        ctx.grad_sink = grad_sink
        ctx.act_level = level
        # a SAVED tensor, so that autograd releases it with the graph right after backward (kept as a plain attribute it lived as
        # long as the loss tensor of the step: two 18 GB buffers alive at C4, and no room for the 16 M-particle batch)
        ctx.save_for_backward(images, act if act is not None else images.new_empty(0), *xs[:-1])
        return xs[-1], logp

    @staticmethod
    def backward(ctx, gx: Optional[torch.Tensor], glogp: Optional[torch.Tensor]):
        spec: FlowSpec = ctx.spec
        images, act, *xs = ctx.saved_tensors
        n = xs[0].shape[0]
        dev = images.device
        gx = torch.zeros(n, spec.d, dtype=_F32, device=dev) if gx is None else _f32c(gx)
        glogp = torch.zeros(n, dtype=_F32, device=dev) if glogp is None else _f32c(glogp)
        level = ctx.act_level
        chunk, scratch_floats = _bwd_plan(spec, n, level)
        act = act if level > 0 else None
        if level > 0 and chunk != n:
            raise RuntimeError("the backward variant changed between forward and backward: the saved activations belong to the "
                               "fused kernel (mf_flow_set_bwd_variant)")
        scratch = torch.empty(max(scratch_floats, 1), dtype=_F32, device=dev)
        # chunks grouped by the number of slab rows they write (at most two groups: full chunks and a ragged last one)
        spans = [(a, min(n, a + chunk)) for a in range(0, n, chunk)]
        groups = {}
        for a, b in spans:
            groups.setdefault(spec.family.slab_rows(b - a), []).append((a, b))
        gflat = None
        g = gx
        slabs = {r: torch.empty(spec.T, r, spec.grad_floats, dtype=_F32, device=dev) for r in groups}
        need_gz = ctx.needs_input_grad[0]             # dL/dz: the reference's transform is differentiable in the base draw
        for t in reversed(range(spec.T)):
            gprev = torch.empty_like(g) if (t > 0 or need_gz) else None
            for r, members in groups.items():
                for k, (a, b) in enumerate(members):
                    _layer_bwd(spec, t, images[t], xs[t][a:b], g[a:b], glogp[a:b], None if gprev is None else gprev[a:b],
                               slabs[r][t], k > 0, scratch, None if act is None else act[t], level)
            g = gprev
        for r, slab in slabs.items():
            part = torch.empty(spec.grad_index.numel(), dtype=_F32, device=dev)
            call("mf_flow_grad_reduce", ptr(slab), spec.T, r, spec.grad_floats, ptr(spec.grad_index), ptr(part),
                 part.numel(), stream_ptr(part))
            gflat = part if gflat is None else gflat + part
        # g is now dL/dz through x and the log-det; log_prob also holds the base density logN(z) = -|z|^2/2 - const
        gz = g - xs[0] * glogp[:, None] if need_gz else None
        if ctx.grad_reduce is not None:
            ctx.grad_reduce(gflat)
        if ctx.grad_sink is not None:
            ctx.grad_sink(gflat)
            return gz, None, None, None, None, None
        return gz, gflat, None, None, None, None


def flow_layers_forward(z: torch.Tensor, flat: torch.Tensor, spec: FlowSpec) -> Tuple[List[torch.Tensor], torch.Tensor]:
    """No-grad helper: every intermediate [z, x_1, ..., x_T] and log_prob (forward_steps / sample)."""
    z = _f32c(z)
    images = pack_images(spec, _f32c(flat.detach()))
    logp = torch.empty(z.shape[0], dtype=_F32, device=z.device)
    xs = [z]
    for t in range(spec.T):
        y = torch.empty_like(z)
        _layer_fwd(spec, t, images[t], xs[-1], y, logp, logp, t == 0)
        xs.append(y)
    return xs, logp


def flow_layers_inverse(x: torch.Tensor, flat: torch.Tensor, spec: FlowSpec) -> List[torch.Tensor]:
    """No-grad: [x, T_T^-1(x), ..., z] — the layers in reverse, d autoregressive passes each
    (mentflow/generate/flows/zuko.py:31-32,43-50)."""
    x = _f32c(x)
    images = pack_images(spec, _f32c(flat.detach()))
    zs = [x]
    for t in reversed(range(spec.T)):
        out = torch.empty_like(x)
        call(spec.family.inv, ptr(images[t]), *spec.family.shape, spec.orders[t], ptr(zs[-1]), x.shape[0], ptr(out),
             stream_ptr(x))
        zs.append(out)
    return zs


# ------------------------------------------------------------------------------------------------ projections + KDE
class ProjKde1dFn(torch.autograd.Function):
    """x[N,d], V[P,d] -> S[P,B] = sum_n exp(-((x_n.V_p - c_k)/sigma)^2 / 2)   (raw kernel sums).

    Replaces the Python loop of mentflow/simulate/simulate.py:30-33 over LinearTransform.forward
    (simulate/transform.py:67-68) + Histogram1D.project (diagnostics/diagnostics.py:116-122) + the kernel matrix of
    marginal_pdf (diagnostics/histogram.py:37-39)."""

    @staticmethod
    def forward(ctx, x, V, coords, sigma: float, radius: int):
        x, V, coords = _f32c(x), _f32c(V), _f32c(coords)
        P, B = V.shape[0], coords.numel()
        S = torch.empty(P, B, dtype=_F32, device=x.device)
        ws = torch.empty(_lib.get_lib().mf_proj_kde_ws_bytes(P, B) // 8, dtype=torch.int64, device=x.device)
        call("mf_proj_kde1d_fwd", ptr(x), x.shape[0], x.shape[1], ptr(V), P, ptr(coords), B, float(sigma), int(radius),
             ptr(S), ptr(ws), stream_ptr(x))
        ctx.save_for_backward(x, V, coords)
        ctx.sigma, ctx.radius = float(sigma), int(radius)
        return S

    @staticmethod
    def backward(ctx, gS):
        x, V, coords = ctx.saved_tensors
        gx = torch.empty_like(x)
        call("mf_proj_kde1d_bwd", ptr(x), x.shape[0], x.shape[1], ptr(V), V.shape[0], ptr(coords), coords.numel(),
             ctx.sigma, ctx.radius, ptr(_f32c(gS)), ptr(gx), 0, stream_ptr(x))
        return gx, None, None, None, None


class ProjKde2dFn(torch.autograd.Function):
    """x[N,d], V0[P,d], V1[P,d] -> S[P,Bx,By] = sum_n Kx_na Ky_nb  (histogram.py:89-101 / joint_pdf :69)."""

    @staticmethod
    def forward(ctx, x, V0, V1, coords_x, coords_y, sigma_x: float, sigma_y: float, radius_x: int, radius_y: int):
        x, V0, V1, cx, cy = _f32c(x), _f32c(V0), _f32c(V1), _f32c(coords_x), _f32c(coords_y)
        P, Bx, By = V0.shape[0], cx.numel(), cy.numel()
        S = torch.empty(P, Bx, By, dtype=_F32, device=x.device)
        ws = torch.empty(_lib.get_lib().mf_proj_kde_ws_bytes(P, Bx * By) // 8, dtype=torch.int64, device=x.device)
        call("mf_proj_kde2d_fwd", ptr(x), x.shape[0], x.shape[1], ptr(V0), ptr(V1), P, ptr(cx), Bx, float(sigma_x),
             int(radius_x), ptr(cy), By, float(sigma_y), int(radius_y), ptr(S), ptr(ws), stream_ptr(x))
        ctx.save_for_backward(x, V0, V1, cx, cy)
        ctx.args = (float(sigma_x), float(sigma_y), int(radius_x), int(radius_y))
        return S

    @staticmethod
    def backward(ctx, gS):
        x, V0, V1, cx, cy = ctx.saved_tensors
        sx, sy, rx, ry = ctx.args
        gx = torch.empty_like(x)
        call("mf_proj_kde2d_bwd", ptr(x), x.shape[0], x.shape[1], ptr(V0), ptr(V1), V0.shape[0], ptr(cx), cx.numel(), sx,
             rx, ptr(cy), cy.numel(), sy, ry, ptr(_f32c(gS)), ptr(gx), 0, stream_ptr(x))
        return gx, None, None, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------ weighted projections
def valid_weights(w: torch.Tensor) -> torch.Tensor:
    """w with every negative, NaN or infinite weight replaced by 0: what the weighted kernels count.  A zero weight passes
    through, so that it keeps its gradient."""
    return torch.where(torch.isfinite(w) & (w >= 0), w, torch.zeros_like(w))


def weight_max(w: torch.Tensor) -> torch.Tensor:
    """[1] device scalar: the largest valid weight, 0 if there is none.  Torch reductions only: no host synchronisation."""
    if w.numel() == 0:
        return torch.zeros(1, dtype=_F32, device=w.device)
    return valid_weights(w).amax().reshape(1)


def _check_weights(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    w = _f32c(w)
    if w.dim() != 1 or w.shape[0] != x.shape[0] or w.device != x.device:
        raise ValueError(f"weights must be a [{x.shape[0]}] tensor on {x.device} (got {tuple(w.shape)} on {w.device})")
    return w


class ProjWKde1dFn(torch.autograd.Function):
    """x[N,d], w[N], V[P,d] -> S[P,B] = sum_n w_n exp(-((x_n.V_p - c_k)/sigma)^2 / 2); differentiable in x and w
    (mf_proj_wkde1d_fwd / _bwd: one backward launch for both gradients, skipped per input by needs_input_grad)."""

    @staticmethod
    def forward(ctx, x, w, V, coords, sigma: float, radius: int):
        x, V, coords = _f32c(x), _f32c(V), _f32c(coords)
        w = _check_weights(x, w)
        P, B = V.shape[0], coords.numel()
        S = torch.empty(P, B, dtype=_F32, device=x.device)
        ws = torch.empty(_lib.get_lib().mf_proj_kde_ws_bytes(P, B) // 8, dtype=torch.int64, device=x.device)
        wmax = weight_max(w)
        call("mf_proj_wkde1d_fwd", ptr(x), ptr(w), ptr(wmax), x.shape[0], x.shape[1], ptr(V), P, ptr(coords), B, float(sigma),
             int(radius), ptr(S), ptr(ws), stream_ptr(x))
        ctx.save_for_backward(x, w, V, coords)
        ctx.sigma, ctx.radius = float(sigma), int(radius)
        return S

    @staticmethod
    def backward(ctx, gS):
        x, w, V, coords = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_w):
            return None, None, None, None, None, None
        gx = torch.empty_like(x) if need_x else None
        gw = torch.empty_like(w) if need_w else None
        call("mf_proj_wkde1d_bwd", ptr(x), ptr(w), x.shape[0], x.shape[1], ptr(V), V.shape[0], ptr(coords), coords.numel(),
             ctx.sigma, ctx.radius, ptr(_f32c(gS)), ptr(gx), ptr(gw), 0, stream_ptr(x))
        return gx, gw, None, None, None, None


class ProjWKde2dFn(torch.autograd.Function):
    """x[N,d], w[N], V0[P,d], V1[P,d] -> S[P,Bx,By] = sum_n w_n Kx_na Ky_nb; differentiable in x and w."""

    @staticmethod
    def forward(ctx, x, w, V0, V1, coords_x, coords_y, sigma_x: float, sigma_y: float, radius_x: int, radius_y: int):
        x, V0, V1, cx, cy = _f32c(x), _f32c(V0), _f32c(V1), _f32c(coords_x), _f32c(coords_y)
        w = _check_weights(x, w)
        P, Bx, By = V0.shape[0], cx.numel(), cy.numel()
        S = torch.empty(P, Bx, By, dtype=_F32, device=x.device)
        ws = torch.empty(_lib.get_lib().mf_proj_kde_ws_bytes(P, Bx * By) // 8, dtype=torch.int64, device=x.device)
        wmax = weight_max(w)
        call("mf_proj_wkde2d_fwd", ptr(x), ptr(w), ptr(wmax), x.shape[0], x.shape[1], ptr(V0), ptr(V1), P, ptr(cx), Bx,
             float(sigma_x), int(radius_x), ptr(cy), By, float(sigma_y), int(radius_y), ptr(S), ptr(ws), stream_ptr(x))
        ctx.save_for_backward(x, w, V0, V1, cx, cy)
        ctx.args = (float(sigma_x), float(sigma_y), int(radius_x), int(radius_y))
        return S

    @staticmethod
    def backward(ctx, gS):
        x, w, V0, V1, cx, cy = ctx.saved_tensors
        sx, sy, rx, ry = ctx.args
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_w):
            return (None,) * 10
        gx = torch.empty_like(x) if need_x else None
        gw = torch.empty_like(w) if need_w else None
        call("mf_proj_wkde2d_bwd", ptr(x), ptr(w), x.shape[0], x.shape[1], ptr(V0), ptr(V1), V0.shape[0], ptr(cx), cx.numel(),
             sx, rx, ptr(cy), cy.numel(), sy, ry, ptr(_f32c(gS)), ptr(gx), ptr(gw), 0, stream_ptr(x))
        return (gx, gw) + (None,) * 8


def proj_whist_sums_1d(x, w, V, edges) -> torch.Tensor:
    """[P,B] fp32 sums of w over the rows whose projection x.V_p lies in each bin (torch.histogram(weight=w) semantics)."""
    x, V, edges = _f32c(x), _f32c(V), _f32c(edges)
    w = _check_weights(x, w)
    P, B = V.shape[0], edges.numel() - 1
    sums = torch.empty(P, B, dtype=_F32, device=x.device)
    ws = torch.empty(_lib.get_lib().mf_proj_kde_ws_bytes(P, B) // 8, dtype=torch.int64, device=x.device)
    wmax = weight_max(w)
    call("mf_proj_whist1d_sums", ptr(x), ptr(w), ptr(wmax), x.shape[0], x.shape[1], ptr(V), P, ptr(edges), B, ptr(sums),
         ptr(ws), stream_ptr(x))
    return sums


def proj_whist_sums_2d(x, w, V0, V1, edges_x, edges_y) -> torch.Tensor:
    """[P,Bx,By] fp32 sums of w per cell (np.histogramdd(weights=w) semantics)."""
    x, V0, V1, ex, ey = _f32c(x), _f32c(V0), _f32c(V1), _f32c(edges_x), _f32c(edges_y)
    w = _check_weights(x, w)
    P, Bx, By = V0.shape[0], ex.numel() - 1, ey.numel() - 1
    sums = torch.empty(P, Bx, By, dtype=_F32, device=x.device)
    ws = torch.empty(_lib.get_lib().mf_proj_kde_ws_bytes(P, Bx * By) // 8, dtype=torch.int64, device=x.device)
    wmax = weight_max(w)
    call("mf_proj_whist2d_sums", ptr(x), ptr(w), ptr(wmax), x.shape[0], x.shape[1], ptr(V0), ptr(V1), P, ptr(ex), Bx,
         ptr(ey), By, ptr(sums), ptr(ws), stream_ptr(x))
    return sums


KDE_PLAN_KERNELS = ("kde1d_fwd", "kde1d_bwd", "kde2d_fwd", "kde2d_bwd")
KDE_PLAN_FIELDS = ("window", "block", "Pg", "groups", "per_wg", "split", "grid_x", "lds_bytes", "shift")   # MF_KDE_PLAN_*


def kde_plan(kernel: str, n: int, P: int, Bx: int, By: int = 1, radius_x: int = 4, radius_y: int = 4) -> dict:
    """The launch shape mf_proj_<kernel> takes for these sizes in this process (mf_proj_kde_plan: host arithmetic only)."""
    out = (C.c_int64 * len(KDE_PLAN_FIELDS))()
    call("mf_proj_kde_plan", KDE_PLAN_KERNELS.index(kernel), n, P, Bx, By, radius_x, radius_y, out)
    return dict(zip(KDE_PLAN_FIELDS, out))


class MultipoleKickFn(torch.autograd.Function):
    """u = MultipoleTransform(order, strength, skew)(x)  (mentflow/simulate/transform.py:98-143)."""

    @staticmethod
    def forward(ctx, x, order: int, k: float, skew: bool):
        x = _f32c(x)
        u = torch.empty_like(x)
        call("mf_multipole_kick_fwd", ptr(x), x.shape[0], x.shape[1], int(order), float(k), int(bool(skew)), ptr(u),
             stream_ptr(x))
        ctx.save_for_backward(x)
        ctx.args = (int(order), float(k), int(bool(skew)))
        return u

    @staticmethod
    def backward(ctx, gu):
        (x,) = ctx.saved_tensors
        order, k, skew = ctx.args
        gx = torch.empty_like(x)
        call("mf_multipole_kick_bwd", ptr(x), x.shape[0], x.shape[1], order, k, skew, ptr(_f32c(gu)), ptr(gx), stream_ptr(x))
        return gx, None, None, None


DISCREPANCY_KINDS = {"kld": 0, "mae": 1, "mse": 2}


class HistNormDiscFn(torch.autograd.Function):
    """S[P,bins] (+ meas[P,bins]) -> (ghat[P,bins], D[P]).

    normalize: marginal_pdf / joint_pdf normalisation (histogram.py:39-43, :69-73);
    discrepancy: mentflow/loss.py:7-17.  With meas=None only ghat is produced (D is an empty tensor)."""

    @staticmethod
    def forward(ctx, S, meas, normalize: bool, pre_scale: float, cell: float, eps: float, kind: int, pad: float,
                batch_div: float):
        S = _f32c(S)
        P = S.shape[0]
        bins = S[0].numel()
        meas_c = None if meas is None else _f32c(meas)
        ghat = torch.empty_like(S)
        D = torch.empty(P if meas is not None else 0, dtype=_F32, device=S.device)
        call("mf_hist_norm_discrepancy_fwd", ptr(S), P, bins, int(normalize), float(pre_scale), float(cell), float(eps),
             ptr(meas_c), int(kind), float(pad), float(batch_div), ptr(ghat), ptr(D) if meas is not None else None,
             stream_ptr(S))
        ctx.save_for_backward(S, meas_c) if meas is not None else ctx.save_for_backward(S)
        ctx.has_meas = meas is not None
        ctx.args = (int(normalize), float(pre_scale), float(cell), float(eps), int(kind), float(pad), float(batch_div))
        return ghat, D

    @staticmethod
    def backward(ctx, gghat, gD):
        if ctx.has_meas:
            S, meas = ctx.saved_tensors
        else:
            (S,) = ctx.saved_tensors
            meas, gD = None, None
        normalize, pre_scale, cell, eps, kind, pad, batch_div = ctx.args
        gS = torch.empty_like(S)
        gD_c = None if gD is None else _f32c(gD)
        gg_c = None if gghat is None else _f32c(gghat)
        call("mf_hist_norm_discrepancy_bwd", ptr(S), S.shape[0], S[0].numel(), normalize, pre_scale, cell, eps, ptr(meas),
             kind, pad, batch_div, ptr(gD_c), ptr(gg_c), ptr(gS), stream_ptr(S))
        return gS, None, None, None, None, None, None, None, None


class EntropySumsFn(torch.autograd.Function):
    """(x[N,d], logp[N]) -> [sum logp, sum |x|^2]  (entropy.py:58-62, prior.py:25-26)."""

    @staticmethod
    def forward(ctx, x, logp):
        x, logp = _f32c(x), _f32c(logp)
        out = torch.empty(2, dtype=_F32, device=x.device)
        scratch = torch.empty(2048, dtype=torch.float64, device=x.device)      # MF_ENTROPY_SCRATCH_DOUBLES
        call("mf_mc_entropy_sums", ptr(x), ptr(logp), x.shape[0], x.shape[1], ptr(out), ptr(scratch), stream_ptr(x))
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, gout):
        (x,) = ctx.saved_tensors
        gout = _f32c(gout)
        gx = torch.empty_like(x)
        call("mf_scale_rows", ptr(x), x.shape[0], x.shape[1], ptr(gout[1:2]), 2.0, ptr(gx), 0, stream_ptr(x))
        glogp = gout[0].expand(x.shape[0]).contiguous()
        return gx, glogp


class KnnEntropyFn(torch.autograd.Function):
    """x[N,d] -> (H, idx[N], rho2[N], sum ln rho): the Kozachenko-Leonenko negative entropy with the k-th nearest other point
    (include/mentflow_hip.h, mf_knn_entropy_*).  Only H is differentiable.  chunks = 0: the built-in cut of the candidate
    range over the grid."""

    @staticmethod
    def forward(ctx, x, k: int, chunks: int):
        x = _f32c(x)
        if x.dim() != 2:
            raise ValueError(f"knn_entropy: x[N, d] expected (got {tuple(x.shape)})")
        n, d = x.shape
        ptr(x)                                             # a CPU tensor is refused before anything is allocated for it
        nbytes = int(_lib.get_lib().mf_knn_entropy_ws_bytes(n, d, int(k), int(chunks)))
        if nbytes < 0:
            raise RuntimeError(f"mf_knn_entropy_ws_bytes failed: {_lib.get_lib().mf_last_error().decode()}")
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
        H = torch.empty((), dtype=_F32, device=x.device)
        S = torch.empty((), dtype=torch.float64, device=x.device)
        idx = torch.empty(n, dtype=torch.int32, device=x.device)
        rho2 = torch.empty(n, dtype=_F32, device=x.device)
        call("mf_knn_entropy_fwd", ptr(x), n, d, int(k), int(chunks), ptr(H), ptr(S), ptr(idx), ptr(rho2), ptr(ws),
             stream_ptr(x))
        ctx.save_for_backward(x, idx, rho2)
        ctx.mark_non_differentiable(idx, rho2, S)
        return H, idx, rho2, S

    @staticmethod
    def backward(ctx, gH, _gidx, _grho2, _gS):
        x, idx, rho2 = ctx.saved_tensors
        n, d = x.shape
        gx = torch.empty_like(x)
        call("mf_knn_entropy_bwd", ptr(x), n, d, ptr(idx), ptr(rho2), ptr(_f32c(gH).reshape(1)), -float(d) / float(n), ptr(gx),
             stream_ptr(x))
        return gx, None, None


def knn_entropy(x: torch.Tensor, k: int = 5, _chunks: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(H, idx, rho2, sum_ln_rho) of KnnEntropyFn.  _chunks is a private override of the number of candidate chunks (tests
    reach the multi-chunk merge with a few thousand points through it); idx and rho2 do not depend on it."""
    return KnnEntropyFn.apply(x, int(k), int(_chunks))


class CovEntropyFn(torch.autograd.Function):
    """x[N,d] -> H = -3 ln(2 pi e) - ln(sqrt(det cov x) + pad)  (entropy.py:35-38; mf_cov_entropy_*)."""

    @staticmethod
    def forward(ctx, x, pad: float):
        x = _f32c(x)
        if x.dim() != 2:
            raise ValueError(f"cov_entropy: x[N, d] expected (got {tuple(x.shape)})")
        n, d = x.shape
        ptr(x)
        nws = int(_lib.get_lib().mf_cov_entropy_ws_doubles(n, d))
        if nws < 0:
            raise RuntimeError(f"mf_cov_entropy_ws_doubles failed: {_lib.get_lib().mf_last_error().decode()}")
        ws = torch.empty(nws, dtype=torch.float64, device=x.device)
        aux = torch.empty(d + d * d, dtype=torch.float64, device=x.device)
        H = torch.empty((), dtype=_F32, device=x.device)
        call("mf_cov_entropy_fwd", ptr(x), n, d, float(pad), ptr(H), ptr(aux), ptr(ws), stream_ptr(x))
        ctx.save_for_backward(x, aux)
        return H

    @staticmethod
    def backward(ctx, gH):
        x, aux = ctx.saved_tensors
        gx = torch.empty_like(x)
        call("mf_cov_entropy_bwd", ptr(x), x.shape[0], x.shape[1], ptr(aux), ptr(_f32c(gH).reshape(1)), ptr(gx), stream_ptr(x))
        return gx, None


def cov_entropy(x: torch.Tensor, pad: float = 1.0e-12) -> torch.Tensor:
    return CovEntropyFn.apply(x, float(pad))


def proj_hist_counts_1d(x, V, edges) -> torch.Tensor:
    x, V, edges = _f32c(x), _f32c(V), _f32c(edges)
    P, B = V.shape[0], edges.numel() - 1
    counts = torch.empty(P, B, dtype=torch.int32, device=x.device)
    call("mf_proj_hist1d_counts", ptr(x), x.shape[0], x.shape[1], ptr(V), P, ptr(edges), B, ptr(counts), stream_ptr(x))
    return counts


def proj_hist_counts_2d(x, V0, V1, edges_x, edges_y) -> torch.Tensor:
    x, V0, V1, ex, ey = _f32c(x), _f32c(V0), _f32c(V1), _f32c(edges_x), _f32c(edges_y)
    P, Bx, By = V0.shape[0], ex.numel() - 1, ey.numel() - 1
    counts = torch.empty(P, Bx, By, dtype=torch.int32, device=x.device)
    call("mf_proj_hist2d_counts", ptr(x), x.shape[0], x.shape[1], ptr(V0), ptr(V1), P, ptr(ex), Bx, ptr(ey), By,
         ptr(counts), stream_ptr(x))
    return counts


# ------------------------------------------------------------------------------------------------ classical MENT
# Thin wrappers over mf_ment_* (include/mentflow_hip.h); mentflow_amd/ment.py builds the slot descriptors.  `prior` is the
# (kind, a, lognorm) triple of the header: kind 0 none, 1 Gaussian, 2 uniform box.
MENT_DESC = 24


def _host_i64(values):
    arr = (C.c_int64 * len(values))(*[int(v) for v in values])
    return arr, C.cast(arr, C.c_void_p)


def ment_prob(x: torch.Tensor, desc: torch.Tensor, meta: torch.Tensor, tables: torch.Tensor, prior=(0, 0.0, 0.0),
              out: Optional[torch.Tensor] = None, multiply: bool = False) -> torch.Tensor:
    """prod over slots of the interpolated Lagrange functions at x[n, d], times the prior; multiply=True: out *= that."""
    x, tables = _f32c(x), _f32c(tables)
    if out is None:
        out = torch.empty(x.shape[0], dtype=_F32, device=x.device)
    call("mf_ment_prob", ptr(x), x.shape[0], x.shape[1], desc.shape[0], ptr(desc), ptr(meta), ptr(tables), tables.numel(),
         int(prior[0]), float(prior[1]), float(prior[2]), int(bool(multiply)), ptr(out), stream_ptr(x))
    return out


def ment_prob_grid(coords: List[torch.Tensor], desc, meta, tables, prior=(0, 0.0, 0.0)) -> Tuple[torch.Tensor, torch.Tensor]:
    """(prob[prod(shape)], fp64 block sums of prob + 1e-15) on the implicit grid of the given per-axis cell centres."""
    tables = _f32c(tables)
    cat = _f32c(torch.cat([c.reshape(-1) for c in coords]))
    shape = [c.numel() for c in coords]
    n = math.prod(shape)
    prob = torch.empty(n, dtype=_F32, device=cat.device)
    sums = torch.empty(max(1, int(_lib.get_lib().mf_ment_blocks(n))), dtype=torch.float64, device=cat.device)
    keep, shp = _host_i64(shape)
    call("mf_ment_prob_grid", ptr(cat), shp, len(shape), desc.shape[0], ptr(desc), ptr(meta), ptr(tables), tables.numel(),
         int(prior[0]), float(prior[1]), float(prior[2]), ptr(prob), ptr(sums), stream_ptr(cat))
    return prob, sums


def ment_block_sums(prob: torch.Tensor) -> torch.Tensor:
    prob = _f32c(prob.reshape(-1))
    sums = torch.empty(max(1, int(_lib.get_lib().mf_ment_blocks(prob.numel()))), dtype=torch.float64, device=prob.device)
    call("mf_ment_block_sums", ptr(prob), prob.numel(), ptr(sums), stream_ptr(prob))
    return sums


def ment_sample(prob: torch.Tensor, shape, block_sums: torch.Tensor, edges: List[torch.Tensor], size: int, noise: bool,
                rnd: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x[size, len(shape)]: cells drawn with probability (prob + 1e-15) / sum, points uniform in the cell (+ the
    0.5 U(-delta, delta) noise per axis).  rnd: [size, 1 + 2 d] uniforms (default torch.rand on the device): column 0
    picks the cell by inverse CDF, columns 1..d place the point, columns d+1..2d are the noise.  A cell with prob = 0
    keeps the weight 1e-15, so rnd[:, 0] = 0 draws cell 0 whatever prob[0] is.  Column 0 is one fp32 number: a draw
    resolves the CDF to 2^-24 of its total, and at most 2^24 distinct cells can be reached."""
    prob = _f32c(prob.reshape(-1))
    d = len(shape)
    if rnd is None:
        rnd = torch.rand(int(size), 1 + 2 * d, device=prob.device)
    rnd = _f32c(rnd)
    cat = _f32c(torch.cat([e.reshape(-1).to(prob.device, _F32) for e in edges]))
    prefix = torch.empty(block_sums.numel() + 1, dtype=torch.float64, device=prob.device)
    x = torch.empty(int(size), d, dtype=_F32, device=prob.device)
    keep, shp = _host_i64(shape)
    call("mf_ment_sample", ptr(prob), shp, d, ptr(block_sums), ptr(prefix), ptr(cat), ptr(rnd), int(size), int(bool(noise)),
         ptr(x), stream_ptr(prob))
    return x


def ment_integrate(minv: torch.Tensor, coords: List[torch.Tensor], meas_axes, desc, meta, tables,
                   prior=(0, 0.0, 0.0)) -> torch.Tensor:
    """pred[b] = sum_t prob(Minv u_bt) (fp64 sums, fixed order): coords[a] = the u coordinates of axis a (bin centres on the
    measured axes, the integration grid on the others).  Returns the flat [nbins] projection (ij order of meas_axes)."""
    tables = _f32c(tables)
    d = len(coords)
    cat = _f32c(torch.cat([c.reshape(-1) for c in coords]))
    counts = [c.numel() for c in coords]
    nbins = math.prod(counts[a] for a in meas_axes)
    npoints = math.prod(counts) // nbins
    m = minv.detach().to("cpu", torch.float32).contiguous().reshape(-1).tolist()
    mh = (C.c_float * (d * d))(*m)
    keep, cnt = _host_i64(counts)
    ma = (C.c_int32 * len(meas_axes))(*[int(a) for a in meas_axes])
    partial = torch.empty(max(1, int(_lib.get_lib().mf_ment_integrate_ws_doubles(nbins, npoints))), dtype=torch.float64,
                          device=cat.device)
    pred = torch.empty(nbins, dtype=_F32, device=cat.device)
    call("mf_ment_integrate", d, C.cast(mh, C.c_void_p), ptr(cat), cnt, len(meas_axes), C.cast(ma, C.c_void_p),
         desc.shape[0], ptr(desc), ptr(meta), ptr(tables), tables.numel(), int(prior[0]), float(prior[1]), float(prior[2]),
         ptr(partial), ptr(pred), stream_ptr(cat))
    return pred


def _check_slots(name: str, desc, meta) -> int:
    """The shape check of the slot descriptors that every MENT entry point taking them shares; returns nslot."""
    nslot = desc.shape[0]
    if desc.dtype != _F32 or tuple(desc.shape) != (nslot, MENT_DESC) or meta.dtype != torch.int32 or tuple(meta.shape) != (nslot, 4):
        raise RuntimeError(f"{name}: desc float32[nslot, {MENT_DESC}] and meta int32[nslot, 4] expected (got "
                           f"{desc.dtype}{tuple(desc.shape)}, {meta.dtype}{tuple(meta.shape)})")
    return nslot


def _check_chain_steps(name: str, x, desc, meta, tables, noise, scale, accepted, step_offset, keep_from, keep_every, out,
                       extra=()) -> Tuple[int, int, int, int, int, int]:
    """The argument checks that mcmc_ment_steps, mala_ment_steps and ais_ment_steps share; `name` opens the messages.  Returns
    (chains, d, steps, step_offset, keep_from, keep_every)."""
    if x.dim() != 2 or not 1 <= x.shape[1] <= 8:
        raise RuntimeError(f"{name}: x[chains, d <= 8] expected (got {tuple(x.shape)})")
    chains, d = x.shape
    for what, t in (("x", x), ("noise", noise), ("scale", scale), ("tables", tables)):
        if t.dtype != _F32:
            raise RuntimeError(f"{name}: {what} must be float32 (got {t.dtype})")
    if accepted.dtype != torch.int32 or tuple(accepted.shape) != (chains,):
        raise RuntimeError(f"{name}: accepted must be int32[{chains}] (got {accepted.dtype}{tuple(accepted.shape)})")
    if noise.dim() != 3 or tuple(noise.shape[1:]) != (d + 1, chains):
        raise RuntimeError(f"{name}: noise[steps, {d + 1}, {chains}] expected (got {tuple(noise.shape)})")
    if tuple(scale.shape) != (d,):
        raise RuntimeError(f"{name}: scale[{d}] expected (got {tuple(scale.shape)})")
    _check_slots(name, desc, meta)
    steps = noise.shape[0]
    step_offset, keep_from, keep_every = int(step_offset), int(keep_from), int(keep_every)
    if step_offset < 0 or keep_from < 0 or keep_every < 1:
        raise RuntimeError(f"{name}: step_offset, keep_from >= 0 and keep_every >= 1 expected")
    if out is not None:
        last = step_offset + steps - 1 - keep_from                   # rows this call may write: those of steps g <= last
        need = last // keep_every + 1 if last >= 0 else 0
        if out.dtype != _F32 or out.dim() != 3 or tuple(out.shape[1:]) != (chains, d) or out.shape[0] < need:
            raise RuntimeError(f"{name}: out[>= {need}, {chains}, {d}] float32 expected (got {out.dtype}"
                               f"{tuple(out.shape)})")
    for t in (noise, scale, accepted, out, desc, meta, tables, *extra):
        if t is not None and t.device != x.device:
            raise RuntimeError(f"{name}: all tensors must be on {x.device} (got one on {t.device})")
    return chains, d, steps, step_offset, keep_from, keep_every


def mcmc_ment_steps(x: torch.Tensor, desc: torch.Tensor, meta: torch.Tensor, tables: torch.Tensor, prior, noise: torch.Tensor,
                    scale: torch.Tensor, accepted: torch.Tensor, step_offset: int = 0, keep_from: int = 0, keep_every: int = 1,
                    out: Optional[torch.Tensor] = None) -> None:
    """Advance the Metropolis-Hastings chains x[chains, d] IN PLACE by noise.shape[0] steps on the MENT density of the slots
    (mf_mcmc_ment_steps, include/mentflow_hip.h).  noise[steps, d + 1, chains]: normal proposal rows and a uniform last row;
    scale[d] on the device; accepted[chains] int32 is added to; out[n_keep, chains, d] (or None) receives the state after every
    step g = step_offset + t with g >= keep_from and (g - keep_from) % keep_every == 0."""
    chains, d, steps, step_offset, keep_from, keep_every = _check_chain_steps(
        "mcmc_ment_steps", x, desc, meta, tables, noise, scale, accepted, step_offset, keep_from, keep_every, out)
    call("mf_mcmc_ment_steps", ptr(x), chains, d, desc.shape[0], ptr(desc), ptr(meta), ptr(tables), tables.numel(),
         int(prior[0]), float(prior[1]), float(prior[2]), ptr(noise), steps, step_offset, ptr(scale), keep_from, keep_every,
         ptr(out), ptr(accepted), stream_ptr(x))


def _check_langevin(name: str, chains: int, drift_clip, logp) -> float:
    """What mala_ment_steps and ais_ment_steps check on top of _check_chain_steps; returns drift_clip as a float."""
    drift_clip = float(drift_clip)
    if not drift_clip >= 0.0:
        raise RuntimeError(f"{name}: drift_clip >= 0 expected (got {drift_clip})")
    if logp is not None and (logp.dtype != _F32 or tuple(logp.shape) != (chains,)):
        raise RuntimeError(f"{name}: logp must be float32[{chains}] (got {logp.dtype}{tuple(logp.shape)})")
    return drift_clip


def mala_ment_steps(x: torch.Tensor, desc: torch.Tensor, meta: torch.Tensor, tables: torch.Tensor, prior, noise: torch.Tensor,
                    scale: torch.Tensor, accepted: torch.Tensor, drift_clip: float = 1.0, step_offset: int = 0,
                    keep_from: int = 0, keep_every: int = 1, out: Optional[torch.Tensor] = None,
                    logp: Optional[torch.Tensor] = None) -> None:
    """Advance the Metropolis-adjusted Langevin chains x[chains, d] IN PLACE by noise.shape[0] steps on the MENT density of the
    slots (mf_mala_ment_steps, include/mentflow_hip.h).  Arguments as mcmc_ment_steps takes them, plus drift_clip >= 0 (the drift
    is truncated to that many proposal standard deviations per axis) and logp[chains] float32 (or None), which receives the
    log-density of the final states."""
    chains, d, steps, step_offset, keep_from, keep_every = _check_chain_steps(
        "mala_ment_steps", x, desc, meta, tables, noise, scale, accepted, step_offset, keep_from, keep_every, out, extra=(logp,))
    drift_clip = _check_langevin("mala_ment_steps", chains, drift_clip, logp)
    call("mf_mala_ment_steps", ptr(x), chains, d, desc.shape[0], ptr(desc), ptr(meta), ptr(tables), tables.numel(),
         int(prior[0]), float(prior[1]), float(prior[2]), ptr(noise), steps, step_offset, ptr(scale), drift_clip, keep_from,
         keep_every, ptr(out), ptr(accepted), ptr(logp), stream_ptr(x))


def ais_ment_steps(x: torch.Tensor, desc: torch.Tensor, meta: torch.Tensor, tables: torch.Tensor, prior, noise: torch.Tensor,
                   betas: torch.Tensor, steps_per_temp: int, scale: torch.Tensor, base_mean, base_scale, logw: torch.Tensor,
                   accepted: torch.Tensor, drift_clip: float = 1.0, temp_offset: int = 0, ntemps: Optional[int] = None,
                   out: Optional[torch.Tensor] = None, logp: Optional[torch.Tensor] = None) -> None:
    """Walk the annealed-importance-sampling chains x[chains, d] IN PLACE through `ntemps` temperatures of the ladder
    betas[K + 1] (float32 on the device, non-decreasing in [0, 1]) from index temp_offset on (default: to the end of the
    ladder), from the Gaussian base N(base_mean, diag base_scale^2) (host sequences of d floats) towards the MENT density of
    the slots (mf_ais_ment_steps, include/mentflow_hip.h).  Per temperature logw[chains] (float64, in / out) takes its
    increment and the chains take steps_per_temp >= 0 Langevin transitions on the tempered density, with scale, drift_clip,
    accepted and logp as mala_ment_steps takes them.  noise[ntemps * steps_per_temp, d + 1, chains]; out (or None)
    [>= (temp_offset + ntemps) * steps_per_temp, chains, d] receives the state after every transition at its global row."""
    name = "ais_ment_steps"
    steps_per_temp, temp_offset = int(steps_per_temp), int(temp_offset)
    if betas.dim() != 1 or betas.dtype != _F32 or betas.numel() < 1:
        raise RuntimeError(f"{name}: betas must be float32[K + 1] (got {betas.dtype}{tuple(betas.shape)})")
    ntemps = betas.numel() - 1 - temp_offset if ntemps is None else int(ntemps)
    if steps_per_temp < 0 or temp_offset < 0 or ntemps < 0 or temp_offset + ntemps + 1 > betas.numel():
        raise RuntimeError(f"{name}: steps_per_temp >= 0 and 0 <= temp_offset <= temp_offset + ntemps <= {betas.numel() - 1} "
                           f"expected (got {steps_per_temp}, {temp_offset}, {ntemps})")
    if noise.dim() == 3 and noise.shape[0] != ntemps * steps_per_temp:
        raise RuntimeError(f"{name}: noise[{ntemps * steps_per_temp}, d + 1, chains] expected (got {tuple(noise.shape)})")
    chains, d = _check_chain_steps(name, x, desc, meta, tables, noise, scale, accepted, temp_offset * steps_per_temp, 0, 1, out,
                                   extra=(logp, logw, betas))[:2]
    drift_clip = _check_langevin(name, chains, drift_clip, logp)
    if logw is None or logw.dtype != torch.float64 or tuple(logw.shape) != (chains,):
        raise RuntimeError(f"{name}: logw must be float64[{chains}]")
    mean, base = [float(v) for v in base_mean], [float(v) for v in base_scale]
    if len(mean) != d or len(base) != d or not all(0.0 < b < math.inf for b in base) or any(m != m for m in mean):
        raise RuntimeError(f"{name}: base_mean[{d}] and base_scale[{d}] > 0 expected (got {mean}, {base})")
    mh, bh = (C.c_float * d)(*mean), (C.c_float * d)(*base)
    call("mf_ais_ment_steps", ptr(x), chains, d, desc.shape[0], ptr(desc), ptr(meta), ptr(tables), tables.numel(),
         int(prior[0]), float(prior[1]), float(prior[2]), ptr(noise), ptr(betas), betas.numel(), ntemps, temp_offset,
         steps_per_temp, ptr(scale), drift_clip, C.cast(mh, C.c_void_p), C.cast(bh, C.c_void_p), ptr(logw), ptr(out),
         ptr(accepted), ptr(logp), stream_ptr(x))


def smc_resample(x: torch.Tensor, logw: torch.Tensor, u: torch.Tensor, groups: int,
                 ess_threshold: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(x_out[chains, d], ancestors int32[chains], stats float64[groups, 4]) of mf_smc_resample (include/mentflow_hip.h):
    systematic resampling of the weighted states x[chains, d] in `groups` islands of chains / groups consecutive chains, each
    from its own uniform u[groups] (float64 on the device) and only where its effective sample size is below ess_threshold
    times its size.  logw[chains] (float64) is updated IN PLACE: the log-weights of an island that resampled all become its
    log mean weight, those of the others keep their bits.  stats[g] = (log mean weight, ess, resampled 0 / 1, max logw).  No
    host synchronisation: every decision is taken on the device."""
    name = "smc_resample"
    if x.dim() != 2 or not 1 <= x.shape[1] <= 8:
        raise RuntimeError(f"{name}: x[chains, d <= 8] expected (got {tuple(x.shape)})")
    chains, d = x.shape
    groups = int(groups)
    if x.dtype != _F32:
        raise RuntimeError(f"{name}: x must be float32 (got {x.dtype})")
    if groups < 1 or chains % groups != 0:
        raise RuntimeError(f"{name}: groups >= 1 that divides the {chains} chains expected (got {groups})")
    if logw is None or logw.dtype != torch.float64 or tuple(logw.shape) != (chains,):
        raise RuntimeError(f"{name}: logw must be float64[{chains}]")
    if u is None or u.dtype != torch.float64 or tuple(u.shape) != (groups,):
        raise RuntimeError(f"{name}: u must be float64[{groups}]")
    for t in (logw, u):
        if t.device != x.device:
            raise RuntimeError(f"{name}: all tensors must be on {x.device} (got one on {t.device})")
    x_out = torch.empty_like(x)
    ancestors = torch.empty(chains, dtype=torch.int32, device=x.device)
    stats = torch.empty(groups, 4, dtype=torch.float64, device=x.device)
    scratch = torch.empty(max(chains, 1), dtype=torch.float64, device=x.device)
    call("mf_smc_resample", ptr(x), ptr(x_out), chains, d, groups, ptr(logw), ptr(u), float(ess_threshold), ptr(ancestors),
         ptr(stats), ptr(scratch), stream_ptr(x))
    return x_out, ancestors, stats


def ment_logprob(x: torch.Tensor, desc: torch.Tensor, meta: torch.Tensor, tables: torch.Tensor, prior=(0, 0.0, 0.0),
                 want_grad: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(logp[n], grad[n, d] or None) of mf_ment_logprob (include/mentflow_hip.h): the sum over slots of log clamp(h, 0, 1e10)
    at x[n, d] plus the log-prior, and its gradient with respect to x.  -inf outside the support (gradient row 0), NaN for a NaN
    coordinate (gradient row NaN); finite where the product of ment_prob under- or overflows."""
    if x.dim() != 2 or not 1 <= x.shape[1] <= 8:
        raise RuntimeError(f"ment_logprob: x[n, d <= 8] expected (got {tuple(x.shape)})")
    x, tables = _f32c(x), _f32c(tables)
    nslot = _check_slots("ment_logprob", desc, meta)
    for t in (desc, meta, tables):
        if t.device != x.device:
            raise RuntimeError(f"ment_logprob: all tensors must be on {x.device} (got one on {t.device})")
    n, d = x.shape
    logp = torch.empty(n, dtype=_F32, device=x.device)
    grad = torch.empty(n, d, dtype=_F32, device=x.device) if want_grad else None
    call("mf_ment_logprob", ptr(x), n, d, nslot, ptr(desc), ptr(meta), ptr(tables), tables.numel(), int(prior[0]),
         float(prior[1]), float(prior[2]), ptr(logp), ptr(grad), stream_ptr(x))
    return logp, grad


def ment_logprob_table_grad(x: torch.Tensor, desc: torch.Tensor, meta: torch.Tensor, tables: torch.Tensor, logp: torch.Tensor,
                            weight: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(grad_log, grad_tab), both [tables.numel()], of mf_ment_logprob_tables_bwd (include/mentflow_hip.h): the gradient of
    sum_n weight[n] logp[n] with respect to log tables (the weighted histogram of responsibilities) and to tables (that divided by
    the table, 0 where the table is not positive).  logp[n] is what ment_logprob returned for the same x and slots, weight[n] the
    upstream gradient; rows with logp = -inf are ignored whatever their weight.  A NaN logp with a non-zero weight, or a
    non-finite weight on a row with finite logp, makes both results all NaN (decided on the device: no host synchronisation).
    Integer accumulation: bitwise reproducible and independent of the order of the rows."""
    if x.dim() != 2 or not 1 <= x.shape[1] <= 8:
        raise RuntimeError(f"ment_logprob_table_grad: x[n, d <= 8] expected (got {tuple(x.shape)})")
    x, tables, logp, weight = _f32c(x), _f32c(tables), _f32c(logp), _f32c(weight)
    n, d = x.shape
    nslot = _check_slots("ment_logprob_table_grad", desc, meta)
    if tuple(logp.shape) != (n,) or tuple(weight.shape) != (n,):
        raise RuntimeError(f"ment_logprob_table_grad: logp[{n}] and weight[{n}] expected (got {tuple(logp.shape)}, "
                           f"{tuple(weight.shape)})")
    for t in (desc, meta, tables, logp, weight):
        if t.device != x.device:
            raise RuntimeError(f"ment_logprob_table_grad: all tensors must be on {x.device} (got one on {t.device})")
    size = tables.numel()
    if n > 0:
        wmax = torch.where(torch.isfinite(logp), weight.abs(), torch.zeros_like(weight)).amax().reshape(1)
    else:
        wmax = torch.zeros(1, dtype=_F32, device=x.device)
    acc = torch.empty(max(size, 1), dtype=torch.int64, device=x.device)
    status = torch.empty(1, dtype=torch.int32, device=x.device)
    grad_log = torch.empty(size, dtype=_F32, device=x.device)
    grad_tab = torch.empty(size, dtype=_F32, device=x.device)
    call("mf_ment_logprob_tables_bwd", ptr(x), n, d, nslot, ptr(desc), ptr(meta), ptr(tables), size, ptr(logp), ptr(weight),
         ptr(wmax), ptr(acc), ptr(grad_log), ptr(grad_tab), ptr(status), stream_ptr(x))
    bad = status != 0
    nan = torch.full_like(grad_log, float("nan"))
    return torch.where(bad, nan, grad_log), torch.where(bad, nan, grad_tab)


class MentLogProbFn(torch.autograd.Function):
    """x[n, d] -> logp[n] of ment_logprob, differentiable in x and in tables: one kernel launch computes the value and, when x
    needs a gradient, d logp / dx, which the backward scales by the incoming gradient.  Rows with logp = -inf pass no gradient
    whatever comes in (0 * inf would be NaN).  When tables needs a gradient the backward launches ment_logprob_table_grad on the
    saved x and logp: d / d tables[e] = sum_n g[n] rho_e(n) / tables[e], 0 where tables[e] <= 0.  Descriptors and the prior are
    constants; the backward is not differentiable again."""

    @staticmethod
    def forward(ctx, x, desc, meta, tables, prior):
        want = bool(ctx.needs_input_grad[0])
        ctx.want_tables = bool(ctx.needs_input_grad[3])
        logp, grad = ment_logprob(x, desc, meta, tables, prior, want_grad=want)
        if ctx.want_tables:
            ctx.save_for_backward(grad, logp, x, desc, meta, tables)
        elif want:
            ctx.save_for_backward(grad, logp)
        return logp

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        grad, logp = ctx.saved_tensors[:2]
        gx = gt = None
        if grad is not None:
            gx = torch.where(torch.isneginf(logp)[:, None], torch.zeros_like(grad), g[:, None] * grad)
        if ctx.want_tables:
            x, desc, meta, tables = ctx.saved_tensors[2:]
            gt = ment_logprob_table_grad(x, desc, meta, tables, logp, g.contiguous())[1].reshape(tables.shape)
        return gx, None, None, gt, None


# ------------------------------------------------------------------------------------------------ sliced Wasserstein distance
# Thin wrappers over mf_swd_* / mf_segsort_* (include/mentflow_hip.h).  sliced_wasserstein is the evaluation path (keys-only sort,
# no graph); SlicedWassersteinFn at the end of the section is the differentiable one.
def swd_project(x: torch.Tensor, directions: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """u[P, N] = (x[N, d] @ directions[d, P]).T, projection-major: each projection is one contiguous segment."""
    x, directions = _f32c(x), _f32c(directions)
    if x.dim() != 2 or directions.dim() != 2 or directions.shape[0] != x.shape[1]:
        raise ValueError(f"swd_project: x[N, d] and directions[d, P] expected (got {tuple(x.shape)}, {tuple(directions.shape)})")
    P, n = directions.shape[1], x.shape[0]
    if out is None:
        out = torch.empty(P, n, dtype=_F32, device=x.device)
    call("mf_swd_project", ptr(x), n, x.shape[1], ptr(directions), P, ptr(out), stream_ptr(x))
    return out


def segmented_sort(keys: torch.Tensor, out: Optional[torch.Tensor] = None, _tile_log2: int = 0) -> torch.Tensor:
    """Each row of keys[P, N] in ascending order (torch.sort's convention: NaN last); `out` may be `keys`.  _tile_log2 is a
    private override of the LDS tile (tests reach the multi-tile merge passes with a few thousand keys through it)."""
    keys = _f32c(keys)
    if keys.dim() != 2:
        raise ValueError(f"segmented_sort: keys[P, N] expected (got {tuple(keys.shape)})")
    P, n = keys.shape
    if out is None:
        out = torch.empty_like(keys)
    nbytes = int(_lib.get_lib().mf_segsort_workspace_bytes(P, n, int(_tile_log2)))
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=keys.device) if nbytes > 0 else None
    call("mf_segsort_f32", ptr(keys), P, n, int(_tile_log2), ptr(out), ptr(ws), stream_ptr(keys))
    return out


def swd_quantile_cost(u: torch.Tensor, v: torch.Tensor, p: float = 2.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(wpp[P] fp64, dist 0-dim fp32) of row-wise SORTED u[P, N1], v[P, N2]: wpp = W_p^p of the two uniform-weight empirical
    measures per row, dist = (mean wpp)^(1/p)."""
    u, v = _f32c(u), _f32c(v)
    if u.dim() != 2 or v.dim() != 2 or u.shape[0] != v.shape[0]:
        raise ValueError(f"swd_quantile_cost: u[P, N1] and v[P, N2] expected (got {tuple(u.shape)}, {tuple(v.shape)})")
    P = u.shape[0]
    nws = int(_lib.get_lib().mf_swd_cost_ws_doubles(P, u.shape[1], v.shape[1]))
    partial = torch.empty(max(1, nws), dtype=torch.float64, device=u.device)
    wpp = torch.empty(P, dtype=torch.float64, device=u.device)
    dist = torch.empty((), dtype=_F32, device=u.device)
    call("mf_swd_quantile_cost", ptr(u), u.shape[1], ptr(v), v.shape[1], P, float(p), ptr(partial), ptr(wpp), ptr(dist),
         stream_ptr(u))
    return wpp, dist


def sliced_wasserstein(x1: torch.Tensor, x2: torch.Tensor, directions: torch.Tensor, p: float = 2.0) -> torch.Tensor:
    """(mean over the columns of directions[d, P] of W_p^p(x1 . dir, x2 . dir))^(1/p) as a 0-dim fp32 device tensor; no
    device-to-host copy.  Equal sizes: both clouds are projected into one [2P, N] buffer and sorted by one launch sequence."""
    P = directions.shape[1]
    if x1.shape[0] == x2.shape[0]:
        u = torch.empty(2 * P, x1.shape[0], dtype=_F32, device=x1.device)
        swd_project(x1, directions, out=u[:P])
        swd_project(x2, directions, out=u[P:])
        segmented_sort(u, out=u)
        u1, u2 = u[:P], u[P:]
    else:
        u1 = swd_project(x1, directions)
        u2 = swd_project(x2, directions)
        segmented_sort(u1, out=u1)
        segmented_sort(u2, out=u2)
    return swd_quantile_cost(u1, u2, p)[1]


def segmented_sort_pairs(keys: torch.Tensor, out: Optional[torch.Tensor] = None, perm: Optional[torch.Tensor] = None,
                         _tile_log2: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sorted, perm): segmented_sort's values bit for bit, and perm[s, r] (int32) = the position in row s of the key at rank r:
    ascending mapped keys (-0.0 before +0.0, NaN last), ties by ascending position; always a permutation.  `out` may be `keys`."""
    keys = _f32c(keys)
    if keys.dim() != 2:
        raise ValueError(f"segmented_sort_pairs: keys[P, N] expected (got {tuple(keys.shape)})")
    P, n = keys.shape
    if out is None:
        out = torch.empty_like(keys)
    if perm is None:
        perm = torch.empty(P, n, dtype=torch.int32, device=keys.device)
    nbytes = int(_lib.get_lib().mf_segsort_pairs_workspace_bytes(P, n, int(_tile_log2)))
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=keys.device) if nbytes > 0 else None
    call("mf_segsort_pairs_f32", ptr(keys), P, n, int(_tile_log2), ptr(out), ptr(perm), ptr(ws), stream_ptr(keys))
    return out, perm


def swd_quantile_cost_bwd(u: torch.Tensor, v: torch.Tensor, wpp: torch.Tensor, gdist: torch.Tensor, p: float = 2.0,
                          perm_u: Optional[torch.Tensor] = None, perm_v: Optional[torch.Tensor] = None,
                          need_u: bool = True, need_v: bool = True) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(gu[P, N1], gv[P, N2]) = gdist * d dist / d (u, v) for the sorted rows and wpp of swd_quantile_cost; gdist is a device
    scalar.  With perm_* (segmented_sort_pairs) the gradient of rank r is stored at position perm[s, r], i.e. in the order of
    the unsorted rows; a side that is not needed is None."""
    u, v = _f32c(u), _f32c(v)
    if u.dim() != 2 or v.dim() != 2 or u.shape[0] != v.shape[0]:
        raise ValueError(f"swd_quantile_cost_bwd: u[P, N1] and v[P, N2] expected (got {tuple(u.shape)}, {tuple(v.shape)})")
    P = u.shape[0]
    if wpp.dtype != torch.float64 or wpp.numel() != P or not wpp.is_contiguous():
        raise ValueError(f"swd_quantile_cost_bwd: wpp[{P}] float64 expected (got {wpp.dtype}{tuple(wpp.shape)})")
    gdist = _f32c(gdist)
    if gdist.numel() != 1:
        raise ValueError(f"swd_quantile_cost_bwd: gdist must hold one value (got {tuple(gdist.shape)})")
    for t, side in ((perm_u, u), (perm_v, v)):
        if t is not None and (t.dtype != torch.int32 or t.shape != side.shape or not t.is_contiguous()):
            raise ValueError(f"swd_quantile_cost_bwd: perm must be contiguous int32{tuple(side.shape)} (got {t.dtype}{tuple(t.shape)})")
    gu = torch.empty_like(u) if need_u else None
    gv = torch.empty_like(v) if need_v else None
    call("mf_swd_quantile_cost_bwd", ptr(u), u.shape[1], ptr(perm_u), ptr(v), v.shape[1], ptr(perm_v), P, float(p), ptr(wpp),
         ptr(gdist), ptr(gu), ptr(gv), stream_ptr(u))
    return gu, gv


def swd_project_bwd(g: torch.Tensor, directions: torch.Tensor, out: Optional[torch.Tensor] = None,
                    accumulate: bool = False) -> torch.Tensor:
    """gx[N, d] (+)= g[P, N].T @ directions[d, P].T: the adjoint of swd_project with respect to the points."""
    g, directions = _f32c(g), _f32c(directions)
    if g.dim() != 2 or directions.dim() != 2 or directions.shape[1] != g.shape[0]:
        raise ValueError(f"swd_project_bwd: g[P, N] and directions[d, P] expected (got {tuple(g.shape)}, {tuple(directions.shape)})")
    P, n = g.shape
    d = directions.shape[0]
    if out is None:
        if accumulate:
            raise ValueError("swd_project_bwd: accumulate needs the buffer to add onto")
        out = torch.empty(n, d, dtype=_F32, device=g.device)
    elif out.dtype != _F32 or tuple(out.shape) != (n, d) or not out.is_contiguous():
        raise ValueError(f"swd_project_bwd: out[{n}, {d}] contiguous float32 expected (got {out.dtype}{tuple(out.shape)})")
    call("mf_swd_project_bwd", ptr(g), n, d, ptr(directions), P, ptr(out), int(bool(accumulate)), stream_ptr(g))
    return out


class SlicedWassersteinFn(torch.autograd.Function):
    """dist = sliced_wasserstein(x1, x2, directions, p), differentiable in x1 and x2 (the directions are constants).

    Forward: projections, a pair sort (keys with their positions) for each side that needs a gradient and the keys-only sort
    for the other, the quantile cost.  Equal sizes with both gradients wanted: one [2P, N] buffer, one launch sequence.
    Backward: the closed-form adjoint of the cost stored straight into unsorted order, then the back-projection; no atomics,
    so two backward passes give the same bits.  Identical clouds give zero gradients (include/mentflow_hip.h)."""

    @staticmethod
    def forward(ctx, x1, x2, directions, p, _tile_log2=0):
        x1, x2, directions = _f32c(x1.detach()), _f32c(x2.detach()), _f32c(directions.detach())
        P = directions.shape[1]
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        perm1 = perm2 = None
        if x1.shape[0] == x2.shape[0] and need1 == need2:
            u = torch.empty(2 * P, x1.shape[0], dtype=_F32, device=x1.device)
            swd_project(x1, directions, out=u[:P])
            swd_project(x2, directions, out=u[P:])
            if need1:
                perm = segmented_sort_pairs(u, out=u, _tile_log2=_tile_log2)[1]
                perm1, perm2 = perm[:P], perm[P:]
            else:
                segmented_sort(u, out=u, _tile_log2=_tile_log2)
            u1, u2 = u[:P], u[P:]
        else:
            u1 = swd_project(x1, directions)
            u2 = swd_project(x2, directions)
            if need1:
                perm1 = segmented_sort_pairs(u1, out=u1, _tile_log2=_tile_log2)[1]
            else:
                segmented_sort(u1, out=u1, _tile_log2=_tile_log2)
            if need2:
                perm2 = segmented_sort_pairs(u2, out=u2, _tile_log2=_tile_log2)[1]
            else:
                segmented_sort(u2, out=u2, _tile_log2=_tile_log2)
        wpp, dist = swd_quantile_cost(u1, u2, p)
        ctx.p = float(p)
        ctx.saved = (u1, u2, perm1, perm2, wpp, directions)          # made here, seen by nobody else: no version checks needed
        return dist

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gdist):
        u1, u2, perm1, perm2, wpp, directions = ctx.saved
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gu1, gu2 = swd_quantile_cost_bwd(u1, u2, wpp, gdist, ctx.p, perm_u=perm1, perm_v=perm2, need_u=need1, need_v=need2)
        gx1 = swd_project_bwd(gu1, directions) if need1 else None
        gx2 = swd_project_bwd(gu2, directions) if need2 else None
        return gx1, gx2, None, None, None
