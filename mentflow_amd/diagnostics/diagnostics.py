"""Histogram diagnostics — mirrors mentflow/diagnostics/diagnostics.py:18-201 on the gfx950 kernels.

``Histogram1D`` / ``Histogram2D`` keep the reference's constructor kwargs, buffers (``edges``, ``coords``,
``resolution``, ``bandwidth``; ``edges_x`` ...) and the externally toggled attributes ``kde`` / ``noise``
(experiments/setup.py:52-60).  ``forward(u)`` evaluates ONE projection; ``simulate.forward`` batches all the
projections of a measurement set into a single fused kernel launch (``Histogram*.batched``).
"""
from __future__ import annotations

import logging
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import torch
from torch.utils.checkpoint import checkpoint

from .. import ops
from ..utils import coords_from_edges

log = logging.getLogger("mentflow_amd.diagnostics")

# An axis is UNIFORM when every bin centre lies within UNIFORM_TOL bin widths of the straight line through its first and
# last centres (fp64).  Why 2e-3 bin widths:
# - it is the size of fp32 rounding: an fp32 linspace stores its edges to half an ulp, 2^-24 |c| / delta bin widths (0 for
#   64 bins on [997, 1003], whose step is a binary fraction; 6.7e-4 for 85 bins on [996.7, 1003.1]); the reference itself
#   forms (u - c_k) / sigma in fp32 with that error, so the tolerance admits grids up to |c| / delta ~ 3e4.
# - within it the kernels stay at that accuracy (kde.hip): the centre weight and its two neighbours are read from the table;
#   the factorised tail |j| >= 2 puts bin kc + j at c_kc + j (c1 - c0), off by <= (2 j + 2) e bin widths (c1 - c0 is off
#   the line's step by <= 2 e); the centre bin rint((u - c0) / (c1 - c0)) may drift by a few hundredths of a bin across
#   the grid, which only moves the window by one bin for u near a midpoint, where it still reaches R + 1/2 - drift bins
#   (ops.kde_radius truncates at ~9 sigma).
# - a graded grid sits whole bins off its line (the two probes of tests/test_kde_launch_paths.py: 8.3 and 1.2) and
#   is evaluated densely by raw_sums, as marginal_pdf / joint_pdf do.
UNIFORM_TOL = 2.0e-3


def is_uniform_axis(edges: torch.Tensor, tol: float = UNIFORM_TOL) -> bool:
    c = coords_from_edges(edges.detach().to("cpu", torch.float64))
    if c.numel() < 2:
        return True
    step = (c[-1] - c[0]) / (c.numel() - 1)
    if not float(step) > 0.0:
        return False
    line = c[0] + step * torch.arange(c.numel(), dtype=torch.float64)
    return float((c - line).abs().max() / step) <= tol


# particles x projections x bins per dense chunk (16 M floats: 64 MiB per kernel matrix)
_DENSE_CHUNK_ELEMS = 1 << 24


def _gauss(u: torch.Tensor, c: torch.Tensor, sigma: float) -> torch.Tensor:
    """[n, P, B] = exp(-((u[n, P] - c[B]) / sigma)^2 / 2)   (histogram.py:37-38)."""
    return torch.exp(-0.5 * ((u[:, :, None] - c[None, None, :]) / sigma) ** 2)


def _dense_chunk_1d(x, V, c, sigma):
    return _gauss(x @ V.T, c, sigma).sum(0)


def _dense_chunk_2d(x, V0, V1, cx, cy, sx, sy):
    return torch.einsum("npa,npb->pab", _gauss(x @ V0.T, cx, sx), _gauss(x @ V1.T, cy, sy))


def _dense_chunk_1d_w(x, w, V, c, sigma):
    return (_gauss(x @ V.T, c, sigma) * w[:, None, None]).sum(0)


def _dense_chunk_2d_w(x, w, V0, V1, cx, cy, sx, sy):
    return torch.einsum("n,npa,npb->pab", w, _gauss(x @ V0.T, cx, sx), _gauss(x @ V1.T, cy, sy))


def _dense_sums(fn, x: torch.Tensor, per_particle: int, *args, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sum over particle chunks of fn(x_chunk, *args): each chunk is recomputed in the backward (checkpoint), so neither
    pass holds more than one chunk's kernel matrix.  With weights, fn(x_chunk, w_chunk, *args)."""
    chunk = max(1, _DENSE_CHUNK_ELEMS // max(1, per_particle))
    total = None
    for a in range(0, x.shape[0], chunk):
        xc = x[a:a + chunk]
        head = (xc,) if weights is None else (xc, weights[a:a + chunk])
        grad = any(t.requires_grad for t in head)
        part = checkpoint(fn, *head, *args, use_reentrant=False) if grad else fn(*head, *args)
        total = part if total is None else total + part
    return total


def weight_total(weights: torch.Tensor) -> torch.Tensor:
    """W = the sum of the valid weights as a device scalar (1 where there is none: the sums are all zero then)."""
    W = ops.valid_weights(weights).sum()
    return torch.where(W > 0, W, torch.ones_like(W))


class Diagnostic(torch.nn.Module):
    def __init__(self, device: torch.device = None, seed: int = None, ndim: int = None) -> None:
        super().__init__()
        self.device = device
        self.seed = seed
        self.ndim = ndim

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError


class Histogram(Diagnostic):
    def __init__(self, noise: bool = False, noise_scale: float = 0.0, noise_type: str = "gaussian", **kws) -> None:
        super().__init__(**kws)
        self.noise = noise
        self.noise_scale = noise_scale
        self.noise_type = noise_type

    def set_noise(self, setting: bool) -> None:
        self.noise = setting

    def _apply_noise(self, hist: torch.Tensor) -> torch.Tensor:
        """diagnostics.py:53-67 (multiplicative measurement noise; off during training)."""
        if self.noise and self.noise_scale > 0.0:
            rng = torch.Generator(device=hist.device)
            if self.seed is not None:
                rng.manual_seed(self.seed)
            if self.noise_type == "uniform":
                frac = torch.rand(hist.shape[0], generator=rng, device=hist.device) * 2.0 * self.noise_scale
            elif self.noise_type == "gaussian":
                frac = torch.randn(hist.shape[0], generator=rng, device=hist.device) * self.noise_scale
            else:
                frac = torch.zeros(hist.shape, device=hist.device)
            hist = torch.clamp(hist * (1.0 + frac), 0.0, None)
        return hist

    # rows of a (d x d) transport matrix consumed by this diagnostic: list of [d] vectors
    def projection_rows(self, matrix: torch.Tensor) -> List[torch.Tensor]:
        raise NotImplementedError

    # A histogram is a SUM over particles followed by a normalisation: raw_sums(x, rows) are the per-projection sums of the
    # particles at hand (kernel sums for kde=True, bin counts otherwise), from_sums(S, n) finishes [P, bins...] histograms from
    # sums over n particles.  batched = from_sums(raw_sums); a data-parallel run all-reduces the sums in between
    # (MENTFlow.loss, simulate.raw_sums).
    # weights [n] (optional, everywhere): one weight per particle; the sums become weighted sums and n is replaced by W, the
    # sum of the valid weights (finite and positive; any other weight counts as 0).  Differentiable in the weights for kde=True.
    def raw_sums(self, x: torch.Tensor, rows: List[torch.Tensor], weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        raise NotImplementedError

    def from_sums(self, S: torch.Tensor, n_total: int, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        raise NotImplementedError

    uniform = True              # every axis on a uniform grid: the KDE kernels apply (set by the subclasses)

    def _log_dense(self) -> None:
        if not getattr(self, "_dense_logged", False):
            self._dense_logged = True
            log.info("%s: non-uniform bin edges, KDE sums evaluated densely in torch (the KDE kernels need a uniform grid)",
                     type(self).__name__)

    def identity_rows(self, x: torch.Tensor) -> List[torch.Tensor]:
        eye = torch.eye(x.shape[1], dtype=x.dtype, device=x.device)
        return [r[None, :] for r in self.projection_rows(eye)]

    def batched(self, x: torch.Tensor, rows: List[torch.Tensor], weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """All P projections in one launch: [P, bins...] normalised histograms (kde) or densities (hard bins)."""
        if weights is None:
            return self.from_sums(self.raw_sums(x, rows), x.shape[0])
        return self.from_sums(self.raw_sums(x, rows, weights), x.shape[0], weights)

    def forward(self, x: torch.Tensor, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._apply_noise(self.batched(x, self.identity_rows(x), weights)[0])


class Histogram1D(Histogram):
    """diagnostics.py:71-131."""

    def __init__(self, edges: torch.Tensor, bandwidth: Optional[float] = None, axis: int = 0,
                 direction: torch.Tensor = None, kde: bool = True, **kws) -> None:
        super().__init__(**kws)
        self.axis = axis
        self.kde = kde
        self.ndim = 1
        self.direction = direction
        if self.direction is not None:
            self.direction = self.direction / torch.norm(self.direction)
        if bandwidth is None:
            bandwidth = 0.5
        self.bandwidth_bins = float(bandwidth)
        self.register_buffer("edges", edges)
        self.register_buffer("coords", coords_from_edges(self.edges))
        self.register_buffer("resolution", edges[1] - edges[0])
        self.register_buffer("bandwidth", bandwidth * self.resolution)
        # host copies of the two scalars every launch needs (read once here: no device->host sync per call, and the
        # step stays capturable into a hipGraph)
        self.resolution_value = float(self.resolution)
        self.bandwidth_value = float(self.bandwidth)
        # non-uniform edges: dense KDE sums, normalised with coords[1] - coords[0] as marginal_pdf does (histogram.py:40)
        self.uniform = is_uniform_axis(edges)
        self.cell_value = self.resolution_value if self.uniform else float(self.coords[1] - self.coords[0])

    def project(self, x: torch.Tensor) -> torch.Tensor:
        """diagnostics.py:116-122: x[:, axis], or x . direction."""
        if self.direction is None:
            return x[:, self.axis]
        return torch.sum(x * self.direction.to(x), dim=1)

    def projection_rows(self, matrix: torch.Tensor) -> List[torch.Tensor]:
        """u[:, axis] = x . matrix[axis]  (or  (x @ M.T) . direction = x . (direction @ M))."""
        if self.direction is None:
            return [matrix[self.axis]]
        return [self.direction.to(matrix) @ matrix]

    def raw_sums(self, x: torch.Tensor, rows: List[torch.Tensor], weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        V = rows[0].to(torch.float32).contiguous()
        if self.kde and not self.uniform:
            self._log_dense()
            if weights is not None:
                return _dense_sums(_dense_chunk_1d_w, x, V.shape[0] * self.coords.numel(), V.to(x), self.coords.to(x),
                                   self.bandwidth_value, weights=ops.valid_weights(weights).to(x))
            return _dense_sums(_dense_chunk_1d, x, V.shape[0] * self.coords.numel(), V.to(x), self.coords.to(x),
                               self.bandwidth_value)
        if self.kde and weights is not None:
            return ops.ProjWKde1dFn.apply(x, weights, V, self.coords, self.bandwidth_value, ops.kde_radius(self.bandwidth_bins))
        if self.kde:
            return ops.ProjKde1dFn.apply(x, V, self.coords, self.bandwidth_value, ops.kde_radius(self.bandwidth_bins))
        if weights is not None:
            return ops.proj_whist_sums_1d(x.detach(), weights.detach(), V, self.edges)
        return ops.proj_hist_counts_1d(x.detach(), V, self.edges).to(torch.float32)

    def from_sums(self, S: torch.Tensor, n_total: int, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.kde and weights is not None:            # (S / W) / (delta * sum_k S_k / W + 1e-10): n replaced by W
            ghat, _ = ops.HistNormDiscFn.apply(S / weight_total(weights), None, True, 1.0, self.cell_value, 1.0e-10, 0, 0.0, 1.0)
            return ghat
        if self.kde:
            ghat, _ = ops.HistNormDiscFn.apply(S, None, True, 1.0 / n_total, self.cell_value, 1.0e-10, 0, 0.0, 1.0)
            return ghat
        widths = (self.edges[1:] - self.edges[:-1])[None, :]
        return S / S.sum(dim=1, keepdim=True) / widths                    # torch.histogram(density=True)


class Histogram2D(Histogram):
    """diagnostics.py:134-201."""

    def __init__(self, axis: Iterable[int], edges: Iterable[torch.Tensor], bandwidth: Iterable[Optional[float]] = (None, None),
                 kde: bool = True, **kws) -> None:
        super().__init__(**kws)
        self.axis = tuple(axis)
        self.kde = kde
        self.ndim = 2
        bx, by = bandwidth
        bx = 0.5 if bx is None else bx
        by = 0.5 if by is None else by
        self.bandwidth_bins = (float(bx), float(by))
        self.register_buffer("edges_x", edges[0])
        self.register_buffer("edges_y", edges[1])
        self.register_buffer("coords_x", coords_from_edges(self.edges_x))
        self.register_buffer("coords_y", coords_from_edges(self.edges_y))
        self.register_buffer("resolution_x", self.edges_x[1] - self.edges_x[0])
        self.register_buffer("resolution_y", self.edges_y[1] - self.edges_y[0])
        self.register_buffer("bandwidth_x", bx * self.resolution_x)
        self.register_buffer("bandwidth_y", by * self.resolution_y)
        self.resolution_values = (float(self.resolution_x), float(self.resolution_y))
        self.bandwidth_values = (float(self.bandwidth_x), float(self.bandwidth_y))
        # one non-uniform axis makes the whole image dense; joint_pdf normalises with the coords steps (histogram.py:70)
        self.uniform = is_uniform_axis(self.edges_x) and is_uniform_axis(self.edges_y)
        self.cell_value = (self.resolution_values[0] * self.resolution_values[1] if self.uniform else
                           float(self.coords_x[1] - self.coords_x[0]) * float(self.coords_y[1] - self.coords_y[0]))

    @property
    def edges(self) -> Tuple[torch.Tensor, torch.Tensor]:
        return (self.edges_x, self.edges_y)

    @property
    def shape(self) -> Tuple[int, int]:
        """(Bx, By): the shape of one projection (used by MENT's integrate mode)."""
        return (self.coords_x.numel(), self.coords_y.numel())

    def project(self, x: torch.Tensor) -> torch.Tensor:
        """diagnostics.py:179-180."""
        return x[:, self.axis]

    def projection_rows(self, matrix: torch.Tensor) -> List[torch.Tensor]:
        return [matrix[self.axis[0]], matrix[self.axis[1]]]

    def raw_sums(self, x: torch.Tensor, rows: List[torch.Tensor], weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        V0 = rows[0].to(torch.float32).contiguous()
        V1 = rows[1].to(torch.float32).contiguous()
        if self.kde and not self.uniform:
            self._log_dense()
            if weights is not None:
                return _dense_sums(_dense_chunk_2d_w, x, V0.shape[0] * (self.coords_x.numel() + self.coords_y.numel()
                                                                        + self.coords_x.numel() * self.coords_y.numel()),
                                   V0.to(x), V1.to(x), self.coords_x.to(x), self.coords_y.to(x), *self.bandwidth_values,
                                   weights=ops.valid_weights(weights).to(x))
            return _dense_sums(_dense_chunk_2d, x, V0.shape[0] * (self.coords_x.numel() + self.coords_y.numel()
                                                                  + self.coords_x.numel() * self.coords_y.numel()),
                               V0.to(x), V1.to(x), self.coords_x.to(x), self.coords_y.to(x), *self.bandwidth_values)
        if self.kde and weights is not None:
            return ops.ProjWKde2dFn.apply(x, weights, V0, V1, self.coords_x, self.coords_y, self.bandwidth_values[0],
                                          self.bandwidth_values[1], ops.kde_radius(self.bandwidth_bins[0]),
                                          ops.kde_radius(self.bandwidth_bins[1]))
        if self.kde:
            return ops.ProjKde2dFn.apply(x, V0, V1, self.coords_x, self.coords_y, self.bandwidth_values[0],
                                         self.bandwidth_values[1], ops.kde_radius(self.bandwidth_bins[0]),
                                         ops.kde_radius(self.bandwidth_bins[1]))
        if weights is not None:
            return ops.proj_whist_sums_2d(x.detach(), weights.detach(), V0, V1, self.edges_x, self.edges_y)
        return ops.proj_hist_counts_2d(x.detach(), V0, V1, self.edges_x, self.edges_y).to(torch.float32)

    def from_sums(self, S: torch.Tensor, n_total: int, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        # (the 2-D normalisation S / (dx dy sum S + 1e-10) never divides by n, so the weights change nothing here)
        if self.kde:
            P, Bx, By = S.shape
            ghat, _ = ops.HistNormDiscFn.apply(S.reshape(P, Bx * By), None, True, 1.0,
                                               self.cell_value, 1.0e-10, 0, 0.0, 1.0)
            return ghat.view(P, Bx, By)
        area = (self.edges_x[1:] - self.edges_x[:-1])[:, None] * (self.edges_y[1:] - self.edges_y[:-1])[None, :]
        return S / S.sum(dim=(1, 2), keepdim=True) / area[None]             # np.histogramdd(density=True)


class Projection(Diagnostic):
    """Projects points onto axis (no density estimation) — diagnostics.py:204-211."""

    def __init__(self, axis: Union[int, Tuple[int]], **kws) -> None:
        super().__init__(**kws)
        self.axis = axis

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x[:, self.axis]
