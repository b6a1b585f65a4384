"""Sampling from gridded densities — mirrors mentflow/sample.py:18-113 on the gfx950 kernels (mentflow_amd/csrc/ment.hip).

``sample_hist`` and ``GridSampler`` draw a cell with probability proportional to ``hist + 1e-15`` (sample.py:28) and a point
uniformly inside it, as the reference does, but by inverse CDF on the device: fp64 per-block sums of the weights, a
fixed-order prefix over the blocks, then a fixed-order scan inside the chosen block.  The uniforms come from ``torch.rand``
on the device (1 + 2 ndim per sample), so ``torch.manual_seed`` fixes a run, and there is no limit on the number of cells
(``torch.multinomial``, which the reference uses, refuses more than 2^24 categories).  ``GridSampler`` called with
``MENT.prob`` itself (not ``log_prob``, not a subclass's override) of a :class:`mentflow_amd.ment.MENT` whose slots all run
through the kernels evaluates the density on the implicit grid (the points are never stored) in the same launch that forms
the block sums.

Quirk kept from the reference: with ``noise`` truthy every axis also gets ``0.5 U(-delta, delta)``, whatever the value of
``noise`` (sample.py:58-60).
"""
from __future__ import annotations

from typing import Callable, List, Tuple

import torch

from . import ops
from .utils import coords_from_edges, get_grid_points


def random_uniform(lb: float, ub: float, size: int, device=None) -> torch.Tensor:
    return lb + (ub - lb) * torch.rand(size, device=device)


def random_choice(items: torch.Tensor, size: int, p: torch.Tensor):
    return items[p.multinomial(num_samples=size, replacement=True)]


def sample_hist_bins(hist: torch.Tensor, size: int) -> torch.Tensor:
    """Flat indices of `size` cells drawn with probability (hist + 1e-15) / sum (sample.py:26-30)."""
    pdf = torch.ravel(hist) + 1.00e-15
    idx = torch.squeeze(torch.nonzero(pdf))
    return random_choice(idx, size, p=(pdf / torch.sum(pdf)))


def _edges_list(edges, ndim: int) -> List[torch.Tensor]:
    if ndim == 1 and torch.is_tensor(edges):
        return [edges]
    return list(edges)


def sample_hist(hist: torch.Tensor, edges: List[torch.Tensor], size: int, noise: float = 0.0,
                device: torch.device = None) -> torch.Tensor:
    """sample.py:33-56: `size` points from the histogram `hist` (any number of axes up to 8) with bin edges `edges`
    (a tensor for 1-D); the result is squeezed like the reference's ([size] for 1-D)."""
    edges = _edges_list(edges, hist.ndim)
    hist = hist.to(torch.float32).contiguous()
    sums = ops.ment_block_sums(hist)
    x = ops.ment_sample(hist, list(hist.shape), sums, edges, int(size), bool(noise))
    if device is not None:
        x = x.to(device)
    return torch.squeeze(x)


class GridSampler:
    """sample.py:59-113."""

    def __init__(self, limits: List[Tuple[float]], shape: Tuple[int], noise: float = 0.0, device: torch.device = None,
                 store: bool = True) -> None:
        self.device = device
        self.shape = shape
        self.limits = limits
        self.ndim = len(limits)
        self.noise = noise
        self.store = store
        self.edges = [torch.linspace(self.limits[axis][0], self.limits[axis][1], self.shape[axis] + 1)
                      for axis in range(self.ndim)]
        self.coords = [coords_from_edges(e) for e in self.edges]
        self.points = None

    def send(self, x: torch.Tensor) -> torch.Tensor:
        return x.type(torch.float32).to(self.device)

    def get_grid_points(self) -> torch.Tensor:
        if self.points is not None:
            return self.points
        points = self.send(get_grid_points(*self.coords))
        if self.store:
            self.points = points
        return points

    def __call__(self, prob_func: Callable, size: int) -> torch.Tensor:
        from .ment import MENT
        # the implicit-grid kernel computes exactly MENT.prob: taken for that method only (not for log_prob, nor for a
        # subclass that overrides prob), else the density handed in is evaluated on the stored points
        owner = getattr(prob_func, "__self__", None)
        fused = None
        if isinstance(owner, MENT) and getattr(prob_func, "__func__", None) is MENT.prob:
            fused = owner.prob_on_grid(self.coords)
        if fused is None:                                      # any density: evaluate it on the stored grid points
            prob = torch.reshape(prob_func(self.get_grid_points()), tuple(self.shape))
            return self.send(sample_hist(prob, self.edges, size=size, noise=self.noise, device=self.device))
        prob, sums = fused                                     # MENT.prob on the implicit grid, block sums included
        x = ops.ment_sample(prob, [int(s) for s in self.shape], sums, self.edges, int(size), bool(self.noise))
        return self.send(torch.squeeze(x))

    def to(self, device):
        self.device = device
        self.edges = [self.send(e) for e in self.edges]
        self.coords = [self.send(c) for c in self.coords]
        if self.points is not None:
            self.points = self.send(self.points)
        return self
