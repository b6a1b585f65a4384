"""Discrepancy functions and the sliced Wasserstein distance — mirrors mentflow/loss.py:7-42.

The reference hands the sorted-quantile cost of each projection to POT's CPU solver (``ot.lp.wasserstein_1d``); here the
projections, a segmented key sort and the quantile integral are HIP kernels (mentflow_amd/csrc/swd.hip), and the
distance comes back as a 0-dim device tensor without a device-to-host copy.  SlicedWassersteindDistance is the evaluation
metric of the reference's interface (no graph); SlicedWassersteinLoss is the same value with a backward pass in HIP."""
from typing import Optional

import torch

from . import ops


def _discrepancy(pred: torch.Tensor, targ: torch.Tensor, kind: str, pad: float, batch_div: float) -> torch.Tensor:
    S = pred.reshape(1, -1)
    _, D = ops.HistNormDiscFn.apply(S, targ.reshape(1, -1), False, 1.0, 1.0, 0.0, ops.DISCREPANCY_KINDS[kind], pad,
                                    float(batch_div))
    return D[0]


def mean_absolute_error(pred: torch.Tensor, targ: torch.Tensor) -> torch.Tensor:
    return _discrepancy(pred, targ, "mae", 0.0, pred.numel())


def mean_square_error(pred: torch.Tensor, targ: torch.Tensor) -> torch.Tensor:
    return _discrepancy(pred, targ, "mse", 0.0, pred.numel())


def kl_divergence(pred: torch.Tensor, targ: torch.Tensor, pad=1.00e-12) -> torch.Tensor:
    """F.kl_div(log(pred + pad), targ, reduction="batchmean"): sum / pred.shape[0]  (loss.py:15-17)."""
    return _discrepancy(pred, targ, "kld", pad, pred.shape[0])


kl_divergence.kind = "kld"
mean_absolute_error.kind = "mae"
mean_square_error.kind = "mse"


class SlicedWassersteindDistance:
    """Sliced Wasserstein Distance (SWD), loss.py:20-42 (the class name keeps the reference's spelling).

    ``(mean over n_projections random unit directions of W_p^p(x1 . dir, x2 . dir))^(1/p)`` for the uniform-weight empirical
    measures of x1[N1, d] and x2[N2, d] (N1 != N2 allowed, d <= 8).  The directions are drawn as the reference draws them
    (``torch.randn(d, n_projections, device=...)``, columns normalised), so ``torch.manual_seed`` fixes the value; the
    keyword-only ``directions[d, P]`` replaces the draw (same slices for two models, tests).  A NaN in an input gives NaN."""

    def __init__(self, n_projections: int = 50, p: int = 2, device=None) -> None:
        self.n_projections = n_projections
        self.p = p
        self.device = device

    @staticmethod
    def _check_clouds(x1: torch.Tensor, x2: torch.Tensor) -> None:
        if x1.dim() != 2 or x2.dim() != 2:
            raise ValueError(f"x1 and x2 must be [N, d] point clouds (got {tuple(x1.shape)}, {tuple(x2.shape)})")
        if x1.shape[1] != x2.shape[1]:
            raise ValueError(f"x1.shape[1]={x1.shape} != x2.shape[1]={x2.shape})")

    def _directions(self, x1: torch.Tensor, x2: torch.Tensor, directions: Optional[torch.Tensor]) -> torch.Tensor:
        """The remaining checks, and the directions[d, P] of this call (drawn unless given) as fp32 on x1's device."""
        d = x1.shape[1]
        if x1.shape[0] == 0 or x2.shape[0] == 0:
            raise ValueError(f"x1 and x2 need at least one point each (got {x1.shape[0]}, {x2.shape[0]})")
        if d < 1 or d > 8:
            raise ValueError(f"the projection kernels support 1 <= d <= 8 features (got {d})")
        if not float(self.p) >= 1.0:
            raise ValueError(f"p must be >= 1 (got {self.p})")
        if directions is None:
            if int(self.n_projections) < 1:
                raise ValueError(f"n_projections must be positive (got {self.n_projections})")
            directions = torch.randn(d, self.n_projections, device=self.device)
            directions = directions / torch.sqrt(torch.sum(directions**2, 0, keepdims=True))
        elif directions.dim() != 2 or directions.shape[0] != d or directions.shape[1] < 1:
            raise ValueError(f"directions must be [d={d}, P >= 1] (got {tuple(directions.shape)})")
        if directions.shape[1] * max(x1.shape[0], x2.shape[0]) >= 2**31:
            raise ValueError(f"{directions.shape[1]} projections of {max(x1.shape[0], x2.shape[0])} points reach 2^31 keys")
        return directions.detach().to(x1.device, torch.float32)

    def __call__(self, x1: torch.Tensor, x2: torch.Tensor, *, directions: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check_clouds(x1, x2)
        if torch.is_grad_enabled() and (x1.requires_grad or x2.requires_grad):
            raise NotImplementedError("SlicedWassersteinDistance is an evaluation metric without a backward pass: call it under "
                                      "torch.no_grad() or on detached samples")
        directions = self._directions(x1, x2, directions)
        return ops.sliced_wasserstein(x1.detach(), x2.detach(), directions, float(self.p))


SlicedWassersteinDistance = SlicedWassersteindDistance


class SlicedWassersteinLoss(SlicedWassersteindDistance):
    """The same distance as a training loss: differentiable in x1 and x2 (ops.SlicedWassersteinFn; the adjoint is closed form,
    HIP kernels, no atomics, reproducible bit for bit).  Same constructor, call signature, direction draw and
    checks as SlicedWassersteindDistance; the directions are constants.  With grad enabled and an input that requires grad the
    result is attached to the graph, otherwise it is exactly what the base class returns.  Identical clouds (distance 0) give
    zero gradients, where autograd of the composed formula gives NaN for p > 1."""

    def __call__(self, x1: torch.Tensor, x2: torch.Tensor, *, directions: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check_clouds(x1, x2)
        if not (torch.is_grad_enabled() and (x1.requires_grad or x2.requires_grad)):
            return super().__call__(x1, x2, directions=directions)
        directions = self._directions(x1, x2, directions)
        return ops.SlicedWassersteinFn.apply(x1, x2, directions, float(self.p))
