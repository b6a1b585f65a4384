"""Entropy estimators — mirrors mentflow/entropy.py:8-62."""
from typing import Any, Optional

import torch

from . import ops
from .prior import Gaussian


class EntropyEstimator(torch.nn.Module):
    """Negative-entropy estimate H from samples and / or their log-density (interface of entropy.py:8-15); `prior`
    turns it into the relative entropy against that prior."""

    def __init__(self, prior: Any = None) -> None:
        super().__init__()
        self.prior = prior

    def forward(self, x: torch.Tensor, log_prob: Optional[torch.Tensor] = None) -> torch.Tensor:
        raise NotImplementedError(type(self).__name__)


class EmptyEntropyEstimator(EntropyEstimator):
    """No entropy term (entropy.py:18-24): the python float 0.0, whatever the inputs."""

    def forward(self, x: torch.Tensor, log_prob: Optional[torch.Tensor] = None) -> float:
        return 0.0


class CovarianceEntropyEstimator(EntropyEstimator):
    """H = -3 ln(2 pi e) - ln(sqrt(det cov(x)) + pad)  (entropy.py:27-38): the negative entropy of the Gaussian with the
    samples' covariance.  The constant is the reference's as it stands, -3 ln(2 pi e) for EVERY dimension (it is the 6-D
    value -(d/2) ln(2 pi e)); it is reproduced, not corrected, and shifts H only.  Moments, determinant, inverse and the
    adjoint run on the GPU without a host synchronisation (ops.CovEntropyFn)."""

    def __init__(self, prior: Any = None, pad: float = 1.00e-12) -> None:
        if prior is not None:
            raise ValueError("This class cannot estimate relative entropy (prior != None).")
        super().__init__(prior=prior)
        self.pad = pad

    def forward(self, x: torch.Tensor, log_prob: Optional[torch.Tensor] = None) -> torch.Tensor:
        return ops.cov_entropy(x, self.pad)


class KNNEntropyEstimator(EntropyEstimator):
    """Kozachenko-Leonenko estimate from the k-th nearest other point of the batch (the reference declares the class,
    entropy.py:41-50, and leaves forward unimplemented):

        H = -[psi(N) - psi(k) + ln c_d + (d / N) sum_i ln rho_k(i)],   c_d = pi^(d/2) / Gamma(d/2 + 1)

    differentiable in x.  1 <= k <= 16, N > k, 1 <= d <= 16, float32 on the GPU; all-pairs search without an N x N buffer
    (ops.KnnEntropyFn, DESIGN.md §6d for the tie-break, floor and non-finite rules)."""

    def __init__(self, prior: Any = None, k: int = 5) -> None:
        if prior is not None:
            raise ValueError("This class cannot estimate relative entropy (prior != None).")
        super().__init__(prior=prior)
        self.k = k

    def forward(self, x: torch.Tensor, log_prob: Optional[torch.Tensor] = None) -> torch.Tensor:
        return ops.knn_entropy(x, self.k)[0]


class MonteCarloEntropyEstimator(EntropyEstimator):
    """H = mean(log_prob) - mean(prior.log_prob(x))  (entropy.py:53-62), both means from one reduction kernel.

    ``sums`` reduces the particles at hand and ``from_sums`` finishes the estimate from already reduced sums — used by
    ``MENTFlow.loss`` so that a data-parallel run can sum across GPUs in between.  For ``prior.Gaussian`` (or no prior) the
    sums are [sum log_prob, sum |x|^2], the prior's sufficient statistic.  Any other prior with a differentiable
    ``log_prob(x)`` (``prior.MENTPrior``, ``ment.UniformPrior``) adds a third entry, sum prior.log_prob(x), from the same
    fixed-order fp64 reduction and its adjoint."""

    def sums(self, x: torch.Tensor, log_prob: torch.Tensor) -> torch.Tensor:
        out = ops.EntropySumsFn.apply(x, log_prob)
        if self.prior is None or isinstance(self.prior, Gaussian):
            return out
        return torch.cat([out, ops.EntropySumsFn.apply(x, self.prior.log_prob(x))[:1]])

    def from_sums(self, sums: torch.Tensor, n_total: int) -> torch.Tensor:
        H = sums[0] / n_total
        if sums.numel() == 3:
            return H - sums[2] / n_total
        if self.prior is not None:
            if not isinstance(self.prior, Gaussian):
                raise NotImplementedError(f"prior {type(self.prior).__name__}: its sum is the third entry of sums(), "
                                          "which these two entries lack")
            H = H - (-0.5 * sums[1] / (n_total * self.prior.scale ** 2) + self.prior.log_norm())
        return H

    def forward(self, x: torch.Tensor, log_prob: torch.Tensor) -> torch.Tensor:
        return self.from_sums(self.sums(x, log_prob), x.shape[0])
