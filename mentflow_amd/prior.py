"""Prior distributions (interface of mentflow/prior.py:4-26)."""
import copy
import math

import torch


class Gaussian:
    """Isotropic Gaussian prior N(0, scale^2 I).  ``log_prob`` is the closed form of
    ``MultivariateNormal(0, scale^2 I).log_prob`` (prior.py:25-26); inside ``MonteCarloEntropyEstimator`` only its
    sufficient statistic sum|x|^2 is needed, which the entropy kernel reduces."""

    def __init__(self, ndim: int = 2, scale: float = 1.0, device=None) -> None:
        self.ndim, self.scale, self.device = int(ndim), float(scale), device

    def to(self, device) -> "Gaussian":
        self.device = device
        return self

    def log_norm(self) -> float:
        """log of the normalisation constant (2 pi scale^2)^(-ndim/2)."""
        return -self.ndim * (math.log(self.scale) + 0.5 * math.log(2.0 * math.pi))

    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        return self.log_norm() - 0.5 * x.square().sum(dim=1) / self.scale ** 2


class MENTPrior:
    """A classical MENT reconstruction (``ment.MENT``: an earlier run with fewer views, other optics, a coarser scan) as the
    prior of ``MonteCarloEntropyEstimator``: ``log_prob(x) = ment.log_density(x, pad)``, differentiable in x on the
    log-density kernel (no counterpart in the reference).

    The density is UNNORMALISED: MENT fixes its Lagrange functions up to the normalisation Z of their product, so the
    relative entropy H comes out offset by the unknown constant log Z, which moves no gradient.  With ``pad > 0`` a point
    outside the support of the reconstruction carries the constant log(pad) with zero gradient (with ``pad = 0``: -inf, which
    makes H infinite as soon as one particle leaves the support).

    Picklable (``MENTFlow.save`` stores the entropy estimator with its prior): the MENT's cached launch plan is dropped and
    rebuilt on first use."""

    def __init__(self, ment, pad: float = 1.0e-12) -> None:
        self.ment, self.pad = ment, float(pad)

    def to(self, device) -> "MENTPrior":
        self.ment.to(device)
        return self

    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        return self.ment.log_density(x, self.pad)

    def __getstate__(self):
        state = dict(self.__dict__)
        ment = copy.copy(self.ment)
        ment._plan = None
        state["ment"] = ment
        return state
