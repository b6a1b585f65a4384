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

``MetropolisHastingsSampler`` (no counterpart in the reference) draws particles from many independent random-walk
Metropolis-Hastings chains instead: it needs point evaluations of the density only, so its cost does not grow as res^ndim.
Same call contract as ``GridSampler``; kernel in mentflow_amd/csrc/mcmc.hip.  ``LangevinSampler`` (no counterpart either) pushes
those proposals along the gradient of the log-density and tests acceptance on logarithms (Metropolis-adjusted Langevin; kernel in
mentflow_amd/csrc/mala.hip).  Both derive from ``_ChainSampler``, which holds everything but the transition.
``AnnealedImportanceSampler`` (no counterpart either) walks such Langevin chains along a temperature ladder from a normalised
Gaussian to the MENT density and carries an importance weight per chain: the weights estimate the normaliser of the density
(``MENT.log_normalization``), and the weighted final states, resampled, are draws from it (kernel in mentflow_amd/csrc/ais.hip).
``SequentialMonteCarloSampler`` (no counterpart either) is that sampler with adaptive resampling per island on the way up the
ladder (kernel in mentflow_amd/csrc/smc.hip) and a weighted population kept from call to call, which follows a density that
changes a little by one reweighting step instead of a new ladder.
"""
from __future__ import annotations

import logging
import math
from typing import Callable, List, Optional, Sequence, Tuple, Union

import torch

from . import _lib, ops
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


def _ment_of(prob_func: Callable, required_by: Optional[str] = None):
    """The MENT whose own ``MENT.prob`` (not ``log_prob``, not a subclass's override) `prob_func` is bound to, else None: the one
    density the fused kernels compute.  With `required_by` (a sampler without a generic path) None is refused instead."""
    from .ment import MENT
    owner = getattr(prob_func, "__self__", None)
    if isinstance(owner, MENT) and getattr(prob_func, "__func__", None) is MENT.prob:
        return owner
    if required_by is not None:
        raise NotImplementedError(f"{required_by} takes the bound MENT.prob of a MENT (got "
                                  f"{getattr(prob_func, '__qualname__', prob_func)}): there is no generic path")
    return None


def _per_axis(name: str, ndim: int, value, default: float, what: str) -> List[float]:
    if value is None:
        return [default] * ndim
    if isinstance(value, (int, float)):
        return [float(value)] * ndim
    out = [float(v) for v in value]
    if len(out) != ndim:
        raise ValueError(f"{name}: {what} must be a float or {ndim} per-axis values (got {len(out)})")
    return out


def _check_axes(name: str, ndim: int, step, bad_step: Optional[str] = None) -> Tuple[int, List[float]]:
    """(ndim, step per axis) of a chain sampler, validated.  bad_step: AnnealedImportanceSampler's wording of a refused step."""
    ndim = int(ndim)
    if not 1 <= ndim <= 8:
        raise ValueError(f"{name}: 1 <= ndim <= 8 expected (got {ndim})")
    steps = [float(step)] * ndim if isinstance(step, (int, float)) else [float(v) for v in step]
    if len(steps) != ndim:
        raise ValueError(bad_step or f"{name}: step must be a float or {ndim} per-axis scales (got {len(steps)})")
    return ndim, steps


def _check_drift(name: str, steps: List[float], drift_clip: float, bad_step: Optional[str] = None) -> float:
    """What a Langevin transition needs on top of _check_axes: step > 0 on every axis and drift_clip >= 0, which is returned."""
    if not all(v > 0 for v in steps):
        raise ValueError(bad_step or f"{name}: step > 0 expected on every axis (got {steps})")
    if not float(drift_clip) >= 0.0:
        raise ValueError(f"{name}: drift_clip >= 0 expected (got {drift_clip})")
    return float(drift_clip)


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
        # the implicit-grid kernel computes exactly MENT.prob, else the density handed in is evaluated on the stored points
        owner = _ment_of(prob_func)
        fused = owner.prob_on_grid(self.coords) if owner is not None else None
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


log = logging.getLogger("mentflow_amd.sample")
_NOISE_CHUNK_BYTES = 256 << 20      # noise of one launch of the fused path (generated per chunk, never for the whole run)


class _ChainSampler:
    """What the particle samplers built on many independent Markov chains share: the constructor arguments, the persistent
    chain states, the noise ([steps, ndim + 1, chains]: normal proposal rows and a uniform last row, drawn on the device in chunks
    of _NOISE_CHUNK_BYTES), the bookkeeping of kept states and acceptance, and the call contract of ``GridSampler``.  A subclass
    gives the transition: ``_fused_steps`` (its kernel), ``_generic_steps`` (the same rule in torch ops) and ``_target`` (what the
    generic path evaluates)."""

    _generic_note = ""             # how the generic path differs, for the log line

    def __init__(self, ndim: int, chains: int, step: Union[float, Sequence[float]], burn: int, thin: int,
                 start: Optional[torch.Tensor], start_scale: float, persistent: bool, burn_persistent: Optional[int],
                 device: torch.device) -> None:
        name = type(self).__name__
        self.ndim, self.step = _check_axes(name, ndim, step)
        self.chains = int(chains)
        if self.chains < 1 or int(burn) < 0 or int(thin) < 1:
            raise ValueError(f"{name}: chains >= 1, burn >= 0 and thin >= 1 expected")
        if start is not None and tuple(start.shape) != (self.chains, self.ndim):
            raise ValueError(f"{name}: start[{self.chains}, {self.ndim}] expected (got {tuple(start.shape)})")
        self.burn, self.thin = int(burn), int(thin)
        self.start, self.start_scale = start, float(start_scale)
        self.persistent = bool(persistent)
        self.burn_persistent = self.thin if burn_persistent is None else int(burn_persistent)
        self.device = device
        self.state: Optional[torch.Tensor] = None
        self.acceptance: Optional[torch.Tensor] = None
        self._logged_generic = False

    def reset(self) -> None:
        """Forget the chain states: the next call starts from `start` (or a fresh normal draw) and burns `burn` steps."""
        self.state = None

    def to(self, device):
        self.device = device
        for name in ("start", "state", "acceptance"):
            t = getattr(self, name)
            if t is not None:
                setattr(self, name, t.to(device))
        return self

    # ---------------------------------------------------------------------------------------------------- internals
    def _fused_args(self, prob_func: Callable):
        owner = _ment_of(prob_func)
        if owner is None:
            return None
        if owner.ndim != self.ndim:
            raise ValueError(f"{type(self).__name__}(ndim={self.ndim}) called with the density of a MENT of ndim={owner.ndim}")
        return owner.fused_args()

    def _init_state(self, prob_func: Callable) -> None:
        device = self.device
        if device is None:
            owner = getattr(prob_func, "__self__", None)
            device = owner._device() if hasattr(owner, "_device") else torch.device(_lib.device_type())
        if self.start is not None:
            self.state = self.start.detach().to(device, torch.float32).clone().contiguous()
        else:
            self.state = self.start_scale * torch.randn(self.chains, self.ndim, device=device)

    def _noise(self, steps: int, device) -> torch.Tensor:
        nz = torch.empty(steps, self.ndim + 1, self.chains, device=device)
        nz[:, :self.ndim].normal_()
        nz[:, self.ndim].uniform_()
        return nz

    def _target(self, prob_func: Callable, fused) -> Optional[Callable]:
        """What `_generic_steps` evaluates when `fused` (the kernel's arguments) is None."""
        return prob_func

    def _fused_steps(self, x, args, noise, scale, accepted, t0, keep_from, keep_every, out) -> None:
        raise NotImplementedError

    def _generic_steps(self, target, noise, scale, accepted, t0, keep_from, keep_every, out) -> None:
        raise NotImplementedError

    def run(self, prob_func: Callable, steps: int, noise: Optional[torch.Tensor] = None, keep_from: int = 0,
            keep_every: int = 1) -> torch.Tensor:
        """Advance every chain by `steps` steps and return the states after the steps g >= keep_from with
        (g - keep_from) % keep_every == 0 as [n_keep, chains, ndim].  noise: [steps, ndim + 1, chains] (normal proposal rows,
        a uniform last row), default drawn on the device in chunks."""
        name = type(self).__name__
        steps, keep_from, keep_every = int(steps), int(keep_from), int(keep_every)
        if steps < 0 or keep_from < 0 or keep_every < 1:
            raise ValueError(f"{name}.run: steps, keep_from >= 0 and keep_every >= 1 expected")
        args = self._fused_args(prob_func)
        target = self._target(prob_func, args)
        if self.state is None:
            self._init_state(prob_func)
        x = self.state
        _lib.ptr(x)                                            # the usual refusal of tensors the library does not compute on
        if noise is not None:
            if tuple(noise.shape) != (steps, self.ndim + 1, self.chains):
                raise ValueError(f"{name}.run: noise[{steps}, {self.ndim + 1}, {self.chains}] expected "
                                 f"(got {tuple(noise.shape)})")
            noise = noise.to(x.device, torch.float32).contiguous()
        if args is None and not self._logged_generic:
            self._logged_generic = True
            log.info("%s: %s is not the bound MENT.prob of a fully fused MENT: the generic path runs (the "
                     "same transition rule in torch ops, %s)", name, getattr(prob_func, "__qualname__", prob_func),
                     self._generic_note)
        n_keep = 0 if steps <= keep_from else (steps - 1 - keep_from) // keep_every + 1
        out = torch.empty(n_keep, self.chains, self.ndim, device=x.device) if n_keep else None
        accepted = torch.zeros(self.chains, dtype=torch.int32, device=x.device)
        scale = torch.tensor(self.step, dtype=torch.float32, device=x.device)
        per = max(1, _NOISE_CHUNK_BYTES // (4 * (self.ndim + 1) * self.chains))
        for t0 in range(0, steps, per):
            t1 = min(steps, t0 + per)
            nz = noise[t0:t1] if noise is not None else self._noise(t1 - t0, x.device)
            if args is not None:
                self._fused_steps(x, args, nz, scale, accepted, t0, keep_from, keep_every, out)
            else:
                self._generic_steps(target, nz, scale, accepted, t0, keep_from, keep_every, out)
        self.acceptance = accepted.sum().to(torch.float32) / float(max(1, steps) * self.chains)
        return out if out is not None else torch.empty(0, self.chains, self.ndim, device=x.device)

    def __call__(self, prob_func: Callable, size: int) -> torch.Tensor:
        size = int(size)
        if not self.persistent:
            self.reset()
        burn = self.burn if self.state is None else self.burn_persistent
        rounds = max(1, math.ceil(size / self.chains))
        kept = self.run(prob_func, burn + rounds * self.thin, keep_from=burn + self.thin - 1, keep_every=self.thin)
        return kept.reshape(-1, self.ndim)[:size]


class MetropolisHastingsSampler(_ChainSampler):
    """`chains` independent random-walk Metropolis-Hastings chains on a density given by point evaluations.

    One step of a chain at x with density p: y = x + step * z (z standard normal per axis), p_new = prob(y), u uniform on
    [0, 1); accept iff ``p_new > 0 ? u * p < p_new : (p_new == 0 and p == 0)``.  Inside the support that is the Metropolis rule;
    a chain outside it (p == 0) random-walks until it finds it and never leaves it again; a NaN p_new is rejected.  The noise
    is ``torch.randn`` / ``torch.rand`` on the device, so ``torch.manual_seed`` fixes a run.

    Called with ``MENT.prob`` itself of a MENT whose slots all run through the kernels, the steps run in the fused kernel
    (state and density in registers, one launch per chunk of steps); any other callable (``log_prob`` is NOT a density, a
    subclass's override, a user function) takes the same rule in torch ops with one ``prob_func`` call per step, logged once.

    ``sampler(prob_func, size)`` runs ``burn + ceil(size / chains) * thin`` steps, keeps every ``thin``-th state after the burn-in
    and returns the first ``size`` rows of the kept block (step-major).  With ``persistent`` later calls continue from the stored
    states and burn only ``burn_persistent`` (default ``thin``) steps: between Gauss-Seidel sub-steps the density moves little.
    """

    _generic_note = "one density call per step"

    def __init__(self, ndim: int, chains: int = 65536, step: Union[float, Sequence[float]] = 0.25, burn: int = 200,
                 thin: int = 10, start: Optional[torch.Tensor] = None, start_scale: float = 1.0, persistent: bool = True,
                 burn_persistent: Optional[int] = None, device: torch.device = None) -> None:
        super().__init__(ndim, chains, step, burn, thin, start, start_scale, persistent, burn_persistent, device)

    def _fused_steps(self, x, args, noise, scale, accepted, t0, keep_from, keep_every, out) -> None:
        ops.mcmc_ment_steps(x, args[0], args[1], args[2], args[3], noise, scale, accepted, step_offset=t0,
                            keep_from=keep_from, keep_every=keep_every, out=out)

    def _generic_steps(self, prob_func, noise, scale, accepted, t0, keep_from, keep_every, out) -> None:
        x, d = self.state, self.ndim
        p = prob_func(x)
        for t in range(noise.shape[0]):
            # the kernel's fma(scale, z, x): the fp32 product is exact in fp64, so this differs from it by a double rounding at most
            y = (x.double() + noise[t, :d].T.double() * scale.double()).float()
            p_new = prob_func(y)
            accept = torch.where(p_new > 0, noise[t, d] * p < p_new, (p_new == 0) & (p == 0))
            x = torch.where(accept[:, None], y, x)
            p = torch.where(accept, p_new, p)
            accepted += accept.to(torch.int32)
            k = t0 + t - keep_from
            if out is not None and k >= 0 and k % keep_every == 0:
                out[k // keep_every] = x
        self.state = x.contiguous()


class LangevinSampler(_ChainSampler):
    """`chains` independent Metropolis-adjusted Langevin chains: the proposals of ``MetropolisHastingsSampler`` pushed along the
    gradient of the log-density, and the acceptance test made on logarithms.

    One step of a chain at x with l = log p(x), g = grad log p(x) and s = step per axis: drift(x) = clamp(s^2 g / 2, -drift_clip
    s, drift_clip s) per axis, y = x + drift(x) + s z, r = (x - y - drift(y)) / s, D = l(y) - l + (|z|^2 - |r|^2) / 2; accept iff
    ``l(y) > -inf ? (l == -inf or log u < D) : (l(y) == -inf and l == -inf)``, and never with a NaN in l(y), z or u.  The
    truncated drift is a function of the state alone, so the Metropolis correction is exact; ``drift_clip`` bounds it in proposal
    standard deviations (h' / h is unbounded next to a zero of a Lagrange function), 0 gives a driftless walk.  The conventions
    are those of the random-walk sampler: a chain inside the support never leaves it, a chain outside it (no drift there)
    random-walks until it finds it.  Because sums of logarithms are compared, the rule holds where the fp32 product of a hundred
    factors has underflowed and the random-walk sampler sees no support at all.

    Called with ``MENT.prob`` itself of a MENT whose slots all run through the kernels, the steps run in the fused kernel
    (mentflow_amd/csrc/mala.hip: state, log-density and gradient in registers).  Otherwise the same rule runs in torch ops, logged
    once, on ``log_density`` if given, else on ``MENT.log_density`` of the MENT that ``prob_func`` is bound to, with the gradient
    from autograd; without either a ``ValueError`` says so.  Call contract, persistence and noise as ``MetropolisHastingsSampler``.
    """

    _generic_note = "one log-density call and one backward pass per step"

    def __init__(self, ndim: int, chains: int = 65536, step: Union[float, Sequence[float]] = 0.25, burn: int = 200,
                 thin: int = 10, start: Optional[torch.Tensor] = None, start_scale: float = 1.0, persistent: bool = True,
                 burn_persistent: Optional[int] = None, device: torch.device = None, drift_clip: float = 1.0,
                 log_density: Optional[Callable] = None) -> None:
        super().__init__(ndim, chains, step, burn, thin, start, start_scale, persistent, burn_persistent, device)
        self.drift_clip = _check_drift(type(self).__name__, self.step, drift_clip)
        self.log_density = log_density

    def _target(self, prob_func: Callable, fused) -> Optional[Callable]:
        from .ment import MENT
        if fused is not None:
            return None
        if self.log_density is not None:
            return self.log_density
        # not _ment_of: log_density also serves a subclass's own prob, which the kernels do not compute, if the subclass says so
        owner = getattr(prob_func, "__self__", None)
        if isinstance(owner, MENT) and getattr(prob_func, "__func__", None) is type(owner).prob:
            # a subclass that overrides prob alone has a density that MENT.log_density does not describe
            if type(owner).prob is MENT.prob or type(owner).log_density is not MENT.log_density:
                if owner.ndim != self.ndim:
                    raise ValueError(f"LangevinSampler(ndim={self.ndim}) called with the density of a MENT of ndim={owner.ndim}")
                return owner.log_density
        raise ValueError("LangevinSampler needs a differentiable log-density: pass log_density=..., or call it with the bound "
                         f"prob of a MENT (got {getattr(prob_func, '__qualname__', prob_func)})")

    def _fused_steps(self, x, args, noise, scale, accepted, t0, keep_from, keep_every, out) -> None:
        ops.mala_ment_steps(x, args[0], args[1], args[2], args[3], noise, scale, accepted, drift_clip=self.drift_clip,
                            step_offset=t0, keep_from=keep_from, keep_every=keep_every, out=out)

    @staticmethod
    def _value_and_grad(log_density: Callable, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(l, grad l) at x with the kernel's conventions: the gradient row of a point outside the support is 0, that of a NaN
        point NaN."""
        x = x.detach().requires_grad_(True)
        with torch.enable_grad():
            lp = log_density(x)
            if not lp.requires_grad:
                raise ValueError("LangevinSampler needs a differentiable log-density: the one it was given returned a tensor that "
                                 "does not depend on x through autograd")
            (g,) = torch.autograd.grad(lp.sum(), x)
        lp = lp.detach()
        g = torch.where(torch.isneginf(lp)[:, None], torch.zeros_like(g), g)
        return lp, torch.where(torch.isnan(lp)[:, None], torch.full_like(g, float("nan")), g)

    def _generic_steps(self, log_density, noise, scale, accepted, t0, keep_from, keep_every, out) -> None:
        x, d = self.state, self.ndim
        a, c = (0.5 * scale) * scale, torch.tensor(self.drift_clip, dtype=torch.float32, device=x.device) * scale

        def drift(g):
            return torch.minimum(torch.maximum(a * g, -c), c)

        lp, g = self._value_and_grad(log_density, x)
        for t in range(noise.shape[0]):
            z, u = noise[t, :d].T, noise[t, d]
            # the kernel's fma(scale, z, x + drift): the fp32 product is exact in fp64, so a double rounding at most apart
            y = ((x + drift(g)).double() + z.double() * scale.double()).float()
            lp_new, g_new = self._value_and_grad(log_density, y)
            r = ((x - y) - drift(g_new)) / scale
            zz = (z * z).sum(1)
            delta = (lp_new - lp) + 0.5 * (zz - (r * r).sum(1))
            outside = torch.isneginf(lp)
            accept = torch.where(lp_new > float("-inf"), outside | (torch.log(u) < delta), torch.isneginf(lp_new) & outside)
            accept = accept & ~torch.isnan(u) & ~torch.isnan(zz)
            x = torch.where(accept[:, None], y, x)
            g = torch.where(accept[:, None], g_new, g)
            lp = torch.where(accept, lp_new, lp)
            accepted += accept.to(torch.int32)
            k = t0 + t - keep_from
            if out is not None and k >= 0 and k % keep_every == 0:
                out[k // keep_every] = x
        self.state = x.contiguous()


_AIS_NOISE_BYTES = 64 << 20         # noise of one launch of the ladder (the cut does not change a bit of the result)


class AnnealedImportanceSampler:
    """Annealed importance sampling (Neal 2001) on the density of a fully fused :class:`mentflow_amd.ment.MENT`: `chains`
    independent chains start from exact draws of a normalised Gaussian base q0 = N(base_mean, diag base_scale^2) and walk the
    ladder ``betas`` (0 = the base, 1 = the MENT density p) through the tempered densities q0^(1 - beta) p^beta.  At every
    temperature a chain's log-weight takes (beta_k - beta_{k-1}) (log p - log q0) at its state, then the chain takes
    ``steps_per_temp`` Langevin transitions (those of ``LangevinSampler``: same proposal, truncated drift and acceptance rule)
    on the tempered density.  The mean of the weights is an unbiased estimate of Z = integral of p, whatever the ladder and
    however short the moves; ``MENT.log_normalization`` turns them into log Z, an effective sample size and the entropy.

    Kernel in mentflow_amd/csrc/ais.hip (state, log-density, gradient and log-weight in registers; one launch per block of
    temperatures whose noise fits _AIS_NOISE_BYTES).  There is no generic path: only the single kernel chain of a MENT whose
    slots all run through the kernels is taken, anything else raises ``NotImplementedError``.

    ``base_scale=None`` takes the scale of a Gaussian prior, or 1.0 per axis under the box prior; chains that start outside
    the support get weight 0.  ``betas=None`` is ``linspace(0, 1, n_temps + 1)``; a ladder of one's own must start at 0, end
    at 1 and not decrease.  ``seed`` fixes the noise (a generator of its own per run), else the device's default generator
    is used.  ``sampler(prob_func, size)`` runs the ladder and returns ``size`` points resampled from the weighted final
    states by systematic resampling with one uniform, so the class serves as ``MENT(sampler=...)``."""

    def __init__(self, ndim: int, chains: int = 4096, n_temps: int = 64, steps_per_temp: int = 2,
                 step: Union[float, Sequence[float]] = 0.25, drift_clip: float = 1.0, base_mean=None, base_scale=None,
                 betas=None, seed: Optional[int] = None, device: torch.device = None) -> None:
        name = type(self).__name__
        bad_step = f"{name}: step must be a positive float or {int(ndim)} positive per-axis scales (got {step})"
        self.ndim, self.step = _check_axes(name, ndim, step, bad_step)
        self.drift_clip = _check_drift(name, self.step, drift_clip, bad_step)
        self.chains, self.steps_per_temp = int(chains), int(steps_per_temp)
        if self.chains < 1 or self.steps_per_temp < 0:
            raise ValueError(f"{name}: chains >= 1 and steps_per_temp >= 0 expected")
        if betas is None:
            if int(n_temps) < 1:
                raise ValueError(f"{name}: n_temps >= 1 expected (got {n_temps})")
            betas = torch.linspace(0.0, 1.0, int(n_temps) + 1)
        betas = torch.as_tensor(betas, dtype=torch.float32).detach().cpu().reshape(-1)
        if betas.numel() < 2 or float(betas[0]) != 0.0 or float(betas[-1]) != 1.0 or not bool((betas[1:] >= betas[:-1]).all()):
            raise ValueError(f"{name}: betas must start at 0, end at 1 and not decrease")
        self.betas = betas
        self.n_temps = betas.numel() - 1
        self.base_mean = _per_axis(name, self.ndim, base_mean, 0.0, "base_mean")
        self.base_scale = None if base_scale is None else _per_axis(name, self.ndim, base_scale, 1.0, "base_scale")
        if self.base_scale is not None and not all(0.0 < b < math.inf for b in self.base_scale):
            raise ValueError(f"{name}: base_scale > 0 expected on every axis (got {self.base_scale})")
        self.seed = None if seed is None else int(seed)
        self.device = device
        self.acceptance: Optional[torch.Tensor] = None
        self.last: Optional[dict] = None                 # what the latest run returned
        self._gen: Optional[torch.Generator] = None      # the latest run's generator: __call__ draws its one uniform from it

    def to(self, device):
        self.device = device
        return self

    def _prepare(self, ment):
        """(kernel arguments of `ment`, device, base scale per axis): the checks every walk starts with."""
        from .ment import MENT
        from .prior import Gaussian
        name = type(self).__name__
        if not isinstance(ment, MENT):
            raise TypeError(f"{name}.run takes a MENT (got {type(ment).__name__})")
        if ment.ndim != self.ndim:
            raise ValueError(f"{name}(ndim={self.ndim}) called with a MENT of ndim={ment.ndim}")
        args = ment.fused_args()
        if args is None:
            raise NotImplementedError(f"{name}: this MENT has slots behind a pre-transform chain or evaluated in torch; only a "
                                      "MENT whose slots all run through the kernels on plain LinearTransforms is supported")
        device = torch.device(self.device) if self.device is not None else ment._device()
        base = self.base_scale
        if base is None:
            base = [float(ment.prior.scale)] * self.ndim if isinstance(ment.prior, Gaussian) else [1.0] * self.ndim
        return args, device, base

    def _start(self, device, base):
        """(generator, x, logw, logp, accepted): exact draws of the base and what the chains carry."""
        gen = None
        if self.seed is not None:
            gen = torch.Generator(device=device)
            gen.manual_seed(self.seed)
        mean_t = torch.tensor(self.base_mean, dtype=torch.float32, device=device)
        base_t = torch.tensor(base, dtype=torch.float32, device=device)
        x = (mean_t + base_t * torch.randn(self.chains, self.ndim, device=device, generator=gen)).contiguous()
        _lib.ptr(x)                                            # the usual refusal of tensors the library does not compute on
        logw = torch.zeros(self.chains, dtype=torch.float64, device=device)
        logp = torch.empty(self.chains, dtype=torch.float32, device=device)
        accepted = torch.zeros(self.chains, dtype=torch.int32, device=device)
        return gen, x, logw, logp, accepted

    def _walk(self, args, base, gen, x, logw, logp, accepted, betas, spt: int, k_from: int, k_to: int) -> None:
        """Temperatures k_from + 1 .. k_to of `betas` (on the device), in launches whose noise fits _AIS_NOISE_BYTES."""
        d, chains, device = self.ndim, self.chains, x.device
        scale = torch.tensor(self.step, dtype=torch.float32, device=device)
        per = max(1, _AIS_NOISE_BYTES // (4 * (d + 1) * chains * max(1, spt)))
        for k0 in range(k_from, k_to, per):
            k1 = min(k_to, k0 + per)
            nz = torch.empty((k1 - k0) * spt, d + 1, chains, device=device)
            for k in range(k1 - k0):                           # drawn per temperature: the stream does not depend on the cut
                nz[k * spt:(k + 1) * spt, :d].normal_(generator=gen)
                nz[k * spt:(k + 1) * spt, d].uniform_(generator=gen)
            ops.ais_ment_steps(x, args[0], args[1], args[2], args[3], nz, betas, spt, scale, self.base_mean, base, logw,
                               accepted, drift_clip=self.drift_clip, temp_offset=k0, ntemps=k1 - k0, logp=logp)

    def run(self, ment) -> dict:
        """Walk the whole ladder on `ment` and return ``x`` [chains, ndim] (the final states), ``logw`` [chains] float64 (the
        log-weights), ``logp`` [chains] (``ment.log_density`` of the final states, as the kernel carries it) and ``accepted``
        [chains] int32, all on the device.  No host synchronisation."""
        args, device, base = self._prepare(ment)
        gen, x, logw, logp, accepted = self._start(device, base)
        self._walk(args, base, gen, x, logw, logp, accepted, self.betas.to(device), self.steps_per_temp, 0, self.n_temps)
        self.acceptance = accepted.sum().to(torch.float32) / float(max(1, self.n_temps * self.steps_per_temp) * self.chains)
        self.last = dict(x=x, logw=logw, logp=logp, accepted=accepted)
        self._gen = gen
        return self.last

    @staticmethod
    def _weights(res: dict) -> Tuple[torch.Tensor, torch.Tensor]:
        """(x, w = exp(logw - max logw) in fp32) of a run's dict: the largest weight is 1, a chain without weight has 0."""
        logw = res["logw"]
        return res["x"], torch.exp(logw - logw.max()).to(torch.float32)

    def sample_weighted(self, prob_func: Callable, size: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Run the ladder and return the final states as they are, with their weights: (x [chains, ndim] fp32, w [chains]
        fp32, w = exp(logw - max logw)) of ``run()``.  Nothing is resampled; `size` is ignored (there are `chains` rows).
        The weighted histograms (``Histogram*.batched(..., weights=w)``, ``MENT.weighted``) consume the pair."""
        return self._weights(self.run(_ment_of(prob_func, required_by=type(self).__name__)))

    def __call__(self, prob_func: Callable, size: int) -> torch.Tensor:
        owner = _ment_of(prob_func, required_by=type(self).__name__)
        res = self.run(owner)
        x, logw = res["x"], res["logw"]
        size = int(size)
        # systematic resampling: the points (u + i) / size, one uniform u, through the cumulative normalised weights
        w = torch.exp(logw - logw.max())
        cdf = torch.cumsum(w, 0)
        u = torch.rand(1, dtype=torch.float64, device=x.device, generator=self._gen)
        pos = (u + torch.arange(size, dtype=torch.float64, device=x.device)) * (cdf[-1] / size)
        idx = torch.searchsorted(cdf, pos, right=True).clamp_(max=self.chains - 1)
        return x[idx]


class SequentialMonteCarloSampler(AnnealedImportanceSampler):
    """A sequential Monte Carlo sampler on the density of a fully fused :class:`mentflow_amd.ment.MENT`: the chains, ladder and
    weights of ``AnnealedImportanceSampler``, plus adaptive resampling on the way and a population that is kept across calls.

    The `chains` states form `groups` independent islands of ``chains / groups`` consecutive chains.  The ladder is walked in
    launches of ``resample_every`` temperatures; after every launch but the last, each island whose effective sample size has
    fallen below ``ess_threshold`` times its size is resampled systematically from its own weights, with one uniform per
    island, and its log-weights all become the island's log mean weight (kernel in mentflow_amd/csrc/smc.hip).  Every decision
    is taken on the device: there is no host synchronisation.  Islands never exchange states, so the `groups` estimates
    ``log_z_groups`` of log Z are independent and their spread is an honest standard error however often the chains were
    resampled (``MENT.log_normalization``).  The noise of the moves is drawn as ``AnnealedImportanceSampler`` draws it and the
    resampling uniforms come from a second generator (seeded ``(seed * 2654435761 + 1) mod 2^63``), so ``ess_threshold=0``
    (no resampling launch at all) gives that class's ``run`` bit for bit.

    ``sampler(prob_func, size)`` serves as ``MENT(sampler=...)``.  The first call (and every call with ``persistent=False``, or
    after ``reset()``) walks the ladder.  Later calls bridge instead: the kept population is reweighted by the ratio of the new
    density to the old one (``logw += log p_new(x) - log p_old(x)``, -inf where either side has no weight), resampled once
    under ``ess_threshold`` and moved by ``bridge_steps`` Langevin transitions on the new density.  Between two Gauss-Seidel
    sub-steps the density changes by a bounded factor in one table, which is one such step away.  In both cases the sample is
    then collected: every island is resampled (which equalises its weights), and ``ceil(size / chains)`` rounds of ``thin``
    transitions on the density each contribute the population.  ``last`` holds the latest dict (its ``logw`` are the weights
    before that forced resampling), ``population`` the kept states with their weights and log-densities, and ``log_z`` the
    running estimate ``logsumexp(log_z_groups) - log groups``, which follows the tables from call to call."""

    def __init__(self, ndim: int, chains: int = 4096, n_temps: int = 64, steps_per_temp: int = 2,
                 step: Union[float, Sequence[float]] = 0.25, drift_clip: float = 1.0, base_mean=None, base_scale=None,
                 betas=None, seed: Optional[int] = None, device: torch.device = None, groups: int = 8,
                 ess_threshold: float = 0.5, resample_every: int = 1, persistent: bool = True, bridge_steps: int = 4,
                 thin: int = 2) -> None:
        super().__init__(ndim, chains, n_temps, steps_per_temp, step, drift_clip, base_mean, base_scale, betas, seed, device)
        name = type(self).__name__
        self.groups = int(groups)
        if self.groups < 1 or self.chains % self.groups != 0:
            raise ValueError(f"{name}: groups >= 1 that divides chains expected (got {groups} for {self.chains} chains)")
        self.ess_threshold = float(ess_threshold)
        if not self.ess_threshold >= 0.0:
            raise ValueError(f"{name}: ess_threshold >= 0 expected (got {ess_threshold})")
        self.resample_every, self.bridge_steps, self.thin = int(resample_every), int(bridge_steps), int(thin)
        if self.resample_every < 1 or self.bridge_steps < 0 or self.thin < 1:
            raise ValueError(f"{name}: resample_every >= 1, bridge_steps >= 0 and thin >= 1 expected")
        self.persistent = bool(persistent)
        self.population: Optional[dict] = None           # x, logw, logp kept from the latest call
        self.log_z: Optional[torch.Tensor] = None
        self._gen_u: Optional[torch.Generator] = None    # the resampling uniforms' generator

    def reset(self) -> None:
        """Forget the population: the next call walks the whole ladder."""
        self.population = None

    def to(self, device):
        self.device = device
        if self.population is not None:
            self.population = {k: v.to(device) for k, v in self.population.items()}
        return self

    # ---------------------------------------------------------------------------------------------------- internals
    def _resample(self, x, logw, threshold: float):
        """One resampling decision per island: (x, ancestors as int64, how many islands resampled); logw in place."""
        u = torch.rand(self.groups, dtype=torch.float64, device=x.device, generator=self._gen_u)
        x, ancestors, stats = ops.smc_resample(x, logw, u, self.groups, threshold)
        return x, ancestors.long(), stats[:, 2].sum()

    def _finish(self, x, logw, logp, accepted, resampled, transitions: int) -> dict:
        per_island = logw.view(self.groups, -1)
        lse = torch.logsumexp(per_island, 1)
        wt = torch.exp(per_island - torch.where(torch.isneginf(lse), torch.zeros_like(lse), lse)[:, None])
        ess = torch.where(torch.isneginf(lse), torch.zeros_like(lse), 1.0 / (wt * wt).sum(1).clamp_min(1e-300))
        log_z_groups = lse - math.log(per_island.shape[1])
        self.log_z = torch.logsumexp(log_z_groups, 0) - math.log(self.groups)
        if transitions:
            self.acceptance = accepted.sum().to(torch.float32) / float(transitions * self.chains)
        self.last = dict(x=x, logw=logw, logp=logp, accepted=accepted, log_z_groups=log_z_groups, ess_groups=ess,
                         resampled=resampled)
        return self.last

    def run(self, ment) -> dict:
        """Walk the whole ladder on `ment` and return what ``AnnealedImportanceSampler.run`` returns (``x``, ``logw``,
        ``logp``, ``accepted``) plus ``log_z_groups`` [groups] float64 (logsumexp of each island's log-weights minus the log
        of its size), ``ess_groups`` [groups] (each island's effective sample size under its final weights) and ``resampled``
        (0-dim: how many island resamplings took place), all on the device.  The final weights are not resampled, so they
        stay informative for the entropy.  The kept population is not touched.  No host synchronisation."""
        args, device, base = self._prepare(ment)
        gen, x, logw, logp, accepted = self._start(device, base)
        self._gen = gen
        self._gen_u = None
        if self.seed is not None:
            self._gen_u = torch.Generator(device=device)
            self._gen_u.manual_seed((self.seed * 2654435761 + 1) % (1 << 63))
        betas = self.betas.to(device)
        resampled = torch.zeros((), dtype=torch.float64, device=device)
        for k0 in range(0, self.n_temps, self.resample_every):
            k1 = min(self.n_temps, k0 + self.resample_every)
            self._walk(args, base, gen, x, logw, logp, accepted, betas, self.steps_per_temp, k0, k1)
            if k1 < self.n_temps and self.ess_threshold > 0.0:
                x, ancestors, count = self._resample(x, logw, self.ess_threshold)
                logp, accepted = logp[ancestors], accepted[ancestors]
                resampled = resampled + count
        return self._finish(x, logw, logp, accepted, resampled, self.n_temps * self.steps_per_temp)

    def _at_target(self, args, base, x, logw, logp, accepted, steps: int) -> None:
        """`steps` Langevin transitions on the density itself: the ladder [1, 1], whose weight increment is exactly 0."""
        ones = torch.ones(2, dtype=torch.float32, device=x.device)
        self._walk(args, base, self._gen, x, logw, logp, accepted, ones, steps, 0, 1)

    def _bridge(self, ment) -> dict:
        args, device, base = self._prepare(ment)
        pop = self.population
        x, logw, lp_old = pop["x"], pop["logw"].clone(), pop["logp"]
        _lib.ptr(x)
        lp_new = ops.ment_logprob(x, args[0], args[1], args[2], args[3])[0]
        dead = torch.isneginf(logw) | torch.isneginf(lp_new) | torch.isneginf(lp_old)
        zero = torch.zeros((), dtype=torch.float64, device=device)
        inc = torch.where(dead, zero, lp_new.double()) - torch.where(dead, zero, lp_old.double())   # never inf - inf
        logw = torch.where(dead, torch.full_like(logw, float("-inf")), logw + inc)
        logp = lp_new
        accepted = torch.zeros(self.chains, dtype=torch.int32, device=device)
        resampled = torch.zeros((), dtype=torch.float64, device=device)
        if self.ess_threshold > 0.0:
            x, ancestors, resampled = self._resample(x, logw, self.ess_threshold)
            logp = logp[ancestors]
        else:
            x = x.clone()
        if self.bridge_steps:
            self._at_target(args, base, x, logw, logp, accepted, self.bridge_steps)
        return self._finish(x, logw, logp, accepted, resampled, self.bridge_steps)

    def sample_weighted(self, prob_func: Callable, size: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The population with its weights, (x [chains, ndim] fp32, w [chains] fp32, w = exp(logw - max logw)): walks the ladder
        or bridges exactly as ``__call__`` decides, but neither forces the final resampling nor runs the collection rounds.
        The population is kept with its unequalised log-weights, from which the next call bridges.  `size` is ignored."""
        owner = _ment_of(prob_func, required_by=type(self).__name__)
        if not self.persistent:
            self.reset()
        res = self.run(owner) if self.population is None else self._bridge(owner)
        self.population = dict(x=res["x"], logw=res["logw"], logp=res["logp"])
        return self._weights(res)

    def __call__(self, prob_func: Callable, size: int) -> torch.Tensor:
        owner = _ment_of(prob_func, required_by=type(self).__name__)
        size = int(size)
        if not self.persistent:
            self.reset()
        res = self.run(owner) if self.population is None else self._bridge(owner)
        args, device, base = self._prepare(owner)
        # a forced resampling of every island equalises the weights; then rounds of moves on the density, each kept
        logw = res["logw"].clone()
        x, ancestors, _ = self._resample(res["x"], logw, 2.0)
        logp = res["logp"][ancestors]
        accepted = torch.zeros(self.chains, dtype=torch.int32, device=device)
        rounds = max(1, math.ceil(size / self.chains))
        out = torch.empty(rounds, self.chains, self.ndim, device=device)
        for r in range(rounds):
            self._at_target(args, base, x, logw, logp, accepted, self.thin)
            out[r] = x
        self.population = dict(x=x, logw=logw, logp=logp)
        return out.reshape(-1, self.ndim)[:size]
