"""Classical MENT (iterative maximum-entropy tomography) — mirrors mentflow/ment.py on the gfx950 kernels of
mentflow_amd/csrc/ment.hip.  Same names, constructor keywords and methods as the reference.

The density is ``prob(x) = prod_ij clamp(h_ij(project_j(T_i x)), 0, 1e10) * exp(prior.log_prob(x))`` in fp32, where each
Lagrange function h_ij is the linear (1-D) or bilinear (2-D) interpolant of its values at the measurement's bin centres,
0 outside the closed hull of the centres (scipy's RegularGridInterpolator with bounds_error=False, fill_value=0, as the
reference uses it).  Every (transform, diagnostic) pair whose transform is a LinearTransform (optionally behind a chain of
pre-transforms, as ``simulate.group_measurements`` splits them) and whose diagnostic is a Histogram1D/2D on uniform bins is
a SLOT of one fused kernel launch per pre-transform chain: its projection rows ``diagnostic.projection_rows(matrix)``, the
centre grid and the table go to the kernel, which evaluates all slots per point.  Any other pair is evaluated in torch on the
device (transform, ``diagnostic.project``, ``LagrangeFunction``): same values, not fused.

``MENT.log_density`` (not in the reference) is the logarithm of that density as a sum of logarithms, differentiable in x, on the
kernel of mentflow_amd/csrc/ment_logp.hip: finite where the fp32 product has left its range, and what ``prior.MENTPrior`` and a
reverse-KL fit of a flow to a MENT solution are built on.

Deliberate differences from the reference (each a bug or a CPU-only limit there):
  - ``simulate_all`` in integrate mode integrates every slot (the reference calls a missing ``simulate_integrate``);
  - integrate mode handles 2-D slots (the reference reshapes with ``diagnostic.shape``, which its Histogram2D lacks);
  - ``prior=None`` is the density the reference's docstring states: uniform on [-100, 100]^ndim (its code names an
    undefined ``UniformPrior``);
  - integrate mode with a ``direction`` diagnostic raises NotImplementedError (the reference silently integrates along
    ``axis``); only ``interpolation="linear"`` exists; priors other than ``prior.Gaussian`` / None raise;
  - ``gauss_seidel_update`` updates the tables with elementwise device ops (the reference loops over bins in Python);
  - ``LagrangeFunction(x)`` returns the interpolant clamped to [0, 1e10] (the clamp MENT.prob applies to every factor);
  - ``ndim > 8`` raises NotImplementedError (the kernels' limit, as for the projection kernels).
"""
from __future__ import annotations

import math
from typing import Any, Callable, List, Optional, Tuple

import torch

from . import ops
from .diagnostics import Histogram, Histogram1D, Histogram2D
from .loss import kl_divergence
from .prior import Gaussian
from .simulate import forward
from .simulate.simulate import apply_pre, split_transform
from .simulate.transform import LinearTransform
from .utils import coords_from_edges, get_grid_points, unravel

# A centre grid is handed to the kernels when every centre lies within this many bin widths of the straight line through
# the first and last ones (fp64).  The kernels place u at (u - c_0) / delta, so this bounds the error of the interpolation
# weight, and with it each factor's error relative to the table's range, at the 1e-5 the tests gate products at.  fp32
# linspace edges of the usual grids sit ~2e-6 bin widths off the line (85 bins on [-4, 4]); offset grids such as
# [997, 1003] (1e-3) take the torch path, which interpolates between the stored centres exactly as scipy does.
UNIFORM_CENTRES_TOL = 1.0e-5
_MAX_TORCH_ROWS = 1 << 22          # points per chunk of the integrate fall-back
MAX_NDIM = 8                       # phase-space dimension limit of the kernels (MENT_DMAX in csrc/ment.hip)


def _uniform_centres(c: torch.Tensor) -> bool:
    c = c.detach().to("cpu", torch.float64).reshape(-1)
    if c.numel() < 2:
        return False
    step = (c[-1] - c[0]) / (c.numel() - 1)
    if not float(step) > 0.0:
        return False
    line = c[0] + step * torch.arange(c.numel(), dtype=torch.float64)
    return float((c - line).abs().max() / step) <= UNIFORM_CENTRES_TOL


def _axis_desc(c: torch.Tensor) -> List[float]:
    c = c.detach().to("cpu", torch.float64).reshape(-1)
    delta = float(c[-1] - c[0]) / (c.numel() - 1)
    return [float(c[0]), float(c[-1]), 1.0 / delta]


def _slot_rows(rows: List[torch.Tensor], coords: List[torch.Tensor], d: int) -> Tuple[List[float], List[int]]:
    """One descriptor row (include/mentflow_hip.h): [r0 | r1 | c0_x, c_last_x, 1/dx | c0_y, c_last_y, 1/dy | 0 0] and
    meta [ndim, Bx, By] (the table offset is appended by the caller)."""
    desc = [0.0] * ops.MENT_DESC
    for k, r in enumerate(rows):
        desc[8 * k:8 * k + d] = [float(v) for v in r.detach().to("cpu", torch.float32).reshape(-1)]
    for k, c in enumerate(coords):
        desc[16 + 3 * k:19 + 3 * k] = _axis_desc(c)
    meta = [len(rows), coords[0].numel(), coords[1].numel() if len(coords) > 1 else 1]
    return desc, meta


def _interp_torch(coords: List[torch.Tensor], values: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """Linear / bilinear interpolation between stored centres (any spacing), 0 outside the hull, NaN for NaN."""
    w, idx, inside, nan = [], [], None, None
    for k, c in enumerate(coords):
        c = c.to(u.device, torch.float32).reshape(-1)
        uk = u[:, k]
        i = (torch.searchsorted(c, uk.contiguous(), right=True) - 1).clamp(0, c.numel() - 2)
        wk = ((uk - c[i]) / (c[i + 1] - c[i])).clamp(max=1.0)
        ok = (uk >= c[0]) & (uk <= c[-1])
        inside = ok if inside is None else inside & ok
        nan = torch.isnan(uk) if nan is None else nan | torch.isnan(uk)
        w.append(wk)
        idx.append(i)
    v = values.to(u.device, torch.float32)
    if len(coords) == 1:
        h = v[idx[0]] * (1.0 - w[0]) + v[idx[0] + 1] * w[0]
    else:
        i, k, wx, wy = idx[0], idx[1], w[0], w[1]
        h = (v[i, k] * ((1.0 - wx) * (1.0 - wy)) + v[i, k + 1] * ((1.0 - wx) * wy) + v[i + 1, k] * (wx * (1.0 - wy))
             + v[i + 1, k + 1] * (wx * wy))
    h = torch.where(inside, h, torch.zeros_like(h))
    return torch.where(nan, torch.full_like(h, float("nan")), h)


class UniformPrior:
    """Uniform density on [-scale, scale]^ndim: the reference's default prior as its docstring states it."""

    def __init__(self, ndim: int = 2, scale: float = 100.0, device=None) -> None:
        self.ndim, self.scale, self.device = int(ndim), float(scale), device

    def to(self, device) -> "UniformPrior":
        self.device = device
        return self

    def log_norm(self) -> float:
        return -self.ndim * math.log(2.0 * self.scale)

    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        inside = (x.abs() <= self.scale).all(dim=1)
        return torch.where(inside, torch.full_like(x[:, 0], self.log_norm()), torch.full_like(x[:, 0], float("-inf")))


def _prior_args(prior) -> Tuple[int, float, float]:
    if isinstance(prior, Gaussian):
        return 1, prior.scale, prior.log_norm()
    if isinstance(prior, UniformPrior):
        return 2, prior.scale, prior.log_norm()
    raise NotImplementedError(f"MENT prior {type(prior).__name__}: the kernels take prior.Gaussian or None (uniform box)")


class LagrangeFunction:
    """ment.py:20-52: h on the grid of bin centres `coords` ([B] tensor for 1-D, [cx, cy] for 2-D) with `values`."""

    def __init__(self, coords: List[torch.Tensor], values: torch.Tensor, **interpolation_kws) -> None:
        self.coords = coords
        self.values = values
        self.interpolation_kws = interpolation_kws
        self.interpolation_kws.setdefault("method", "linear")
        self.interpolation_kws.setdefault("bounds_error", False)
        self.interpolation_kws.setdefault("fill_value", 0.0)
        method = self.interpolation_kws["method"]
        if method != "linear" or self.interpolation_kws["bounds_error"] or self.interpolation_kws["fill_value"] != 0.0:
            raise NotImplementedError(f"LagrangeFunction: interpolation method '{method}' (bounds_error="
                                      f"{self.interpolation_kws['bounds_error']}, fill_value="
                                      f"{self.interpolation_kws['fill_value']}): only 'linear' with fill_value 0 exists")
        self.set_values(values)

    def coord_list(self) -> List[torch.Tensor]:
        return [self.coords] if torch.is_tensor(self.coords) else list(self.coords)

    def uniform(self) -> bool:
        return all(_uniform_centres(c) for c in self.coord_list())

    def set_values(self, values: torch.Tensor) -> None:
        self.values = values

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """clamp(h, 0, 1e10) at projected coordinates x ([n] or [n, 1] for 1-D, [n, 2] for 2-D): a tensor on x's device.
        The clamp is MENT.prob's (ment.py:231), applied here on every grid; it differs from the bare interpolant only for
        tables with negative entries, which an update with lr > 1 can produce."""
        coords = self.coord_list()
        u = x.reshape(x.shape[0], len(coords)).to(torch.float32).contiguous()
        if not self.uniform():
            return torch.clamp(_interp_torch(coords, self.values, u), 0.0, 1.00e10)
        dim = len(coords)
        desc, meta = _slot_rows([torch.eye(dim)[k] for k in range(dim)], coords, dim)
        dt = torch.tensor([desc], dtype=torch.float32).to(u.device)
        mt = torch.tensor([meta + [0]], dtype=torch.int32).to(u.device)
        tab = self.values.to(u.device, torch.float32).reshape(-1).contiguous()
        return ops.ment_prob(u, dt, mt, tab)


class _Chain:
    """Slots that share one pre-transform chain: one kernel launch per evaluation."""

    def __init__(self, pre):
        self.pre = pre
        self.slots: List[Tuple[int, int]] = []
        self.desc: List[List[float]] = []
        self.meta: List[List[int]] = []
        self.rows: List[List[torch.Tensor]] = []
        self.desc_t = self.meta_t = None


class MENT:
    """ment.py:55-428: iterative maximum-entropy tomography (MENT) solver."""

    def __init__(self, ndim: int, transforms: List[Callable], diagnostics: List[List[Callable]],
                 measurements: List[List[torch.Tensor]], discrepancy_function: Callable = kl_divergence, prior: Any = None,
                 interpolation: str = "linear", mode: str = "integrate", integration_limits: List[Tuple[float]] = None,
                 integration_shape: Tuple[int] = None, sampler: Optional[Callable] = None, n_samples: int = 1000000,
                 device: Optional[torch.device] = None, verbose: bool = False) -> None:
        if interpolation != "linear":
            raise NotImplementedError(f"MENT interpolation '{interpolation}': only 'linear' is implemented")
        if not 1 <= int(ndim) <= MAX_NDIM:
            raise NotImplementedError(f"MENT with ndim={ndim}: the kernels take 1 <= ndim <= {MAX_NDIM}")
        self.device = device
        self.verbose = verbose
        self.mode = mode
        self.ndim = ndim
        self.epoch = 0
        self._plan = None
        self.transforms = transforms
        self.diagnostics = self.set_diagnostics(diagnostics)
        self.measurements = self.set_measurements(measurements)
        self.discrepancy_function = discrepancy_function
        self.prior = prior
        if self.prior is None:
            self.prior = UniformPrior(ndim=ndim, scale=100.0)
        _prior_args(self.prior)
        self.integration_limits = integration_limits
        self.integration_shape = integration_shape
        self.sampler = sampler
        self._weighted = False                                # see the `weighted` property
        self.n_samples = int(n_samples)
        self.interpolation = interpolation
        self.lagrange_functions = self.initialize_lagrange_functions()
        self.log_z: Optional[torch.Tensor] = None            # log of the normaliser, once log_normalization has estimated it

    @property
    def weighted(self) -> bool:
        """Sample mode with particle weights: when set, a simulation takes the sampler's states with their importance weights
        (``sampler.sample_weighted``) and bins them as they are, instead of ``n_samples`` equal-weight rows resampled from them.
        An attribute, set after construction (the constructor keeps the reference's signature); setting it with a sampler
        that has no ``sample_weighted`` raises ``TypeError``, and so does a simulation after ``sampler`` was replaced by one
        that has none."""
        return self._weighted

    @weighted.setter
    def weighted(self, value: bool) -> None:
        if value:
            self._check_weighted_sampler()
        self._weighted = bool(value)

    def _check_weighted_sampler(self) -> None:
        if not callable(getattr(self.sampler, "sample_weighted", None)):
            raise TypeError(f"MENT.weighted needs a sampler with sample_weighted (AnnealedImportanceSampler, "
                            f"SequentialMonteCarloSampler); got {type(self.sampler).__name__}")

    def send(self, x):
        return x.type(torch.float32).to(self.device)

    def set_diagnostics(self, diagnostics: List[List[Callable]]):
        self.diagnostics = diagnostics
        if self.diagnostics is None:
            self.diagnostics = [[]]
        self._plan = None
        return self.diagnostics

    def set_measurements(self, measurements: List[List[torch.Tensor]]):
        self.measurements = measurements
        if self.measurements is None:
            self.measurements = [[]]
        return self.measurements

    def initialize_lagrange_functions(self) -> List[List[LagrangeFunction]]:
        self.lagrange_functions = []
        for index in range(len(self.measurements)):
            self.lagrange_functions.append([])
            for measurement, diagnostic in zip(self.measurements[index], self.diagnostics[index]):
                edges = diagnostic.edges
                if measurement.ndim == 1:
                    coords = coords_from_edges(edges)
                else:
                    coords = [coords_from_edges(e) for e in edges]
                values = (measurement > 0.0).float()
                self.lagrange_functions[-1].append(LagrangeFunction(coords, values, method=self.interpolation))
        self._plan = None
        return self.lagrange_functions

    def normalize_projection(self, projection: torch.Tensor, index: int, diag_index: int) -> torch.Tensor:
        diagnostic = self.diagnostics[index][diag_index]
        if diagnostic.ndim == 1:
            bin_volume = diagnostic.edges[1] - diagnostic.edges[0]
        else:
            bin_volume = math.prod((e[1] - e[0]) for e in diagnostic.edges)
        return projection / projection.sum() / bin_volume

    def get_meas_points(self, index: int, diag_index: int) -> torch.Tensor:
        diagnostic = self.diagnostics[index][diag_index]
        if diagnostic.ndim == 1:
            return coords_from_edges(diagnostic.edges)
        return get_grid_points(*[coords_from_edges(e) for e in diagnostic.edges])

    def _axes(self, index: int, diag_index: int) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
        meas_axis = self.diagnostics[index][diag_index].axis
        if type(meas_axis) is int:
            meas_axis = (meas_axis,)
        meas_axis = tuple(meas_axis)
        return meas_axis, tuple(a for a in range(self.ndim) if a not in meas_axis)

    def _integration_coords(self, index: int, diag_index: int) -> List[torch.Tensor]:
        limits = self.integration_limits[index][diag_index]
        shape = self.integration_shape[index][diag_index]
        _, int_axis = self._axes(index, diag_index)
        return [self.send(torch.linspace(limits[k][0], limits[k][1], shape[k])) for k in range(len(int_axis))]

    def get_integration_points(self, index: int, diag_index: int) -> torch.Tensor:
        int_coords = self._integration_coords(index, diag_index)
        if len(int_coords) == 1:
            return self.send(int_coords[0])
        return self.send(get_grid_points(*int_coords))

    def evaluate_lagrange_function(self, u: torch.Tensor, index: int, diag_index: int) -> torch.Tensor:
        diagnostic = self.diagnostics[index][diag_index]
        lagrange_function = self.lagrange_functions[index][diag_index]
        return self.send(lagrange_function(diagnostic.project(u)))

    # ---------------------------------------------------------------------------------------------------- the density
    def _device(self):
        if self.device is not None:
            return torch.device(self.device)
        for m in unravel(self.measurements):
            return m.device
        return torch.device("cpu")

    def _get_plan(self):
        """(chains, torch_slots): the slots of each pre-transform chain ((), the chain of plain LinearTransforms, comes
        first and carries the prior) and the (i, j) pairs evaluated in torch."""
        dev = self._device()
        if self._plan is not None and self._plan[2] == dev:
            return self._plan[0], self._plan[1]
        chains = {(): _Chain(())}
        torch_slots = []
        for i, transform in enumerate(self.transforms):
            try:
                pre, linear = split_transform(transform)
            except NotImplementedError:
                pre, linear = None, None
            for j, diagnostic in enumerate(self.diagnostics[i]):
                lf = self.lagrange_functions[i][j]
                ok = linear is not None and isinstance(diagnostic, (Histogram1D, Histogram2D)) and lf.uniform()
                if not ok:
                    torch_slots.append((i, j))
                    continue
                key = tuple(id(t) for t in pre)
                chain = chains.setdefault(key, _Chain(pre))
                rows = diagnostic.projection_rows(linear.matrix)
                desc, meta = _slot_rows(rows, lf.coord_list(), self.ndim)
                chain.slots.append((i, j))
                chain.desc.append(desc)
                chain.meta.append(meta)
                chain.rows.append(rows)
        for chain in chains.values():
            off, meta = 0, []
            for m in chain.meta:
                meta.append(m + [off])
                off += m[1] * m[2]
            chain.desc_t = torch.tensor(chain.desc, dtype=torch.float32).reshape(-1, ops.MENT_DESC).to(dev)
            chain.meta_t = torch.tensor(meta, dtype=torch.int32).reshape(-1, 4).to(dev)
        self._plan = (list(chains.values()), torch_slots, dev, {})
        return self._plan[0], self._plan[1]

    def _torch_slot_args(self, i: int, j: int):
        """(desc, meta) that hand a slot outside the chains to the log-density kernel on its projected coordinates (identity
        rows), or None when its centres are not uniform (_interp_torch then).  Decided once per plan: the test of the centres
        reads them on the host."""
        cache = self._plan[3]
        if (i, j) not in cache:
            lf = self.lagrange_functions[i][j]
            args = None
            if lf.uniform():
                coords = lf.coord_list()
                dim = len(coords)
                desc, meta = _slot_rows([torch.eye(dim)[k] for k in range(dim)], coords, dim)
                args = (torch.tensor([desc], dtype=torch.float32).to(self._plan[2]),
                        torch.tensor([meta + [0]], dtype=torch.int32).to(self._plan[2]))
            cache[(i, j)] = args
        return cache[(i, j)]

    def _tables(self, chain: _Chain) -> torch.Tensor:
        if not chain.slots:
            return torch.zeros(1, dtype=torch.float32, device=self._device())
        return torch.cat([self.lagrange_functions[i][j].values.to(self._device(), torch.float32).reshape(-1)
                          for i, j in chain.slots]).contiguous()

    def fully_fused(self) -> bool:
        """Every slot is a kernel slot of the plain-LinearTransform chain (the implicit-grid and integrate kernels apply)."""
        chains, torch_slots = self._get_plan()
        return not torch_slots and len(chains) == 1

    def log_prob(self, x: torch.Tensor, pad: float = 1.00e-12) -> torch.Tensor:
        return torch.log(self.prob(x) + pad)

    def log_density(self, x: torch.Tensor, pad: float = 0.0, normalized: bool = False) -> torch.Tensor:
        """log of the (unnormalised) density of ``prob``, differentiable in x and in the Lagrange tables
        (``lagrange_functions[i][j].values``): the sum over all slots of log clamp(h, 0, 1e10) plus ``prior.log_prob(x)``, from
        ops.MentLogProbFn per pre-transform chain (autograd runs through the chain's pre-transforms) and, for the slots outside
        the chains, from the same kernel on their projected coordinates or from ``_interp_torch`` when their centres are not
        uniform.

        Where ``log_prob`` is log(prob + pad) of an fp32 product — the constant log(pad) once a hundred factors have
        underflowed — this sums logarithms: finite and accurate wherever every factor is positive.  Outside the support the
        value is -inf and the gradient row 0 (nothing pulls such a point); a NaN coordinate gives NaN in both.  The derivative
        is that of the cell which holds the point: the right derivative at an interior bin centre, the left one at the last
        centre.  A table whose ``values`` require a gradient receives d / d values[e] = sum_n g_n rho_e(x_n) / values[e], the
        weighted histogram of the responsibilities rho (the share of the interpolant h that node e carries at the point, in
        [0, 1]) divided by the table; an entry that is not positive receives 0 (it is outside MENT's support and stays there, as
        under ``gauss_seidel_update``), a factor on the upper clamp is a constant, and rows outside the support pass nothing.
        That makes the MENT dual log Z(exp lambda) - sum g_hat Delta lambda an ordinary autograd objective in lambda = log
        values (examples/fit_ment_dual.py).  ``pad > 0`` returns logaddexp(log_density, log pad), which is log(prob + pad)
        wherever that is representable.  ``normalized=True`` subtracts the ``log_z`` that ``log_normalization`` stored (a
        ``RuntimeError`` if it has not run): the log of a density that integrates to 1, up to the error of that estimate, which
        does not follow later changes of the tables.  No host synchronisation: the call, and its backward, can be captured in a
        graph."""
        if normalized and getattr(self, "log_z", None) is None:
            raise RuntimeError("MENT.log_density(normalized=True): no log Z has been estimated yet; call log_normalization() first")
        chains, torch_slots = self._get_plan()
        x = x.to(torch.float32)
        prior = _prior_args(self.prior)
        total = None
        for chain in chains:
            xin = apply_pre(x, chain.pre) if chain.pre else x
            lp = ops.MentLogProbFn.apply(xin.contiguous(), chain.desc_t, chain.meta_t, self._tables(chain),
                                         prior if total is None else (0, 0.0, 0.0))
            total = lp if total is None else total + lp
        transported = {}
        for i, j in torch_slots:
            if i not in transported:
                transported[i] = self.transforms[i](x)
            lf = self.lagrange_functions[i][j]
            coords = lf.coord_list()
            u = self.diagnostics[i][j].project(transported[i]).reshape(x.shape[0], len(coords)).to(torch.float32)
            args = self._torch_slot_args(i, j)
            if args is not None:
                lp = ops.MentLogProbFn.apply(u.contiguous(), args[0], args[1],
                                             lf.values.to(u.device, torch.float32).reshape(-1).contiguous(), (0, 0.0, 0.0))
            else:
                h = _interp_torch(coords, lf.values, u)
                zero = h <= 0.0                            # outside the hull, a zero of the table (or a negative entry)
                top = h >= 1.0e10                          # on the upper clamp: a constant
                lp = torch.log(torch.where(zero | top, torch.ones_like(h), h))
                lp = torch.where(top, torch.full_like(h, math.log(1.0e10)), lp)
                lp = torch.where(zero, torch.full_like(h, float("-inf")), lp)
            total = total + lp
        # a row that any term puts outside the support takes no gradient through the terms that are finite there
        total = torch.where(torch.isneginf(total), torch.full_like(total, float("-inf")), total)
        if pad > 0.0:
            total = torch.logaddexp(total, torch.full_like(total, math.log(pad)))
        if normalized:
            total = total - self.log_z.to(total.device)
        return total

    def log_normalization(self, sampler: Optional[Callable] = None, **kws) -> dict:
        """Estimate the normaliser Z = integral of exp(log_density) by annealed importance sampling and return, as 0-dim fp64
        tensors on the device (no host synchronisation), with w_i = exp(logw_i) the weights of the C chains, w_bar their mean and
        wt_i = w_i / sum w:

          log_z        logsumexp(logw) - log C, the log of the unbiased estimate w_bar of Z;
          ess          (sum w)^2 / sum w^2, the effective number of chains (C for equal weights);
          log_z_se     sqrt(sum (w_i / w_bar - 1)^2) / C, the standard error of log_z by the delta method;
          entropy      log_z - sum wt_i log_density(x_i), the entropy -integral (p / Z) log (p / Z) of the normalised density from
                       the weighted final states (rows of weight 0 contribute 0);
          accept_rate  the share of accepted Langevin transitions.

        ``sampler`` is a :class:`mentflow_amd.sample.AnnealedImportanceSampler` (default: one built from ``**kws``, e.g.
        ``chains``, ``n_temps``, ``steps_per_temp``, ``step``, ``base_scale``, ``seed``).  ``log_z`` is stored as ``self.log_z``
        for ``log_density(normalized=True)``.  A :class:`mentflow_amd.sample.SequentialMonteCarloSampler` is passed as
        ``sampler``; its result carries ``log_z_groups``, the estimates of its G independent islands, and then ``log_z`` is
        logsumexp(log_z_groups) - log G and ``log_z_se`` is std(exp(log_z_groups - log_z), unbiased) / sqrt(G) (NaN for G = 1):
        the spread of independent estimates, valid however often the chains were resampled, which the delta method over chains
        is not.  ``ess`` and ``entropy`` come from the final weights as before.  Only a MENT whose slots all run through the kernels on plain LinearTransforms
        is supported: one with slots behind a pre-transform chain, or evaluated in torch, raises ``NotImplementedError``."""
        from .sample import AnnealedImportanceSampler
        if not self.fully_fused():
            raise NotImplementedError("MENT.log_normalization: this MENT has slots behind a pre-transform chain or evaluated in "
                                      "torch; only the single kernel chain of plain LinearTransforms is supported")
        if sampler is None:
            sampler = AnnealedImportanceSampler(self.ndim, device=self._device(), **kws)
        elif kws:
            raise TypeError("MENT.log_normalization: pass either a sampler or the arguments to build one, not both")
        res = sampler.run(self)
        logw, lp = res["logw"], res["logp"].double()
        chains = logw.numel()
        lse = torch.logsumexp(logw, 0)
        wt = torch.exp(logw - lse)                            # normalised weights: they sum to 1
        log_z = lse - math.log(chains)
        ess = 1.0 / (wt * wt).sum()
        log_z_se = torch.sqrt(((chains * wt - 1.0) ** 2).sum()) / chains
        if "log_z_groups" in res:                             # independent islands: their mean, and its error from their spread
            lzg = res["log_z_groups"]
            groups = lzg.numel()
            log_z = torch.logsumexp(lzg, 0) - math.log(groups)
            log_z_se = torch.exp(lzg - log_z).std(unbiased=True) / math.sqrt(groups) if groups > 1 else log_z * float("nan")
        entropy = log_z - torch.where(wt > 0, wt * lp, torch.zeros_like(wt)).sum()
        total = max(1, sampler.n_temps * sampler.steps_per_temp) * chains
        self.log_z = log_z
        return dict(log_z=log_z, ess=ess, log_z_se=log_z_se, entropy=entropy,
                    accept_rate=res["accepted"].sum().double() / float(total))

    def table_responsibilities(self, x: torch.Tensor, weights: Optional[torch.Tensor] = None) -> List[List[torch.Tensor]]:
        """sum_n w_n rho(x_n) per slot, in the shape of each table: rho is the share of the slot's interpolant that a node of
        the cell holding the point carries (1-D: a (1 - w) / h and b w / h; they sum to 1 per slot and point), so each result
        is the w-weighted soft histogram of the batch on the slot's centres.  ``weights`` [len(x)] defaults to 1 / len(x);
        rows outside the support contribute nothing.  This is the model-side term of the gradient of the MENT dual in the
        log-tables, for every slot from one batch.  One code path for every kind of slot: autograd of ``log_density`` on
        leaf copies of the tables, multiplied by the tables."""
        x = x.to(torch.float32)
        if weights is None:
            weights = torch.full((x.shape[0],), 1.0 / max(x.shape[0], 1), dtype=torch.float32, device=x.device)
        functions = [lf for group in self.lagrange_functions for lf in group]
        kept = [lf.values for lf in functions]
        leaves = [v.detach().to(torch.float32).clone().requires_grad_(True) for v in kept]
        try:
            for lf, leaf in zip(functions, leaves):
                lf.values = leaf
            with torch.enable_grad():
                lp = self.log_density(x.detach())
                total = (torch.where(torch.isneginf(lp), torch.zeros_like(lp), lp) * weights.to(lp.device, torch.float32)).sum()
                grads = torch.autograd.grad(total, leaves, allow_unused=True) if leaves else []
        finally:
            for lf, v in zip(functions, kept):
                lf.values = v
        flat = [torch.zeros_like(leaf) if g is None else g * leaf.detach() for g, leaf in zip(grads, leaves)]
        out, at = [], 0
        for group in self.lagrange_functions:
            out.append(flat[at:at + len(group)])
            at += len(group)
        return out

    def prob(self, x: torch.Tensor) -> torch.Tensor:
        chains, torch_slots = self._get_plan()
        x = x.to(torch.float32).contiguous()
        prior = _prior_args(self.prior)
        out = None
        for chain in chains:
            xin = apply_pre(x, chain.pre).contiguous() if chain.pre else x
            out = ops.ment_prob(xin, chain.desc_t, chain.meta_t, self._tables(chain), prior if out is None else (0, 0.0, 0.0),
                                out=out, multiply=out is not None)
        transported = {}
        for i, j in torch_slots:
            if i not in transported:
                transported[i] = self.transforms[i](x)
            h = self.evaluate_lagrange_function(transported[i], i, j)
            out = out * torch.clamp(h, 0.0, 1.00e10)
        return out

    def prob_on_grid(self, coords: List[torch.Tensor]):
        """(prob, block sums) on the implicit tensor grid of the cell centres `coords` (GridSampler's fast path), or None
        when a slot runs outside the kernels."""
        args = self.fused_args()
        if len(coords) != self.ndim or args is None:
            return None
        coords = [c.to(self._device(), torch.float32) for c in coords]
        return ops.ment_prob_grid(coords, *args)

    def fused_args(self):
        """(desc, meta, tables, prior args) of the one kernel chain whose product is exactly ``prob`` (what the implicit-grid
        and Metropolis-Hastings kernels take), or None when a slot runs outside the kernels."""
        if not self.fully_fused():
            return None
        chain = self._get_plan()[0][0]
        return chain.desc_t, chain.meta_t, self._tables(chain), _prior_args(self.prior)

    def sample(self, size: int) -> torch.Tensor:
        return self.send(self.sampler(self.prob, size))

    def _sample_for_simulation(self) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """(x, weights) of one sample-mode simulation: n_samples equal-weight rows (weights None), or with `weighted` the
        sampler's own states and their weights."""
        if not self.weighted:
            return self.send(self.sample(int(self.n_samples))), None
        self._check_weighted_sampler()                        # the sampler may have been replaced since the flag was set
        x, w = self.sampler.sample_weighted(self.prob, int(self.n_samples))
        return self.send(x), self.send(w)

    def sample_and_log_prob(self, size: int) -> Tuple[torch.Tensor, torch.Tensor]:
        x = self.sample(size)
        return x, self.log_prob(x)

    def discrepancy_vector(self, predictions: List[List[torch.Tensor]]) -> List[torch.Tensor]:
        return [self.discrepancy_function(pred, meas) for pred, meas in zip(unravel(predictions), unravel(self.measurements))]

    # ---------------------------------------------------------------------------------------------------- projections
    def _simulate_integrate(self, index: int, diag_index: int) -> torch.Tensor:
        diagnostic = self.diagnostics[index][diag_index]
        transform = self.transforms[index]
        if getattr(diagnostic, "direction", None) is not None:
            raise NotImplementedError("MENT integrate mode: a Histogram1D with a `direction` has no measurement axis to "
                                      "integrate around (use mode='sample')")
        meas_axis, int_axis = self._axes(index, diag_index)
        int_coords = self._integration_coords(index, diag_index)
        if isinstance(transform, LinearTransform) and self.fully_fused():
            chain = self._get_plan()[0][0]
            centres = [self.send(coords_from_edges(e)) for e in ([diagnostic.edges] if diagnostic.ndim == 1
                                                                  else diagnostic.edges)]
            axis_coords = [None] * self.ndim
            for a, c in zip(meas_axis, centres):
                axis_coords[a] = c
            for a, c in zip(int_axis, int_coords):
                axis_coords[a] = c
            prediction = ops.ment_integrate(transform.matrix_inv, axis_coords, meas_axis, chain.desc_t, chain.meta_t,
                                            self._tables(chain), _prior_args(self.prior))
        else:                    # any transform with an inverse: chunks of explicit points through prob()
            meas_points = self.send(self.get_meas_points(index, diag_index)).reshape(-1, len(meas_axis))
            int_points = self.get_integration_points(index, diag_index).reshape(-1, len(int_axis))
            nb, nt = meas_points.shape[0], int_points.shape[0]
            prediction = torch.zeros(nb, dtype=torch.float32, device=meas_points.device)
            per = max(1, _MAX_TORCH_ROWS // max(1, nt))
            for b0 in range(0, nb, per):
                b1 = min(nb, b0 + per)
                u = torch.zeros(b1 - b0, nt, self.ndim, dtype=torch.float32, device=meas_points.device)
                for k, a in enumerate(int_axis):
                    u[:, :, a] = int_points[None, :, k]
                for k, a in enumerate(meas_axis):
                    u[:, :, a] = meas_points[b0:b1, k][:, None]
                x = transform.inverse(u.reshape(-1, self.ndim))
                prediction[b0:b1] = self.prob(x).reshape(b1 - b0, nt).double().sum(1).float()
        if diagnostic.ndim > 1:
            prediction = prediction.reshape(diagnostic.shape)
        return self.normalize_projection(self.send(prediction), index, diag_index)

    def _simulate_sample(self, index: int, diag_index: int) -> torch.Tensor:
        x, weights = self._sample_for_simulation()
        diagnostic = self.diagnostics[index][diag_index]
        prediction = None
        for chain in self._get_plan()[0]:
            if (index, diag_index) in chain.slots:
                rows = chain.rows[chain.slots.index((index, diag_index))]
                xin = apply_pre(x, chain.pre) if chain.pre else x
                prediction = diagnostic._apply_noise(diagnostic.batched(xin, [r[None, :].to(x) for r in rows], weights)[0])
        if prediction is None:
            if weights is not None and not isinstance(diagnostic, Histogram):
                raise NotImplementedError(
                    f"weighted simulation: {type(diagnostic).__name__} (measurement [{index}][{diag_index}]) takes no particle "
                    "weights; histogram diagnostics do (Histogram1D / Histogram2D)")
            u = self.transforms[index](x)
            prediction = diagnostic(u) if weights is None else diagnostic(u, weights)
        return self.normalize_projection(prediction, index, diag_index)

    def simulate(self, index: int, diag_index: int, **kws) -> torch.Tensor:
        if self.mode == "integrate":
            return self._simulate_integrate(index, diag_index, **kws)
        elif self.mode == "sample":
            return self._simulate_sample(index, diag_index, **kws)
        raise ValueError(f"Invalide mode {self.mode}")

    def gauss_seidel_update(self, lr: float = 1.0, thresh: float = 1.0e-10, **kws) -> None:
        """Gauss-Seidel relaxation: every slot in turn is re-simulated with the tables updated so far, then
        h <- h * (1 + lr * (g / g* - 1)) where g != 0 and g* != 0 (g* < thresh counts as 0)."""
        for index in range(len(self.transforms)):
            if self.verbose:
                print(f"index={index}")
            for diag_index in range(len(self.diagnostics[index])):
                lagrange_function = self.lagrange_functions[index][diag_index]
                measurement = self.measurements[index][diag_index]
                prediction = self.simulate(index, diag_index, **kws)
                prediction = torch.where(prediction < thresh, torch.zeros_like(prediction), prediction)
                values = lagrange_function.values
                meas = measurement.to(values.device).reshape(values.shape)
                pred = prediction.to(values.device).reshape(values.shape)
                updated = values * (1.0 + lr * ((meas / pred) - 1.0))
                lagrange_function.set_values(torch.where((meas != 0.0) & (pred != 0.0), updated, values))
        self.epoch += 1

    def simulate_all(self, **kws) -> List[List[torch.Tensor]]:
        predictions = []
        if self.mode == "integrate":
            for index in range(len(self.transforms)):
                predictions.append([self._simulate_integrate(index, j, **kws) for j in range(len(self.diagnostics[index]))])
        elif self.mode == "sample":
            x, weights = self._sample_for_simulation()
            predictions = forward(x, self.transforms, self.diagnostics, weights)
        return predictions

    # ---------------------------------------------------------------------------------------------------- state
    def save(self, path: str) -> None:
        state = {"lagrange_functions": self.lagrange_functions, "epoch": self.epoch, "transforms": self.transforms,
                 "diagnostics": self.diagnostics, "measurements": self.measurements, "prior": self.prior,
                 "ndim": self.ndim, "sampler": self.sampler, "weighted": self.weighted}
        torch.save(state, path)

    def load(self, path: str, device: torch.device = None) -> None:
        state = torch.load(path, map_location=device, weights_only=False)
        self.lagrange_functions = state["lagrange_functions"]
        self.epoch = state["epoch"]
        self.transforms = state["transforms"]
        self.diagnostics = state["diagnostics"]
        self.measurements = state["measurements"]
        self.prior = state["prior"]
        self.ndim = state["ndim"]
        self.sampler = state["sampler"]
        self.weighted = bool(state.get("weighted", False))     # after the sampler: the setter checks it
        self._plan = None
        self.to(device)

    def to(self, device):
        self.device = device
        self._plan = None
        if self.transforms is not None:
            for i in range(len(self.transforms)):
                self.transforms[i] = self.transforms[i].to(device)
        if self.diagnostics is not None:
            for i in range(len(self.diagnostics)):
                for j in range(len(self.diagnostics[i])):
                    self.diagnostics[i][j] = self.diagnostics[i][j].to(device)
        if self.measurements is not None:
            for i in range(len(self.measurements)):
                for j in range(len(self.measurements[i])):
                    self.measurements[i][j] = self.measurements[i][j].to(device)
        if self.sampler is not None:
            self.sampler = self.sampler.to(device)
        if self.prior is not None:
            self.prior = self.prior.to(device)
        for i in range(len(self.lagrange_functions)):
            for j in range(len(self.lagrange_functions[i])):
                lf = self.lagrange_functions[i][j]
                lf.values = self.send(lf.values)
                lf.coords = self.send(lf.coords) if torch.is_tensor(lf.coords) else [self.send(c) for c in lf.coords]
        return self
