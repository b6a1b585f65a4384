#!/usr/bin/env python
"""Fit classical MENT by descent on its dual on one MI355X: the usage document of the table gradient of `MENT.log_density`
(mentflow_amd/csrc/ment_tabgrad.hip).

The MENT density is p(x) = prior(x) prod_s h_s(u_s(x)) / Z.  With lambda_s = log h_s on the bin centres, g_hat_s the measured
(normalised) projections and Delta_s the bin widths, the Lagrange functions that reproduce the measurements minimise the convex

    F(lambda) = log Z(exp lambda) - sum_s sum_b g_hat_s[b] Delta_s lambda_s[b],

whose gradient is (model responsibilities) - (measured bin masses).  `gauss_seidel_update` reaches that point by simulating one
slot at a time; here one backward through `log_density` gives the gradient for EVERY slot from a single grid batch, and Adam does
the rest.  log Z is logsumexp of `log_density` on a regular grid (rows at -inf, outside the support, are dropped).

A 2-D two-Gaussian mixture, six 1-D projections of 32 bins.  The integrate-mode mean absolute discrepancy of the projections is
printed next to that of the same number of Gauss-Seidel epochs.

    python examples/fit_ment_dual.py
    python examples/fit_ment_dual.py --steps 300 --grid 256
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mentflow_amd as mf                                    # noqa: E402
from mentflow_amd.loss import mean_absolute_error            # noqa: E402
from mentflow_amd.ment import MENT                           # noqa: E402

MIXTURE = ((0.6, (-0.9, 0.5), 0.55), (0.4, (1.0, -0.6), 0.75))     # (weight, mean, isotropic sigma)


def mixture_projection(row: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
    """The mixture's exact projection along `row` (unit length), integrated over the bins and normalised as a density."""
    edges = edges.double()
    mass = torch.zeros(edges.numel() - 1, dtype=torch.float64)
    for weight, mean, sigma in MIXTURE:
        m = float(row[0]) * mean[0] + float(row[1]) * mean[1]
        cdf = 0.5 * (1.0 + torch.special.erf((edges - m) / (sigma * math.sqrt(2.0))))
        mass += weight * (cdf[1:] - cdf[:-1])
    return mass / mass.sum() / (edges[1] - edges[0])


def build_model(dev, views: int = 6, bins: int = 32, xmax: float = 4.0, prior_scale: float = 2.0, resolution: int = 129) -> MENT:
    """A MENT in integrate mode on `views` rotated 1-D projections of the mixture, its tables at their initial values."""
    edges = torch.linspace(-xmax, xmax, bins + 1)
    transforms, measurements = [], []
    for k in range(views):
        matrix = mf.simulate.rotation_matrix(math.pi * k / views).float()
        transforms.append(mf.simulate.LinearTransform(matrix).to(dev))
        measurements.append([mixture_projection(matrix[0], edges).float().to(dev)])
    diagnostics = [[mf.diagnostics.Histogram1D(axis=0, edges=edges).to(dev)] for _ in transforms]
    return MENT(ndim=2, transforms=transforms, diagnostics=diagnostics, measurements=measurements,
                discrepancy_function=mean_absolute_error, prior=mf.prior.Gaussian(ndim=2, scale=prior_scale), mode="integrate",
                integration_limits=[[[(-xmax, xmax)]] for _ in transforms], integration_shape=[[[resolution]] for _ in transforms],
                device=dev)


def grid_points(dev, xmax: float, n: int):
    """(points [n * n, 2], cell volume) of the regular grid on which log Z is summed."""
    c = torch.linspace(-xmax, xmax, n)
    return torch.stack(torch.meshgrid(c, c, indexing="ij"), dim=-1).reshape(-1, 2).to(dev), (2.0 * xmax / (n - 1)) ** 2


def mean_discrepancy(model: MENT) -> float:
    with torch.no_grad():
        return float(torch.stack([d.float() for d in model.discrepancy_vector(model.simulate_all())]).mean())


def dual_descent(model: MENT, grid: torch.Tensor, cell: float, steps: int, lr: float = 0.1, report=None):
    """Adam on the dual in lambda = log tables; the tables are set through set_values(exp(lambda) * support), where support marks
    the bins the measurement fills (an empty bin keeps a zero table, as under the multiplicative update).  Returns the lambdas."""
    functions = [lf for group in model.lagrange_functions for lf in group]
    targets = [m for group in model.measurements for m in group]
    widths = [float(d.edges[1] - d.edges[0]) for group in model.diagnostics for d in group]
    support = [(t > 0.0).float() for t in targets]
    lam = [torch.zeros_like(t, requires_grad=True) for t in targets]
    opt = torch.optim.Adam(lam, lr=lr)
    for step in range(steps):
        opt.zero_grad()
        for lf, l, s in zip(functions, lam, support):
            lf.set_values(torch.exp(l) * s)
        lp = model.log_density(grid)
        log_z = torch.logsumexp(lp[torch.isfinite(lp)], dim=0) + math.log(cell)
        dual = log_z - sum((t * w * l).sum() for t, w, l in zip(targets, widths, lam))
        dual.backward()
        opt.step()
        if report is not None:
            report(step, float(dual.detach()))
    with torch.no_grad():
        for lf, l, s in zip(functions, lam, support):
            lf.set_values(torch.exp(l) * s)
    return lam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--lr", type=float, default=0.1)
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    xmax = 4.0
    model = build_model(dev, xmax=xmax)
    print(f"initial tables: mean |projection - measurement| = {mean_discrepancy(model):.3e}")
    grid, cell = grid_points(dev, xmax, args.grid)
    t0 = time.time()
    dual_descent(model, grid, cell, args.steps, args.lr,
                 report=lambda step, f: print(f"step {step:4d}  dual {f:.6f}") if step % 10 == 0 else None)
    torch.cuda.synchronize()
    t_dual = time.time() - t0
    print(f"dual descent, {args.steps} steps on a {args.grid}^2 grid ({t_dual:.2f} s): "
          f"mean |projection - measurement| = {mean_discrepancy(model):.3e}")

    other = build_model(dev, xmax=xmax)
    t0 = time.time()
    for _ in range(args.steps):
        other.gauss_seidel_update(lr=1.0)
    torch.cuda.synchronize()
    print(f"gauss_seidel_update, {args.steps} epochs ({time.time() - t0:.2f} s): "
          f"mean |projection - measurement| = {mean_discrepancy(other):.3e}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
