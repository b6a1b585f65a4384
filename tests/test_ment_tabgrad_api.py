"""The table gradient through the public interface: ops.MentLogProbFn differentiable in x and tables together, MENT.log_density
filling the gradient of every Lagrange table on each of its three paths (the kernel chains, the kernel on the projected
coordinates of a slot outside the chains, _interp_torch on a grid that is not uniform), MENT.table_responsibilities, and the dual
descent of examples/fit_ment_dual.py against the same loop in fp64 torch.  Emulator here, MI355X with -m gpu.  The kernel's
numbers are gated in tests/test_ment_tabgrad_kernels.py."""
import math
import os
import sys

import pytest
import torch

import mentflow_amd as mf
from _ment_fp64 import interp64
from mentflow_amd import ops
from mentflow_amd.ment import MENT, UniformPrior
from test_ment_logp_kernels import MIXED8, make_slots

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import fit_ment_dual as example          # noqa: E402


def test_function_gives_gradients_to_x_and_tables_together(backend):
    d = 3
    gen = torch.Generator().manual_seed(2)
    slots, desc, meta, tab = make_slots(d, MIXED8[:4], gen)
    desc, meta, tab = desc.to(backend), meta.to(backend), tab.to(backend)
    x = (1.2 * torch.randn(700, d, generator=gen)).to(backend)
    x[5, 0] = 30.0                                                   # outside the support: -inf
    prior = (1, 1.5, -1.0)
    g = torch.randn(700, generator=gen).to(backend)
    g[5] = float("inf")                                              # a non-finite incoming gradient at a -inf row
    xr = x.clone().requires_grad_(True)
    lp_old = ops.MentLogProbFn.apply(xr, desc, meta, tab, prior)
    (gx_old,) = torch.autograd.grad(lp_old, xr, g)
    tr = tab.clone().requires_grad_(True)
    lp = ops.MentLogProbFn.apply(xr, desc, meta, tr, prior)
    assert torch.equal(lp.detach(), lp_old.detach()) and torch.isneginf(lp[5])
    gx, gt = torch.autograd.grad(lp, (xr, tr), g)
    assert torch.equal(gx, gx_old), "the x gradient is bitwise what it is without the table gradient"
    want = ops.ment_logprob_table_grad(x, desc, meta, tab, lp.detach(), g)[1]
    assert torch.equal(gt, want) and gt.shape == tab.shape and torch.isfinite(gt).all() and float(gt.abs().max()) > 0
    # tables alone
    lp = ops.MentLogProbFn.apply(x, desc, meta, tr, prior)
    assert lp.requires_grad
    assert torch.equal(torch.autograd.grad(lp, tr, g)[0], want)
    # a shaped table keeps its shape
    t2 = tab.clone().reshape(1, -1).requires_grad_(True)
    (g2,) = torch.autograd.grad(ops.MentLogProbFn.apply(x, desc, meta, t2, prior), t2, g)
    assert g2.shape == t2.shape and torch.equal(g2.reshape(-1), want)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gr = g.clone().requires_grad_(True)
        (gt,) = torch.autograd.grad(ops.MentLogProbFn.apply(x, desc, meta, tr, prior), tr, gr, create_graph=True)
        gt.sum().backward()


def test_tables_without_requires_grad_take_the_old_path(backend, monkeypatch):
    d = 2
    gen = torch.Generator().manual_seed(4)
    slots, desc, meta, tab = make_slots(d, MIXED8[:3], gen)
    desc, meta, tab = desc.to(backend), meta.to(backend), tab.to(backend)
    x = (1.2 * torch.randn(300, d, generator=gen)).to(backend)
    lp0, grad = ops.ment_logprob(x, desc, meta, tab, want_grad=True)
    calls = []
    real = ops.ment_logprob
    monkeypatch.setattr(ops, "ment_logprob_table_grad", lambda *a, **k: pytest.fail("the table kernel must not be launched"))
    monkeypatch.setattr(ops, "ment_logprob", lambda *a, **k: calls.append(k.get("want_grad")) or real(*a, **k))
    xr = x.clone().requires_grad_(True)
    lp = ops.MentLogProbFn.apply(xr, desc, meta, tab, (0, 0.0, 0.0))
    assert len(lp.grad_fn.saved_tensors) == 2, "gradient rows and logp, as before"
    lp.sum().backward()
    assert calls == [True] and torch.equal(lp.detach(), lp0)
    assert torch.equal(xr.grad, torch.where(torch.isneginf(lp0)[:, None], torch.zeros_like(grad), grad))
    assert not ops.MentLogProbFn.apply(x, desc, meta, tab, (0, 0.0, 0.0)).requires_grad


class Cubic:
    """A transform MENT cannot split into pre-transforms and a matrix: its slot is evaluated on its projected coordinates."""

    def __call__(self, x):
        return x + 0.05 * x ** 3

    def to(self, device):
        return self


def every_route_model(backend):
    """4-D (x, px, y, py) with py ~ 1000.  The plain chain (identity transport: a kernel slot on x, a torch slot on py with the
    offset grid [997, 1003], whose fp32 centres are not uniform), a multipole + rotation pre-chain, and a transform outside the
    chains whose slot has uniform centres (the kernel on its projected coordinates, identity rows)."""
    gen = torch.Generator().manual_seed(12)
    blocks = torch.block_diag(mf.simulate.rotation_matrix(math.radians(60.0)).float(),
                              mf.simulate.rotation_matrix(math.radians(30.0)).float())
    chain = mf.simulate.CompositeTransform(mf.simulate.MultipoleTransform(order=3, strength=0.6), mf.simulate.LinearTransform(blocks))
    transforms = [mf.simulate.LinearTransform(torch.eye(4)).to(backend), chain.to(backend), Cubic()]
    wide = lambda axis: mf.diagnostics.Histogram1D(axis=axis, edges=torch.linspace(-5.0, 5.0, 41)).to(backend)
    offset = mf.diagnostics.Histogram1D(axis=3, edges=torch.linspace(997.0, 1003.0, 31)).to(backend)
    diagnostics = [[wide(0), offset], [wide(0), wide(2)], [wide(2)]]
    meas = [[torch.ones(d.edges.numel() - 1).to(backend) for d in ds] for ds in diagnostics]
    model = MENT(ndim=4, transforms=transforms, diagnostics=diagnostics, measurements=meas,
                 prior=UniformPrior(ndim=4, scale=2000.0), mode="sample", device=backend)
    for lf in mf.utils.unravel(model.lagrange_functions):
        lf.set_values((0.25 + 1.75 * torch.rand(lf.values.shape, generator=gen)).to(backend).requires_grad_(True))
    return model


def every_route_points(backend):
    x = torch.randn(3001, 4, generator=torch.Generator().manual_seed(3))
    x[:, 3] = 1000.0 + 1.4 * x[:, 3]
    return x.to(backend)


def test_log_density_backward_fills_the_gradient_of_every_table(backend):
    """This is the test that fails without the table gradient.  Per 1-D slot the responsibilities of a live point sum to 1, so
    sum_e grad[e] values[e] = sum of the upstream weights over the live rows, on every path."""
    model = every_route_model(backend)
    chains, torch_slots = model._get_plan()
    assert len(chains) == 2 and torch_slots == [(0, 1), (2, 0)]
    assert model._torch_slot_args(0, 1) is None and model._torch_slot_args(2, 0) is not None
    x = every_route_points(backend)
    w = torch.randn(3001, generator=torch.Generator().manual_seed(5)).to(backend)
    ld = model.log_density(x)
    live = torch.isfinite(ld)
    assert 2000 < int(live.sum()) < 3001 and not torch.isnan(ld).any()
    (torch.where(live, ld, torch.zeros_like(ld)) * w).sum().backward()
    total, scale = float(w[live].double().sum()), float(w[live].abs().double().sum())
    for lf in mf.utils.unravel(model.lagrange_functions):
        assert lf.values.grad is not None and lf.values.grad.shape == lf.values.shape
        assert torch.isfinite(lf.values.grad).all() and float(lf.values.grad.abs().max()) > 0
        got = float((lf.values.grad.double() * lf.values.detach().double()).sum())
        assert abs(got - total) <= 1e-5 * scale, (got, total)


def test_table_responsibilities(backend):
    model = every_route_model(backend)
    x = every_route_points(backend)
    live = torch.isfinite(model.log_density(x).detach())
    kept = [lf.values for lf in mf.utils.unravel(model.lagrange_functions)]
    resp = model.table_responsibilities(x)
    assert [len(r) for r in resp] == [2, 2, 1]
    assert all(lf.values is v and v.grad is None for lf, v in zip(mf.utils.unravel(model.lagrange_functions), kept))
    share = float(live.double().mean())
    for r, lf in zip(mf.utils.unravel(resp), mf.utils.unravel(model.lagrange_functions)):
        assert r.shape == lf.values.shape and not r.requires_grad and (r >= 0).all()
        assert abs(float(r.double().sum()) - share) <= 1e-5
    # weights, and the autograd route spelt out
    w = torch.rand(3001, generator=torch.Generator().manual_seed(9)).to(backend)
    resp = mf.utils.unravel(model.table_responsibilities(x, w))
    ld = model.log_density(x)
    (torch.where(torch.isneginf(ld), torch.zeros_like(ld), ld) * w).sum().backward()
    for r, lf in zip(resp, mf.utils.unravel(model.lagrange_functions)):
        assert torch.equal(r, lf.values.grad * lf.values.detach())
        assert abs(float(r.double().sum()) - float(w[live].double().sum())) <= 1e-5 * float(w[live].sum())


# ------------------------------------------------------------------------------------------------------- the dual descent
def density64(x, rows, coords, tables, prior_scale):
    """fp64 log-density of the example's model (tests/_ment_fp64.interp64): -inf outside the support."""
    total = -(x * x).sum(1) / (2.0 * prior_scale ** 2) - 2.0 * (math.log(prior_scale) + 0.5 * math.log(2.0 * math.pi))
    dead = torch.zeros(x.shape[0], dtype=torch.bool)
    for r, t in zip(rows, tables):
        h = interp64([coords], t, (x @ r)[:, None])
        zero = h <= 0.0
        dead |= zero.detach()
        total = total + torch.log(torch.where(zero, torch.ones_like(h), h))
    return torch.where(dead, torch.full_like(total, float("-inf")), total)


def discrepancy64(rows, mats, coords, tables, targets, prior_scale, xmax, resolution=129):
    """Mean absolute difference between the measured projections and the fp64 line integrals of the density through the bin
    centres (what MENT's integrate mode computes)."""
    t = torch.linspace(-xmax, xmax, resolution, dtype=torch.float64)
    out = []
    for m, target in zip(mats, targets):
        u = torch.stack(torch.meshgrid(coords, t, indexing="ij"), dim=-1).reshape(-1, 2)
        p = torch.exp(density64(u @ m, rows, coords, tables, prior_scale)).reshape(coords.numel(), resolution).sum(1)
        out.append((p / p.sum() / (coords[1] - coords[0]) - target).abs().mean())
    return float(torch.stack(out).mean())


def test_dual_descent_follows_the_fp64_loop(backend):
    """The example's loop (128^2 grid, 50 Adam steps at lr 0.1) on the library against the same loop in fp64 torch on the CPU.  Both
    follow the same Adam trajectory: the library's final mean discrepancy must be <= 2 x the fp64 loop's (2 x covers fp32 tables)
    and <= 0.1 x the initial one (fp64 measured 0.025 x)."""
    xmax, steps, lr, n, prior_scale = 4.0, 50, 0.1, 128, 2.0
    model = example.build_model(backend, xmax=xmax, prior_scale=prior_scale)
    grid, cell = example.grid_points(backend, xmax, n)
    example.dual_descent(model, grid, cell, steps, lr)
    lib_tables = [lf.values.detach().double().cpu() for lf in mf.utils.unravel(model.lagrange_functions)]

    mats = [t.matrix.double().cpu() for t in model.transforms]
    rows = [m[0] for m in mats]
    coords = model.lagrange_functions[0][0].coord_list()[0].double().cpu()
    targets = [m.double().cpu() for m in mf.utils.unravel(model.measurements)]
    width = float(model.diagnostics[0][0].edges[1] - model.diagnostics[0][0].edges[0])
    support = [(t > 0).double() for t in targets]
    grid64 = grid.double().cpu()
    lam = [torch.zeros_like(t, requires_grad=True) for t in targets]
    opt = torch.optim.Adam(lam, lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        lp = density64(grid64, rows, coords, [torch.exp(l) * s for l, s in zip(lam, support)], prior_scale)
        dual = torch.logsumexp(lp[torch.isfinite(lp)], dim=0) + math.log(cell) - sum((t * width * l).sum() for t, l in zip(targets, lam))
        dual.backward()
        opt.step()
    ref_tables = [(torch.exp(l) * s).detach() for l, s in zip(lam, support)]

    args = (rows, mats, coords)
    first = discrepancy64(*args, support, targets, prior_scale, xmax)
    lib = discrepancy64(*args, lib_tables, targets, prior_scale, xmax)
    ref = discrepancy64(*args, ref_tables, targets, prior_scale, xmax)
    print({"initial": first, "library": lib, "fp64": ref, "library (integrate mode)": example.mean_discrepancy(model)})
    assert lib <= 2.0 * ref
    assert lib <= 0.1 * first
