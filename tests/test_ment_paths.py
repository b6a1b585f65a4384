"""Classical MENT's routes below the public API, each against an fp64 evaluation of the same density: pre-transform chains
(one multiply-mode launch per chain, ``apply_pre`` in sample mode), slots evaluated in torch (non-uniform centres), the chunked
``transform.inverse`` route of integrate mode, and GridSampler's choice of the implicit-grid kernel.  Emulator here, MI355X
with -m gpu.  Gates as in test_ment_kernels.py: 3e-5 of the largest fp64 value for products of a few fp32 factors."""
import math

import numpy as np
import pytest
import torch

import mentflow_amd as mf
from _ment_fp64 import interp64
from mentflow_amd import ops
from mentflow_amd.ment import MENT, LagrangeFunction
from mentflow_amd.sample import GridSampler
from mentflow_amd.utils import coords_from_edges


def rot(deg):
    return mf.simulate.LinearTransform(mf.simulate.rotation_matrix(math.radians(deg)).float())


def kick_chain(strength, deg):
    return mf.simulate.CompositeTransform(mf.simulate.MultipoleTransform(order=3, strength=strength), rot(deg))


def prob64(model, x):
    """prod_ij clamp(h_ij(project_j(T_i x))) * prior, with T_i applied as the model's own transforms (fp32) and h in fp64."""
    p = torch.ones(x.shape[0], dtype=torch.float64)
    for i, t in enumerate(model.transforms):
        u = t(x)
        for j, diag in enumerate(model.diagnostics[i]):
            lf = model.lagrange_functions[i][j]
            up = diag.project(u).reshape(x.shape[0], -1).cpu()
            p = p * interp64(lf.coord_list(), lf.values.cpu(), up).clamp(0.0, 1e10)
    s = model.prior.scale
    xd = x.double().cpu()
    return p * torch.exp(-x.shape[1] * (math.log(s) + 0.5 * math.log(2 * math.pi)) - 0.5 * (xd * xd).sum(1) / s ** 2)


def chain_model(backend, mode="sample", sampler=None, torch_slot=True):
    """2-D: a plain rotation, two kick + rotation chains, and (torch_slot) a second diagnostic with non-uniform edges."""
    gen = torch.Generator().manual_seed(4)
    transforms = [rot(0.0), kick_chain(0.6, 60.0), kick_chain(-0.6, 120.0)]
    uni = mf.diagnostics.Histogram1D(axis=0, edges=torch.linspace(-3.0, 3.0, 31)).to(backend)
    diagnostics = [[uni] for _ in transforms]
    if torch_slot:
        graded = torch.tensor(np.sinh(np.linspace(-1.8, 1.8, 26)), dtype=torch.float32)
        diagnostics[0].append(mf.diagnostics.Histogram1D(axis=0, edges=graded).to(backend))
    meas = [[torch.ones(d.edges.numel() - 1).to(backend) for d in ds] for ds in diagnostics]
    model = MENT(ndim=2, transforms=[t.to(backend) for t in transforms], diagnostics=diagnostics, measurements=meas,
                 prior=mf.prior.Gaussian(ndim=2, scale=2.0), mode=mode, sampler=sampler, n_samples=20000,
                 integration_limits=[[[(-3.0, 3.0)] for _ in ds] for ds in diagnostics],
                 integration_shape=[[[90] for _ in ds] for ds in diagnostics], device=backend)
    for lf in mf.utils.unravel(model.lagrange_functions):
        lf.set_values((0.3 + 1.4 * torch.rand(lf.values.shape, generator=gen)).to(backend))
    return model


def test_prob_with_chains_and_torch_slots(backend):
    model = chain_model(backend)
    chains, torch_slots = model._get_plan()
    assert len(chains) == 3 and torch_slots == [(0, 1)] and not model.fully_fused()
    x = (torch.randn(3000, 2, generator=torch.Generator().manual_seed(1)) * 1.2).to(backend)
    got = model.prob(x).cpu().double()
    ref = prob64(model, x)
    assert float(ref.max()) > 0
    assert float((got - ref).abs().max()) <= 3e-5 * float(ref.max())


class FixedSampler:
    def __init__(self, x):
        self.x = x

    def __call__(self, prob_func, size):
        return self.x[:size]

    def to(self, device):
        return self


def test_sample_mode_applies_the_pre_transforms(backend):
    x = (torch.randn(20000, 2, generator=torch.Generator().manual_seed(2)) * 0.9).to(backend)
    model = chain_model(backend, sampler=FixedSampler(x))
    for i in range(3):
        got = model.simulate(i, 0)
        diag = model.diagnostics[i][0]
        want = model.normalize_projection(diag(model.transforms[i](x)), i, 0)
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-6 * float(want.max()))
    torch_slot = model.simulate(0, 1)                                   # the generic route of a non-uniform diagnostic
    assert torch.allclose(torch_slot, model.normalize_projection(model.diagnostics[0][1](x), 0, 1), rtol=1e-5, atol=1e-7)


def integrate64(model, i, j):
    diag = model.diagnostics[i][j]
    c = coords_from_edges(diag.edges).to(model._device())
    g = torch.linspace(-3.0, 3.0, 90).to(model._device())
    u = torch.stack([c[:, None].expand(-1, 90).reshape(-1), g[None, :].expand(c.numel(), -1).reshape(-1)], 1)
    x = model.transforms[i].inverse(u)
    p = prob64(model, x).reshape(c.numel(), 90).sum(1)
    return p / p.sum() / float(diag.edges[1] - diag.edges[0])


def test_integrate_through_transform_inverse(backend, monkeypatch):
    """Kick chains have no affine inverse: integrate mode evaluates explicit points x = T^-1 u through prob(), in chunks of
    bins (made small here so that several chunks run)."""
    monkeypatch.setattr(mf.ment, "_MAX_TORCH_ROWS", 1000)
    model = chain_model(backend, mode="integrate", torch_slot=False)
    for i in range(3):
        got = model.simulate(i, 0).cpu().double()
        ref = integrate64(model, i, 0).cpu()
        assert float((got - ref).abs().max()) <= 3e-5 * float(ref.max())


def test_integrate_kernel_and_chunked_route_agree(backend, monkeypatch):
    """The same rotation as a plain LinearTransform (integrate kernel) and wrapped in a CompositeTransform (chunked route)."""
    monkeypatch.setattr(mf.ment, "_MAX_TORCH_ROWS", 2000)
    preds = []
    for wrap in (False, True):
        t = rot(35.0)
        t = mf.simulate.CompositeTransform(t) if wrap else t
        diag = mf.diagnostics.Histogram1D(axis=0, edges=torch.linspace(-3.0, 3.0, 41)).to(backend)
        model = MENT(ndim=2, transforms=[t.to(backend), rot(100.0).to(backend)], diagnostics=[[diag], [diag]],
                     measurements=[[torch.ones(40).to(backend)], [torch.ones(40).to(backend)]],
                     prior=mf.prior.Gaussian(ndim=2, scale=1.5), mode="integrate",
                     integration_limits=[[[(-3.0, 3.0)]]] * 2, integration_shape=[[[300]]] * 2, device=backend)
        gen = torch.Generator().manual_seed(9)
        for lf in mf.utils.unravel(model.lagrange_functions):
            lf.set_values((0.2 + torch.rand(40, generator=gen)).to(backend))
        preds.append(model.simulate(0, 0).cpu())
    assert float((preds[0] - preds[1]).abs().max()) <= 3e-5 * float(preds[0].max())


def test_grid_sampler_takes_the_kernel_for_ment_prob_only(backend, monkeypatch):
    """MENT.prob itself runs on the implicit grid; an override of prob in a subclass is sampled as given."""
    x = torch.zeros(1)
    model = chain_model(backend, torch_slot=False)
    model.transforms = [rot(0.0).to(backend), rot(70.0).to(backend), rot(140.0).to(backend)]
    model._plan = None
    sampler = GridSampler(limits=[(-3.0, 3.0)] * 2, shape=(20, 20)).to(backend)
    calls = []
    real = ops.ment_prob_grid
    monkeypatch.setattr(ops, "ment_prob_grid", lambda *a, **k: calls.append(1) or real(*a, **k))
    torch.manual_seed(0)
    x = sampler(model.prob, 4000)
    assert calls == [1] and x.shape == (4000, 2)

    class HalfPlane(MENT):
        def prob(self, x):
            return super().prob(x) * (x[:, 0] > 0).float()

    half = chain_model(backend, torch_slot=False)
    half.__class__ = HalfPlane
    torch.manual_seed(0)
    y = sampler(half.prob, 4000)
    assert calls == [1]                                        # not the implicit-grid kernel
    assert bool((y[:, 0] > 0).all())


def test_lagrange_function_clamps_on_every_grid(backend):
    v = torch.tensor([1.0, -2.0, 0.5, 3.0]).to(backend)
    u = torch.tensor([-1.0, -0.5, 0.2, 1.0]).to(backend)
    even = LagrangeFunction(torch.tensor([-1.0, -1.0 / 3, 1.0 / 3, 1.0]).to(backend), v)
    graded = LagrangeFunction(torch.tensor([-1.0, -0.6, 0.4, 1.0]).to(backend), v)
    assert even.uniform() and not graded.uniform()
    for lf in (even, graded):
        h = lf(u).cpu()
        assert bool((h >= 0).all()) and float(h[0]) == 1.0 and float(h[-1]) == 3.0
        assert float(h[1]) == 0.0                                # the interpolant is negative there


def test_more_than_eight_dimensions_raise():
    diag = mf.diagnostics.Histogram1D(axis=0, edges=torch.linspace(-1, 1, 5))
    with pytest.raises(NotImplementedError, match="ndim=9"):
        MENT(ndim=9, transforms=[mf.simulate.LinearTransform(torch.eye(9))], diagnostics=[[diag]],
             measurements=[[torch.ones(4)]])
