"""prior.MENTPrior in MonteCarloEntropyEstimator and MENTFlow.loss: a classical MENT reconstruction as the prior of MENT-Flow.
Emulator here, MI355X with -m gpu (the `backend` fixture); the data-parallel case runs 2 gloo ranks on the emulator.

Bounds.  Estimator level: MENTPrior over a MENT without measurement slots and with a Gaussian prior of scale a IS that Gaussian,
evaluated per point in fp32 by the log-density kernel (<= 6 roundings per term: the squares' sum, the scaling, the constant) in
front of the shared fp64 sum, where the Gaussian route reduces sum |x|^2 in fp64 and scales once: |dH| <= 1e-5 at |H| ~ 5, and
the gradients -x / a^2 / N agree to 1e-6 relative elementwise.  Loss level: the same fp32 terms enter the fixed-order fp64
reduction of the loss and a hand-made fp64 mean: 1e-6 relative."""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mentflow_amd as mf
from conftest import EMU_LIB
from mentflow_amd import ops
from mentflow_amd.entropy import MonteCarloEntropyEstimator
from mentflow_amd.ment import MENT, UniformPrior
from mentflow_amd.prior import Gaussian, MENTPrior

PAD = 1.0e-12


def rot(deg):
    return mf.simulate.LinearTransform(mf.simulate.rotation_matrix(math.radians(deg)).float())


def ment_2d(device, views=4, bins=40):
    """A 2-D, 4-view MENT (Gaussian prior of scale 3) with smooth positive Lagrange functions on [-4, 4]."""
    gen = torch.Generator().manual_seed(33)
    transforms = [rot(180.0 * k / views).to(device) for k in range(views)]
    diag = mf.diagnostics.Histogram1D(axis=0, edges=torch.linspace(-4.0, 4.0, bins + 1)).to(device)
    model = MENT(ndim=2, transforms=transforms, diagnostics=[[diag] for _ in transforms],
                 measurements=[[torch.ones(bins).to(device)] for _ in transforms], prior=Gaussian(ndim=2, scale=3.0),
                 mode="sample", device=device)
    c = mf.utils.coords_from_edges(diag.edges.cpu())
    for lf in mf.utils.unravel(model.lagrange_functions):
        lf.set_values((torch.exp(-c ** 2 / (2 * 0.8 ** 2)) * (0.8 + 0.4 * torch.rand(bins, generator=gen)) + 0.02).to(device))
    return model


def bare_ment(device, d, a):
    """No measurement slots: the density is the Gaussian prior alone."""
    return MENT(ndim=d, transforms=[], diagnostics=[], measurements=[], prior=Gaussian(ndim=d, scale=a), mode="sample",
                device=device)


# ---------------------------------------------------------------------------------------------- estimator level
def test_ment_prior_without_slots_is_the_gaussian_prior(backend):
    d, a, n = 4, 1.7, 5000
    gen = torch.Generator().manual_seed(3)
    x = (1.3 * torch.randn(n, d, generator=gen)).to(backend)
    logq = torch.randn(n, generator=gen).to(backend)
    out = []
    for prior in (MENTPrior(bare_ment(backend, d, a), pad=0.0), Gaussian(ndim=d, scale=a)):
        xr = x.clone().requires_grad_(True)
        est = MonteCarloEntropyEstimator(prior)
        H = est(xr, logq)
        H.backward()
        out.append((float(H.detach()), xr.grad.clone()))
    (Hm, gm), (Hg, gg) = out
    print("H", Hm, Hg, "max rel grad", float(((gm - gg).abs() / gg.abs().clamp_min(1e-30)).max()))
    assert abs(Hm - Hg) <= 1e-5
    assert float(gg.abs().min()) > 0 and bool(((gm - gg).abs() <= 1e-6 * gg.abs()).all())


def test_sums_for_gaussian_and_none_are_bitwise_the_two_entropy_sums(backend):
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(3000, 3, generator=gen).to(backend)
    logq = torch.randn(3000, generator=gen).to(backend)
    want = ops.EntropySumsFn.apply(x, logq)
    for prior in (None, Gaussian(ndim=3, scale=1.2)):
        est = MonteCarloEntropyEstimator(prior)
        got = est.sums(x, logq)
        assert got.shape == (2,) and torch.equal(got, want)
        assert torch.equal(est(x, logq), est.from_sums(want, 3000))
    three = MonteCarloEntropyEstimator(MENTPrior(bare_ment(backend, 3, 1.2))).sums(x, logq)
    assert three.shape == (3,) and torch.equal(three[:2], want)
    with pytest.raises(NotImplementedError, match="third entry"):
        MonteCarloEntropyEstimator(UniformPrior(ndim=3, scale=9.0)).from_sums(want, 3000)


def test_uniform_prior_takes_the_same_route(backend):
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2000, 2, generator=gen).to(backend)
    logq = torch.randn(2000, generator=gen).to(backend)
    prior = UniformPrior(ndim=2, scale=50.0)
    H = MonteCarloEntropyEstimator(prior)(x, logq)
    assert abs(float(H) - (float(logq.double().mean()) - prior.log_norm())) <= 1e-5


# ---------------------------------------------------------------------------------------------- loss level
def flow_problem(device, generic=False):
    from mentflow_amd.harness import build_problem
    prob = build_problem(ndim=2, num=4, bins=24, xmax=3.5, seed=21, transforms=2, prior_scale=1.0, device=device,
                         dist_name="swissroll", optics="2d_linear", meas_samples=4000, penalty_parameter=20.0, hidden_layers=2,
                         hidden_units=32)
    prob.model.entropy_estimator = MonteCarloEntropyEstimator(MENTPrior(ment_2d(device), pad=PAD))
    if generic:                     # a discrepancy callable the fused tail does not know: the generic loop
        prob.model.discrepancy_function = _plain_kld
    return prob


def _plain_kld(pred, targ):
    return mf.loss.kl_divergence(pred, targ)


@pytest.mark.parametrize("generic", [False, True])
def test_loss_is_the_hand_composed_sum(backend, generic):
    prob = flow_problem(backend, generic)
    model = prob.model
    assert (model._fused_plan() is None) == generic
    n = 3000
    z = (1.5 * torch.randn(n, 2, generator=torch.Generator().manual_seed(8))).to(backend)       # some particles leave the support
    model.generator.inject_z = z
    L, H, D = model.loss(n)
    L.backward()
    grads = [p.grad.clone() for p in model.parameters()]
    assert all(torch.isfinite(g).all() and float(g.abs().max()) > 0 for g in grads)
    with torch.no_grad():
        x, logq = model.generator.sample_and_log_prob(n)
        ld = model.entropy_estimator.prior.ment.log_density(x, PAD)
        outside = int((ld == math.log(PAD)).sum())
        Dh = model.discrepancy_vector(mf.simulate.forward(x, model.transforms, model.diagnostics))
        Hh = float(logq.double().mean() - ld.double().mean())
        Lh = Hh + model.penalty_parameter * float(torch.stack(Dh).double().mean())
    print("generic" if generic else "fused", "L", float(L), Lh, "H", float(H), Hh, "particles outside the support", outside)
    assert outside > 0, "the pad must be exercised"
    assert abs(float(H) - Hh) <= 1e-6 * abs(Hh)
    assert abs(float(L) - Lh) <= 1e-6 * abs(Lh)


def test_save_load_and_to(backend, tmp_path):
    prob = flow_problem(backend)
    model = prob.model
    n = 500
    z = torch.randn(n, 2, generator=torch.Generator().manual_seed(2)).to(backend)
    model.generator.inject_z = z
    L0 = float(model.loss(n)[0].detach())
    assert model.entropy_estimator.prior.ment._plan is not None
    import pickle
    live = model.entropy_estimator.prior
    copy = pickle.loads(pickle.dumps(live))
    assert copy.ment._plan is None and copy.pad == PAD and live.ment._plan is not None      # the plan stays out of the pickle
    path = str(tmp_path / "model.pt")
    model.save(path)
    assert model.entropy_estimator.prior.ment._plan is not None, "saving must not drop the live plan"
    other = flow_problem(backend).model
    other.entropy_estimator = MonteCarloEntropyEstimator(None)
    other.load(path, device=backend)
    prior = other.entropy_estimator.prior
    assert isinstance(prior, MENTPrior) and prior.pad == PAD and prior.ment._plan is None
    other.generator.inject_z = z
    assert float(other.loss(n)[0].detach()) == L0
    moved = []
    prior.ment.to = lambda device: moved.append(device)
    other.to(backend)
    assert moved == [backend]


# ---------------------------------------------------------------------------------------------- data-parallel
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, z, out, generic):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from mentflow_amd import _lib, dist as mfdist
    _lib.use_library(EMU_LIB)
    dev = mfdist.init_from_env(backend="gloo")
    prob = flow_problem(dev, generic)
    n = z.shape[0]
    n_local = mfdist.local_batch(n)
    start = sum((n // world + (1 if r < n % world else 0)) for r in range(rank))
    prob.model.generator.inject_z = z[start:start + n_local].clone()
    L, H, D = prob.model.loss(n)
    L.backward()
    g = torch.cat([p.grad.reshape(-1) for p in prob.model.parameters()])
    out[rank] = (float(L.detach()), float(H.detach()), g)
    dist.destroy_process_group()


@pytest.mark.parametrize("generic", [False, True])
def test_two_ranks_equal_one(emu_library, generic):
    """The third entropy sum joins the one all-reduce: (L, H) and the parameter gradients of 2 ranks are the single-process values
    on the concatenated batch (bounds of tests/test_distributed.py)."""
    from mentflow_amd import _lib
    _lib.use_library(emu_library)
    n = 257
    z = 1.5 * torch.randn(n, 2, generator=torch.Generator().manual_seed(5))
    prob = flow_problem(torch.device("cpu"), generic)
    prob.model.generator.inject_z = z
    L, H, D = prob.model.loss(n)
    L.backward()
    g1 = torch.cat([p.grad.reshape(-1) for p in prob.model.parameters()])
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, _free_port(), z, out, generic), nprocs=2, join=True)
    for r in (0, 1):
        Lr, Hr, gr = out[r]
        assert abs(Lr - float(L.detach())) < 1e-5 + 20 * 1e-6 and abs(Hr - float(H.detach())) < 1e-5
        torch.testing.assert_close(gr, g1, rtol=1e-4, atol=1e-6 * float(g1.abs().max()))
    assert out[0][0] == out[1][0] and torch.equal(out[0][2], out[1][2])
