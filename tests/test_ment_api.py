"""Classical MENT public interface (mentflow_amd.ment / sample / train.MENTTrainer): signatures of the reference, refusals,
the diagnostics' project / shape, save / load, the trainer, and the solver itself on small problems (emulator here, the
MI355X with -m gpu)."""
import inspect
import math

import pytest
import torch

import mentflow_amd as mf
import mentflow_amd.harness  # noqa: F401  (mf.harness)
from mentflow_amd.ment import MENT, LagrangeFunction
from mentflow_amd.sample import GridSampler, sample_hist
from mentflow_amd.train import MENTTrainer


def params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_signatures_match_the_reference():
    E = inspect.Parameter.empty
    assert params(MENT.__init__) == [
        ("self", E), ("ndim", E), ("transforms", E), ("diagnostics", E), ("measurements", E),
        ("discrepancy_function", mf.loss.kl_divergence), ("prior", None), ("interpolation", "linear"), ("mode", "integrate"),
        ("integration_limits", None), ("integration_shape", None), ("sampler", None), ("n_samples", 1000000),
        ("device", None), ("verbose", False)]
    for name in ("send", "set_diagnostics", "set_measurements", "initialize_lagrange_functions", "normalize_projection",
                 "get_meas_points", "get_integration_points", "evaluate_lagrange_function", "prob", "log_prob", "sample",
                 "sample_and_log_prob", "discrepancy_vector", "simulate", "simulate_all", "save", "load", "to"):
        assert callable(getattr(MENT, name)), name
    assert params(MENT.gauss_seidel_update)[:3] == [("self", E), ("lr", 1.0), ("thresh", 1e-10)]
    assert params(LagrangeFunction.__init__)[:3] == [("self", E), ("coords", E), ("values", E)]
    assert params(sample_hist) == [("hist", E), ("edges", E), ("size", E), ("noise", 0.0), ("device", None)]
    assert params(GridSampler.__init__) == [("self", E), ("limits", E), ("shape", E), ("noise", 0.0), ("device", None),
                                             ("store", True)]
    assert params(MENTTrainer.__init__) == [("self", E), ("model", None), ("plot", None), ("eval", None),
                                             ("output_dir", None), ("notebook", False)]
    assert params(MENTTrainer.train) == [("self", E), ("epochs", E), ("lr", 0.99), ("thresh", 1e-10), ("savefig_kws", None),
                                         ("dmax", 0.0)]
    for name in ("random_uniform", "random_choice", "sample_hist_bins"):
        assert callable(getattr(mf.sample, name))
    assert issubclass(MENTTrainer, mf.train.Trainer)


def small_problem(device, ndim=4, num=6, bins=16, mode="sample", res=8, n_samples=20000, seed=1):
    torch.manual_seed(seed)
    transforms = [t.to(device) for t in mf.harness.make_transforms_nd_1d(num, ndim, seed)]
    diag = mf.diagnostics.Histogram1D(axis=0, edges=torch.linspace(-3.5, 3.5, bins + 1), bandwidth=0.5).to(device)
    diagnostics = [[diag] for _ in transforms]
    x = torch.randn(50000, ndim) * torch.tensor([1.0, 0.6, 1.3, 0.8][:ndim] + [1.0] * max(0, ndim - 4))
    x = x.to(device)
    diag.kde = False
    meas = [[d(t(x)) for d in ds] for t, ds in zip(transforms, diagnostics)]
    diag.kde = True
    sampler = GridSampler(limits=ndim * [(-3.5, 3.5)], shape=ndim * [res]).to(device)
    model = MENT(ndim=ndim, transforms=transforms, diagnostics=diagnostics, measurements=meas,
                 prior=mf.prior.Gaussian(ndim=ndim, scale=3.0), mode=mode, sampler=sampler, n_samples=n_samples,
                 integration_limits=[[(ndim - 1) * [(-3.5, 3.5)]] for _ in transforms],
                 integration_shape=[[(ndim - 1) * [res]] for _ in transforms], device=device)
    return model


def mean_kl(model, preds=None):
    preds = model.simulate_all() if preds is None else preds
    return float(torch.stack([d.float() for d in model.discrepancy_vector(preds)]).mean())


def test_refusals():
    with pytest.raises(NotImplementedError, match="cubic"):
        LagrangeFunction(torch.linspace(0, 1, 5), torch.ones(5), method="cubic")
    diag = mf.diagnostics.Histogram1D(axis=0, edges=torch.linspace(-1, 1, 5))
    kw = dict(ndim=2, transforms=[mf.simulate.LinearTransform(torch.eye(2))], diagnostics=[[diag]],
              measurements=[[torch.ones(4)]])
    with pytest.raises(NotImplementedError, match="nearest"):
        MENT(interpolation="nearest", **kw)
    with pytest.raises(NotImplementedError, match="prior"):
        MENT(prior=object(), **kw)
    m = MENT(**kw)
    assert isinstance(m.prior, mf.ment.UniformPrior) and m.prior.scale == 100.0
    dirdiag = mf.diagnostics.Histogram1D(axis=0, edges=torch.linspace(-1, 1, 5), direction=torch.tensor([1.0, 1.0]))
    m = MENT(ndim=2, transforms=[mf.simulate.LinearTransform(torch.eye(2))], diagnostics=[[dirdiag]],
             measurements=[[torch.ones(4)]], integration_limits=[[[(-1, 1)]]], integration_shape=[[[5]]])
    with pytest.raises(NotImplementedError, match="direction"):
        m.simulate(0, 0)
    m.mode = "bogus"
    with pytest.raises(ValueError):
        m.simulate(0, 0)


def test_no_cpu_fallback():
    import __graft_entry__ as g
    import os
    from mentflow_amd import _lib
    if not os.path.exists(g.LIB):
        pytest.skip("gfx950 library not built")
    _lib.use_library(g.LIB)
    lf = LagrangeFunction(torch.linspace(0, 1, 5), torch.ones(5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lf(torch.rand(8))


def test_histogram_project_and_shape():
    x = torch.randn(10, 4)
    h1 = mf.diagnostics.Histogram1D(axis=2, edges=torch.linspace(-1, 1, 5))
    assert torch.equal(h1.project(x), x[:, 2])
    d = torch.tensor([1.0, 0.0, 1.0, 0.0])
    h1d = mf.diagnostics.Histogram1D(axis=0, edges=torch.linspace(-1, 1, 5), direction=d)
    assert torch.allclose(h1d.project(x), (x[:, 0] + x[:, 2]) / math.sqrt(2.0))
    h2 = mf.diagnostics.Histogram2D(axis=(0, 3), edges=[torch.linspace(-1, 1, 6), torch.linspace(-1, 1, 8)])
    assert torch.equal(h2.project(x), x[:, (0, 3)])
    assert h2.shape == (5, 7)


def test_lagrange_function_nonuniform_grid_runs_in_torch(backend):
    c = torch.tensor([-1.0, -0.5, 0.25, 1.0]).to(backend)
    v = torch.tensor([1.0, 2.0, 0.5, 3.0]).to(backend)
    lf = LagrangeFunction(c, v)
    u = torch.tensor([-1.0, -0.75, 0.0, 1.0, 1.01, float("nan")]).to(backend)
    h = lf(u).cpu()
    assert torch.allclose(h[:5], torch.tensor([1.0, 1.5, 2.0 - 1.5 * (0.5 / 0.75), 3.0, 0.0]))
    assert torch.isnan(h[5])


def test_save_load_roundtrip(backend, tmp_path):
    model = small_problem(backend, num=3, res=6, n_samples=5000)
    model.lagrange_functions[1][0].set_values(model.lagrange_functions[1][0].values * 1.5)
    model.epoch = 3
    x = torch.randn(300, 4).to(backend)
    p = model.prob(x)
    path = str(tmp_path / "ment.pt")
    model.save(path)
    other = small_problem(backend, num=3, res=6, n_samples=5000, seed=2)
    other.load(path, device=backend)
    assert other.epoch == 3
    assert torch.equal(other.prob(x), p)


def test_trainer_runs_and_logs(backend):
    torch.manual_seed(0)
    model = small_problem(backend, num=3, res=6, n_samples=5000)
    seen = []

    def evaluate(m):
        seen.append(m.epoch)
        return {"discrepancy": mean_kl(m)}

    trainer = MENTTrainer(model=model, eval=evaluate)
    trainer.verbose = False
    trainer.train(epochs=2, lr=0.9)
    assert trainer.history["epoch"] == [0, 1, 2] and seen == [0, 1, 2] and model.epoch == 2
    assert set(trainer.history) >= {"epoch", "iteration", "time", "D_norm"}
    assert all(isinstance(v, float) for v in trainer.history["D_norm"])
    # dmax stops at the first evaluation at or below it
    trainer = MENTTrainer(model=model, eval=lambda m: {"discrepancy": 0.0})
    trainer.verbose = False
    trainer.train(epochs=5, dmax=0.0)
    assert trainer.history["epoch"] == [0] and model.epoch == 2


def test_sample_mode_reduces_kl(backend):
    torch.manual_seed(0)
    n = 200000 if backend.type == "cuda" else 30000
    model = small_problem(backend, ndim=4, num=6, bins=16, res=10, n_samples=n)
    kl = [mean_kl(model)]
    for _ in range(3):
        model.gauss_seidel_update(lr=0.9)
        kl.append(mean_kl(model))
    assert kl[-1] < 0.5 * kl[0], kl
    assert all(torch.isfinite(v.values).all() for v in mf.utils.unravel(model.lagrange_functions))


def test_integrate_and_sample_agree_2d(backend):
    """The same tables simulated both ways: line integrals on a dense grid vs KDE histograms of grid samples."""
    torch.manual_seed(3)
    transforms = [t.to(backend) for t in mf.harness.make_transforms_2d_linear(4)]
    diag = mf.diagnostics.Histogram1D(axis=0, edges=torch.linspace(-3.0, 3.0, 25), bandwidth=0.5).to(backend)
    x = (torch.randn(40000, 2) * torch.tensor([1.0, 0.5])).to(backend)
    diag.kde = False
    meas = [[diag(t(x))] for t in transforms]
    diag.kde = True
    n = 400000 if backend.type == "cuda" else 60000
    model = MENT(ndim=2, transforms=transforms, diagnostics=[[diag] for _ in transforms], measurements=meas,
                 prior=mf.prior.Gaussian(ndim=2, scale=2.0), mode="integrate",
                 integration_limits=[[[(-3.0, 3.0)]] for _ in transforms], integration_shape=[[[200]] for _ in transforms],
                 sampler=GridSampler(limits=[(-3.0, 3.0)] * 2, shape=(120, 120)).to(backend), n_samples=n, device=backend)
    model.gauss_seidel_update(lr=0.9)
    integ = model.simulate_all()
    model.mode = "sample"
    samp = [[model.simulate(i, 0)] for i in range(len(transforms))]
    for a, b in zip(mf.utils.unravel(integ), mf.utils.unravel(samp)):
        a, b = a.cpu(), b.cpu()
        assert abs(float(a.sum() - b.sum())) < 1e-3 * float(a.sum())
        assert float((a - b).abs().max()) < 0.08 * float(a.max()), float((a - b).abs().max() / a.max())
