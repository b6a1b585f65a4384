"""Public interface of the sliced Wasserstein distance and the model evaluator (mentflow_amd.loss.SlicedWassersteinDistance,
mentflow_amd.Evaluator): signature of the reference, seeding, exact properties, refusals, and the evaluator on a small MENTFlow
and a small MENT problem (emulator here, the MI355X with -m gpu); the reference's evaluation shapes on the GPU only."""
import inspect
import math

import numpy as np
import pytest
import torch

import _swd_fp64 as ref
import mentflow_amd as mf
from mentflow_amd.distributions import get_distribution
from mentflow_amd.harness import build_problem
from mentflow_amd.loss import SlicedWassersteinDistance, SlicedWassersteindDistance
from mentflow_amd.train import MENTTrainer


def unit_directions(d, P, gen):
    dirs = torch.randn(d, P, generator=gen)
    return dirs / dirs.norm(dim=0, keepdim=True)


def test_signature_matches_the_reference():
    E = inspect.Parameter.empty
    assert SlicedWassersteinDistance is SlicedWassersteindDistance is mf.loss.SlicedWassersteindDistance
    assert [(p.name, p.default) for p in inspect.signature(SlicedWassersteindDistance.__init__).parameters.values()] == [
        ("self", E), ("n_projections", 50), ("p", 2), ("device", None)]
    call = inspect.signature(SlicedWassersteindDistance.__call__).parameters
    assert list(call) == ["self", "x1", "x2", "directions"]
    assert call["directions"].kind is inspect.Parameter.KEYWORD_ONLY and call["directions"].default is None
    swd = SlicedWassersteindDistance()
    assert (swd.n_projections, swd.p, swd.device) == (50, 2, None)
    assert [(p.name, p.default) for p in inspect.signature(mf.Evaluator.__init__).parameters.values()] == [
        ("self", E), ("size", E), ("discrepancy", mf.loss.kl_divergence), ("distance", None), ("distribution", None)]
    assert mf.Evaluator is mf.evaluate.Evaluator


def test_seed_fixes_the_value(backend):
    gen = torch.Generator().manual_seed(0)
    x1 = torch.randn(700, 4, generator=gen).to(backend)
    x2 = (0.3 + torch.randn(500, 4, generator=gen)).to(backend)
    swd = SlicedWassersteinDistance(n_projections=13, p=2, device=backend)
    torch.manual_seed(7)
    a = swd(x1, x2)
    torch.manual_seed(7)
    b = swd(x1, x2)
    c = swd(x1, x2)                                            # the generator moved on: other slices
    assert a.dim() == 0 and a.dtype == torch.float32 and a.device.type == backend.type
    assert torch.equal(a, b) and not torch.equal(a, c)
    # the draw is the reference's: randn(d, n_projections) on the device, columns normalised
    torch.manual_seed(7)
    dirs = torch.randn(4, 13, device=backend)
    dirs = dirs / torch.sqrt(torch.sum(dirs**2, 0, keepdims=True))
    assert torch.equal(swd(x1, x2, directions=dirs), a)
    x1n, x2n, dn = x1.cpu().numpy(), x2.cpu().numpy(), dirs.cpu().numpy()
    want_sq = float(np.mean(ref.swd_wpp(x1n, x2n, dn, 2.0)))
    bound = float(np.mean(ref.wpp_bound_p2(x1n, x2n, dn))) + (2.0 ** -22 + 1e-6) * want_sq       # see test_translation
    assert abs(float(a) ** 2 - want_sq) <= bound


@pytest.mark.parametrize("p", [1, 2, 3])
def test_identity_and_symmetry(backend, p):
    gen = torch.Generator().manual_seed(1)
    x = (torch.randn(1500, 6, generator=gen) * 3.0).to(backend)
    y = (torch.randn(1500, 6, generator=gen) + 0.5).to(backend)
    dirs = unit_directions(6, 20, gen).to(backend)
    swd = SlicedWassersteinDistance(p=p)
    assert float(swd(x, x, directions=dirs)) == 0.0
    assert float(swd(x, x.flip(0), directions=dirs)) == 0.0    # a permutation of the same cloud: the sort is exact
    assert torch.equal(swd(x, y, directions=dirs), swd(y, x, directions=dirs))


def test_translation(backend):
    """x2 = x1 + t moves every projection rigidly by t . dir_p, so W_2^2 = (t . dir_p)^2 per projection and W_1 = |t . dir_p|.
    Points and shift lie on a 2^-10 grid so that x1 + t is exact in fp32.  Gate: the end-to-end bound of
    tests/test_swd_kernels.py on the mean of the per-projection costs, plus the rounding of the result to fp32 (2^-24 relative
    on the distance, 2^-23 on its square; 2^-22 allows for the root's own rounding) and the cost kernel's 1e-6."""
    gen = torch.Generator().manual_seed(2)
    d, P, N = 6, 50, 4000
    x1 = torch.round(torch.randn(N, d, generator=gen) * 1024.0) / 1024.0
    t = torch.round(torch.randn(d, generator=gen) * 512.0) / 1024.0
    x2 = x1 + t
    assert torch.equal((x2.double() - x1.double()), t.double().expand(N, d))
    dirs = unit_directions(d, P, gen)
    got = float(SlicedWassersteinDistance(p=2)(x1.to(backend), x2.to(backend), directions=dirs.to(backend)))
    shift = t.double().numpy() @ dirs.double().numpy()
    want_sq = float(np.mean(shift**2))
    dl = ref.delta(x1.numpy(), x2.numpy())
    bound = float(np.mean(4.0 * dl * np.abs(shift) + 4.0 * dl * dl)) + (2.0 ** -22 + 1e-6) * want_sq
    print(f"translation: |got^2 - want^2| / bound = {abs(got * got - want_sq) / bound:.2e}")
    assert abs(got * got - want_sq) <= bound


def test_error_cases(backend):
    x = torch.randn(40, 3).to(backend)
    swd = SlicedWassersteinDistance(n_projections=4, device=backend)
    with pytest.raises(ValueError, match=r"x1.shape\[1\]"):
        swd(x, torch.randn(40, 2).to(backend))
    with pytest.raises(ValueError, match="at least one point"):
        swd(x, x[:0])
    with pytest.raises(ValueError, match="at least one point"):
        swd(x[:0], x)
    with pytest.raises(ValueError, match="d <= 8"):
        swd(torch.randn(10, 9).to(backend), torch.randn(10, 9).to(backend))
    with pytest.raises(ValueError, match="2\\^31"):
        swd(x, x, directions=torch.empty(3, 2**31 // 40 + 1, device="meta"))
    with pytest.raises(ValueError, match="directions"):
        swd(x, x, directions=torch.randn(2, 4).to(backend))
    xg = x.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="no_grad"):
        swd(xg, x)
    with pytest.raises(NotImplementedError, match="no_grad"):
        swd(x, xg)
    with torch.no_grad():
        assert torch.isfinite(swd(xg, x).cpu())
    bad = x.clone()
    bad[17, 1] = float("nan")
    assert torch.isnan(swd(bad, x).cpu()) and torch.isnan(swd(x, bad[:30]).cpu())
    with pytest.raises(ValueError, match="distribution"):
        mf.Evaluator(100, distance=swd)


def test_no_cpu_fallback():
    import os
    import __graft_entry__ as g
    from mentflow_amd import _lib
    if not os.path.exists(g.LIB):
        g.build()
    _lib.use_library(g.LIB)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SlicedWassersteinDistance(n_projections=3)(torch.randn(8, 2), torch.randn(8, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mf.ops.segmented_sort(torch.randn(2, 8))


# ------------------------------------------------------------------------------------------------ evaluator
def test_evaluator_on_a_flow(backend, capsys):
    prob = build_problem(ndim=2, num=3, bins=16, xmax=3.5, seed=21, transforms=2, prior_scale=1.0, device=backend,
                         meas_samples=4000, dist_name="swissroll", optics="2d_linear")
    evaluator = mf.Evaluator(3000, distance=SlicedWassersteinDistance(n_projections=10, device=backend),
                             distribution=get_distribution("swissroll", ndim=2, seed=21))
    torch.manual_seed(0)
    result = evaluator(prob.model)
    assert set(result) == {"discrepancy", "distance"}
    assert isinstance(result["discrepancy"], float) and isinstance(result["distance"], float)
    assert math.isfinite(result["discrepancy"]) and result["discrepancy"] > 0.0
    assert math.isfinite(result["distance"]) and result["distance"] > 0.0
    out = capsys.readouterr().out
    assert "disc(y_model, y_true)" in out and "dist(x_model, x_true)" in out
    # the discrepancy is the mean of the model's own discrepancy function over the measurements of the same samples
    plain = mf.Evaluator(3000)
    plain.verbose = False
    r2 = plain(prob.model)
    assert r2["distance"] is None and math.isfinite(r2["discrepancy"])
    # as the eval hook of the Trainer
    seen = []
    opt = torch.optim.AdamW(prob.model.parameters(), lr=1e-3, weight_decay=0.0)
    evaluator.verbose = False
    trainer = mf.train.Trainer(prob.model, opt, eval=lambda m: seen.append(evaluator(m)), verbose=False)
    trainer.train(epochs=1, iterations=2, batch_size=512, eval_batch_size=512)
    assert len(seen) == 1 and math.isfinite(seen[0]["distance"])


def test_evaluator_drives_the_ment_trainer(backend):
    from test_ment_api import small_problem
    torch.manual_seed(0)
    n = 100000 if backend.type == "cuda" else 20000
    model = small_problem(backend, ndim=4, num=6, bins=16, res=10, n_samples=n)
    truth = get_distribution("gaussian", ndim=4, seed=3)
    evaluator = mf.Evaluator(n, distance=SlicedWassersteinDistance(n_projections=8, device=backend), distribution=truth)
    evaluator.verbose = False
    first = evaluator(model)
    assert math.isfinite(first["discrepancy"]) and math.isfinite(first["distance"]) and first["distance"] > 0.0
    trainer = MENTTrainer(model=model, eval=evaluator)
    trainer.verbose = False
    dmax = 0.5 * first["discrepancy"]
    trainer.train(epochs=6, lr=0.9, dmax=dmax)
    D = trainer.history["D_norm"]
    assert all(isinstance(v, float) and math.isfinite(v) for v in D)
    assert len(D) < 7 and D[-1] <= dmax and all(v > dmax for v in D[:-1])      # stopped at the first epoch at or below dmax


# ------------------------------------------------------------------------------------------------ the reference's shapes
@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", [(50000, 50000), (1000000, 1000000), (50000, 30011)])
def test_reference_evaluation_shapes(n1, n2):
    """d = 6, P = 50, nearby Gaussians (experiments/*/setup.py::setup_eval: 50 000 samples each; 1 000 000 is the size of the
    reference's ground-truth sets) against the fp64 restatement, gated by the end-to-end bound on the mean cost."""
    from mentflow_amd import _lib
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(n1 + n2)
    d, P = 6, 50
    x1 = torch.randn(n1, d, generator=gen)
    x2 = 0.15 + 1.05 * torch.randn(n2, d, generator=gen)
    dirs = unit_directions(d, P, gen)
    swd = SlicedWassersteinDistance(n_projections=P, p=2, device=dev)
    a = swd(x1.to(dev), x2.to(dev), directions=dirs.to(dev))
    b = swd(x1.to(dev), x2.to(dev), directions=dirs.to(dev))
    assert torch.equal(a, b)
    got = float(a)
    want = ref.swd_wpp(x1.numpy(), x2.numpy(), dirs.numpy(), 2.0)
    bound = float(np.mean(ref.wpp_bound_p2(x1.numpy(), x2.numpy(), dirs.numpy()))) + (2.0 ** -22 + 1e-6) * float(np.mean(want))
    err = abs(got * got - float(np.mean(want)))
    print(f"{n1} vs {n2}: SWD {got:.7f} (fp64 {math.sqrt(float(np.mean(want))):.7f}), |got^2 - want^2| / bound = {err / bound:.2e}")
    assert err <= bound
