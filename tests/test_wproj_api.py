"""Particle weights through the public interface: Histogram1D / Histogram2D (raw_sums, batched, forward, from_sums),
simulate.forward, sample_weighted of the annealed and the sequential Monte Carlo sampler, and MENT.weighted.  Emulator
here, the MI355X with -m gpu.  References are fp64 (tests/_wproj_fp64.py) or the unweighted path of the same object.

Gates: the suite's histogram gate rtol 2e-5 + atol 1e-6 and gradient gate rtol 1e-3 + atol 2e-5 max|g| + 1e-6
(tests/test_kde_launch_paths.py); weights 1 against the unweighted call rtol 1e-6.

MENT(mode="sample") with .weighted = True (an attribute: tests/test_ment_api.py pins the constructor to the reference's
signature) against the same model's mode="integrate" prediction.  The fp64 prototype of the weighted
estimator (`python tests/_wproj_fp64.py`: the samplers' fp64 prototype of tests/_smc_fp64.py, the weighted KDE of every view in
fp64, on cases (a) and (b) and the settings of tests/test_ais_api.py: 2 048 chains, 32 temperatures) printed, as the max-abs
difference over all views and bins for seeds 0 .. 4:

  case a, ais: 0.1362 0.1115 0.1152 0.1276 0.1277   worst 0.1362   (largest predicted density 0.721)
  case a, smc: 0.1362 0.1115 0.1152 0.1276 0.1277   worst 0.1362   (8 islands, threshold 0.5: no island fell below it)
  case b, ais: 0.1233 0.0948 0.0881 0.0879 0.1056   worst 0.1233   (largest predicted density 0.577)
  case b, smc: 0.1233 0.0948 0.0881 0.0879 0.1056   worst 0.1233

Most of it is not Monte-Carlo noise: the sample-mode prediction is a Gaussian KDE of half a bin's bandwidth on 0.5-wide bins of
tables that jump by up to a factor 3 from bin to bin, and the integrate-mode one is the density at the bin centres.  Gates,
about twice the worst as tests/test_smc_api.py sets its own: 0.27 for case (a), 0.25 for case (b)."""
import os

import numpy as np
import pytest
import torch

import mentflow_amd as mf
from _wproj_fp64 import integration_grids, normalise_1d, normalise_2d
from conftest import GOLDEN
from mentflow_amd.diagnostics import Histogram1D, Histogram2D, Projection
from mentflow_amd.ment import MENT
from mentflow_amd.sample import AnnealedImportanceSampler, MetropolisHastingsSampler, SequentialMonteCarloSampler
from mentflow_amd.simulate import CompositeTransform, LinearTransform, MultipoleTransform, forward, rotation_matrix
from test_ais_api import SETTINGS, build

MENT_GATE = {"a": 0.27, "b": 0.25}


def assert_hist(h, ho):
    torch.testing.assert_close(h.detach().double().cpu(), ho.detach().double().cpu(), rtol=2e-5, atol=1e-6)


def assert_grad(g, go):
    go = go.detach().double().cpu()
    torch.testing.assert_close(g.detach().double().cpu(), go, rtol=1e-3, atol=2e-5 * float(go.abs().max()) + 1e-6)


def _edges(B, graded, lo=-3.0, hi=3.0):
    t = torch.linspace(-1.0, 1.0, B + 1)
    if graded:
        t = 0.5 * (t + t ** 3)                                  # bins that widen towards the ends
    return lo + (t + 1.0) * 0.5 * (hi - lo)


def _diag(ndim, kde, graded, device):
    if ndim == 1:
        return Histogram1D(axis=1, edges=_edges(16, graded), bandwidth=0.5, kde=kde).to(device)
    return Histogram2D(axis=(0, 2), edges=[_edges(9, graded), _edges(7, False, -2.5, 3.0)], bandwidth=(0.5, 0.5), kde=kde).to(device)


CONFIGS = [(nd, kde, graded) for nd in (1, 2) for kde in (True, False) for graded in (False, True)]
IDS = [f"{nd}d-{'kde' if kde else 'bins'}-{'graded' if g else 'uniform'}" for nd, kde, g in CONFIGS]


# ------------------------------------------------------------------------------------------------ diagnostics
@pytest.mark.parametrize("ndim,kde,graded", CONFIGS, ids=IDS)
def test_unit_and_integer_weights(backend, ndim, kde, graded):
    gen = torch.Generator().manual_seed(3)
    n = 301
    x = torch.randn(n, 3, generator=gen).to(backend)
    diag = _diag(ndim, kde, graded, backend)
    assert diag.uniform is (not graded)
    plain = diag(x)
    torch.testing.assert_close(diag(x, torch.ones(n, device=backend)), plain, rtol=1e-6, atol=1e-12)
    rows = diag.identity_rows(x)
    torch.testing.assert_close(diag.batched(x, rows, torch.ones(n, device=backend)), diag.batched(x, rows), rtol=1e-6, atol=1e-12)
    # integer weights 1 .. 3: the histogram of the rows repeated that many times
    k = torch.randint(1, 4, (n,), generator=gen)
    w = k.to(torch.float32).to(backend)
    repeated = x[torch.repeat_interleave(torch.arange(n), k).to(backend)]
    assert_hist(diag(x, w), diag(repeated))
    S = diag.raw_sums(x, rows, w)
    assert_hist(S, diag.raw_sums(repeated, rows))
    assert_hist(diag.from_sums(S, n, w), diag.from_sums(diag.raw_sums(repeated, rows), repeated.shape[0]))
    # invalid weights count as zero, also in W
    bad = w.clone()
    bad[3], bad[5], bad[9] = -2.0, float("nan"), float("inf")
    zeroed = bad.clone()
    zeroed[3] = zeroed[5] = zeroed[9] = 0.0
    assert_hist(diag(x, bad), diag(x, zeroed))
    if kde:                                                     # (hard bins divide by the total, as torch.histogram(density=True))
        assert bool((diag(x, torch.zeros(n, device=backend)) == 0).all()), "no valid weight: zeros, not NaN"


@pytest.mark.parametrize("ndim,graded", [(1, False), (1, True), (2, False), (2, True)],
                         ids=["1d-uniform", "1d-graded", "2d-uniform", "2d-graded"])
def test_gradients_in_points_and_weights(backend, ndim, graded):
    gen = torch.Generator().manual_seed(4)
    n = 257
    x0 = torch.randn(n, 3, generator=gen)
    w0 = torch.exp(torch.randn(n, generator=gen))
    w0[5] = 0.0                                                 # a zero weight has a gradient: it can grow
    diag = _diag(ndim, True, graded, backend)
    x, w = x0.clone().to(backend).requires_grad_(True), w0.clone().to(backend).requires_grad_(True)
    h = diag(x, w)
    G = torch.randn(h.shape, generator=gen)
    (h * G.to(backend)).sum().backward()
    # fp64 autograd of the dense formula
    x64, w64 = x0.clone().double().requires_grad_(True), w0.clone().double().requires_grad_(True)
    wv = torch.where(w64 >= 0, w64, torch.zeros_like(w64))
    if ndim == 1:
        c = diag.coords.double().cpu()
        K = torch.exp(-0.5 * ((x64[:, 1, None] - c) / diag.bandwidth_value) ** 2)
        ho = normalise_1d((wv[:, None] * K).sum(0), wv.sum(), diag.cell_value)
    else:
        cx, cy = diag.coords_x.double().cpu(), diag.coords_y.double().cpu()
        Kx = torch.exp(-0.5 * ((x64[:, 0, None] - cx) / diag.bandwidth_values[0]) ** 2)
        Ky = torch.exp(-0.5 * ((x64[:, 2, None] - cy) / diag.bandwidth_values[1]) ** 2)
        ho = normalise_2d(torch.einsum("n,na,nb->ab", wv, Kx, Ky), diag.cell_value)
    (ho * G.double()).sum().backward()
    assert_hist(h, ho)
    assert_grad(x.grad, x64.grad)
    assert_grad(w.grad, w64.grad)
    # per-input skipping: a weight gradient alone, a point gradient alone
    xa, wa = x0.to(backend), w0.clone().to(backend).requires_grad_(True)
    (diag(xa, wa) * G.to(backend)).sum().backward()
    assert torch.equal(wa.grad, w.grad)
    xb, wb = x0.clone().to(backend).requires_grad_(True), w0.to(backend)
    (diag(xb, wb) * G.to(backend)).sum().backward()
    assert torch.equal(xb.grad, x.grad)


# ------------------------------------------------------------------------------------------------ simulate.forward
def _measurement_set(kind, device):
    angles = (0.0, 0.7, 1.9)
    if kind == "1d":
        diag = Histogram1D(axis=0, edges=_edges(16, False), bandwidth=0.5).to(device)
        transforms = [LinearTransform(rotation_matrix(torch.tensor(a)).float()).to(device) for a in angles]
        return transforms, [[diag] for _ in angles], 2
    if kind == "2d":
        diag = Histogram2D(axis=(0, 1), edges=[_edges(9, False), _edges(7, False, -2.5, 3.0)], bandwidth=(0.5, 0.5)).to(device)
        transforms = [LinearTransform(rotation_matrix(torch.tensor(a)).float()).to(device) for a in angles]
        return transforms, [[diag] for _ in angles], 2
    diag = Histogram1D(axis=0, edges=_edges(16, False), bandwidth=0.5).to(device)
    kick = MultipoleTransform(order=3, strength=0.4).to(device)
    transforms = [CompositeTransform(kick, LinearTransform(rotation_matrix(torch.tensor(a)).float())).to(device) for a in angles]
    return transforms, [[diag] for _ in angles], 2


@pytest.mark.parametrize("kind", ["1d", "2d", "multipole"])
def test_simulate_forward_with_weights(backend, kind):
    transforms, diagnostics, d = _measurement_set(kind, backend)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(500, d, generator=gen).to(backend)
    w = torch.exp(torch.randn(500, generator=gen)).to(backend)
    groups, generic = mf.simulate.group_measurements(transforms, diagnostics)
    assert len(groups) == 1 and not generic, "one fused launch group"
    pred = forward(x, transforms, diagnostics, weights=w)
    for i, t in enumerate(transforms):
        assert_hist(pred[i][0], diagnostics[i][0](t(x.clone()), w))
    plain = forward(x, transforms, diagnostics)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(plain, forward(x, transforms, diagnostics, weights=None)))
    assert not torch.allclose(plain[0][0], pred[0][0])


def test_simulate_forward_refuses_weights_for_a_projection(backend):
    transforms, diagnostics, d = _measurement_set("1d", backend)
    diagnostics[1] = [diagnostics[1][0], Projection(axis=0)]
    x = torch.randn(64, d).to(backend)
    forward(x, transforms, diagnostics)                         # unweighted: served by the generic loop
    with pytest.raises(NotImplementedError, match="Projection"):
        forward(x, transforms, diagnostics, weights=torch.ones(64, device=backend))


# ------------------------------------------------------------------------------------------------ samplers
KWS = dict(SETTINGS, chains=256, n_temps=8)


def test_sample_weighted_returns_the_run(backend):
    model, _ = build("a", backend)
    s = AnnealedImportanceSampler(2, seed=2, **KWS).to(backend)
    x, w = s.sample_weighted(model.prob)
    res = AnnealedImportanceSampler(2, seed=2, **KWS).to(backend).run(model)
    assert x.shape == (256, 2) and w.shape == (256,) and x.dtype == w.dtype == torch.float32
    assert torch.equal(x, res["x"]) and torch.equal(w, torch.exp(res["logw"] - res["logw"].max()).float())
    assert float(w.max()) == 1.0
    model_b, _ = build("b", backend)
    s = SequentialMonteCarloSampler(6, seed=2, groups=4, **KWS).to(backend)
    x, w = s.sample_weighted(model_b.prob, 100000)              # size is ignored: the population as it is
    res = SequentialMonteCarloSampler(6, seed=2, groups=4, **KWS).to(backend).run(model_b)
    assert x.shape == (256, 6) and torch.equal(x, res["x"])
    assert torch.equal(w, torch.exp(res["logw"] - res["logw"].max()).float())
    # the population is kept unequalised, and the next call bridges from it
    pop = s.population
    assert torch.equal(pop["logw"], res["logw"]) and torch.equal(pop["x"], res["x"])
    per = pop["logw"].view(4, -1)
    wt = torch.exp(per - torch.logsumexp(per, 1, keepdim=True))
    ess = 1.0 / (wt * wt).sum(1)
    assert bool((ess < per.shape[1] - 1e-6).any()), f"unequal weights in some island (ess {ess.tolist()} of {per.shape[1]})"
    model_b.lagrange_functions[0][0].set_values(model_b.lagrange_functions[0][0].values * 1.2)
    x2, w2 = s.sample_weighted(model_b.prob)
    assert float(s.last["accepted"].sum()) <= s.bridge_steps * 256, "a bridge: bridge_steps transitions, not the ladder"
    assert x2.shape == (256, 6) and not torch.equal(x2, x) and bool(torch.isfinite(w2).all())


def test_call_returns_the_parent_commits_bits(emu_library):
    """__call__ of both samplers is untouched: on the emulator it returns the rows tests/golden/wproj_sampler_bits.npz holds,
    written once from the emulator before sample_weighted existed."""
    from mentflow_amd import _lib
    _lib.use_library(emu_library)
    dev = torch.device("cpu")
    with np.load(os.path.join(GOLDEN, "wproj_sampler_bits.npz")) as f:
        gold = {k: torch.from_numpy(f[k]) for k in f.files}
    model, _ = build("a", dev)
    assert torch.equal(AnnealedImportanceSampler(2, seed=2, **KWS).to(dev)(model.prob, 300), gold["ais_a"])
    model, _ = build("b", dev)
    s = SequentialMonteCarloSampler(6, seed=2, groups=4, **KWS).to(dev)
    assert torch.equal(s(model.prob, 300), gold["smc_b_first"])
    assert torch.equal(s(model.prob, 300), gold["smc_b_second"])


# ------------------------------------------------------------------------------------------------ MENT
@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("name", ["ais", "smc"])
def test_weighted_ment_against_integrate_mode(backend, case, name, monkeypatch):
    """Gate and prototype figures: module docstring.  The gate is wide (mostly the systematic gap between a half-bin KDE and a
    point density), so beside it the test pins what the model bins: the (x, w) of a same-seed sampler's sample_weighted, through
    simulate.forward with those weights, at the histogram gate; that this differs from binning the same x without weights; and
    that `chains` rows reach the histograms, with weights, not n_samples."""
    model, _ = build(case, backend)
    integration_grids(model, case)
    model.mode = "integrate"
    ref = torch.stack([p[0] for p in model.simulate_all()])
    d = model.ndim

    def fresh():                                                # same seed: the same ladder, states and weights every time
        return (AnnealedImportanceSampler(d, seed=5, **SETTINGS) if name == "ais" else
                SequentialMonteCarloSampler(d, seed=5, groups=8, **SETTINGS)).to(backend)

    weighted = MENT(ndim=d, transforms=model.transforms, diagnostics=model.diagnostics, measurements=model.measurements,
                    prior=model.prior, mode="sample", sampler=fresh(), device=backend)
    weighted.weighted = True
    assert weighted.n_samples == 1000000
    for i, lf in enumerate(model.lagrange_functions):
        weighted.lagrange_functions[i][0].set_values(lf[0].values)
    seen = []                                                   # (rows, weights given) of every raw_sums call
    for row in model.diagnostics:
        def spy(x, rows, weights=None, _inner=row[0].raw_sums):
            seen.append((x.shape[0], None if weights is None else tuple(weights.shape)))
            return _inner(x, rows, weights)
        monkeypatch.setattr(row[0], "raw_sums", spy)
    pred = torch.stack([p[0] for p in weighted.simulate_all()])
    assert seen and all(s == (SETTINGS["chains"], (SETTINGS["chains"],)) for s in seen), seen
    diff = float((pred - ref).abs().max())
    print(f"case {case}, {name}: max |weighted sample-mode - integrate-mode| = {diff:.4f} (gate {MENT_GATE[case]})")
    assert pred.shape == ref.shape and diff <= MENT_GATE[case]
    # what was binned: the weighted states of the sampler, with their weights
    x, w = fresh().sample_weighted(weighted.prob)
    assert x.shape == (SETTINGS["chains"], d) and float(w.min()) < 0.5 < float(w.max()), "weights that matter"
    direct = forward(x, model.transforms, model.diagnostics, weights=w)
    direct = torch.stack([weighted.normalize_projection(p[0], i, 0) for i, p in enumerate(direct)])
    assert_hist(pred, direct)
    plain = forward(x, model.transforms, model.diagnostics)
    plain = torch.stack([weighted.normalize_projection(p[0], i, 0) for i, p in enumerate(plain)])
    lost = float((pred - plain).abs().max())
    print(f"case {case}, {name}: max |weighted - the same states without weights| = {lost:.4f}")
    assert lost > 100 * (2e-5 * float(plain.max()) + 1e-6), "dropping the weights must show far beyond the histogram gate"
    # one sub-step's prediction, from a fresh sampler again: the same states, one view
    weighted.sampler = fresh()
    seen.clear()
    one = weighted.simulate(0, 0)
    assert seen == [(SETTINGS["chains"], (SETTINGS["chains"],))], seen
    assert_hist(one, direct[0])
    assert float((one - ref[0]).abs().max()) <= MENT_GATE[case]
    if name == "smc":                                           # the population is kept unequalised; the next sub-step bridges
        assert weighted.sampler.population is not None
        weighted.simulate(1, 0)
        assert float(weighted.sampler.last["accepted"].sum()) <= weighted.sampler.bridge_steps * SETTINGS["chains"]
    weighted.gauss_seidel_update()
    assert all(bool(torch.isfinite(lf[0].values).all()) for lf in weighted.lagrange_functions)
    # without the flag the same model bins n_samples equal-weight rows
    weighted.weighted = False
    weighted.n_samples = 3000
    seen.clear()
    weighted.simulate(0, 0)
    assert seen == [(3000, None)], seen


class _Moments(mf.diagnostics.Diagnostic):
    """a diagnostic with no weighted form"""

    def forward(self, x):
        return x.mean(0)


class _FixedWeighted:
    """any sampler with sample_weighted serves: fixed rows and weights (the annealed samplers refuse a MENT that is not fully
    fused, which one with a diagnostic outside the kernels is not)"""

    def __init__(self, x, w):
        self.x, self.w = x, w

    def sample_weighted(self, prob_func, size=None):
        return self.x, self.w

    def to(self, device):
        return self


def test_weighted_ment_names_a_diagnostic_without_weights(backend):
    model, _ = build("a", backend)
    gen = torch.Generator().manual_seed(1)
    x, w = torch.randn(500, 2, generator=gen).to(backend), torch.rand(500, generator=gen).to(backend)
    m = MENT(ndim=2, transforms=model.transforms, diagnostics=model.diagnostics, measurements=model.measurements,
             prior=model.prior, mode="sample", sampler=_FixedWeighted(x, w), device=backend)
    m.weighted = True
    direct = model.diagnostics[0][0](model.transforms[0](x), w)
    assert_hist(m.simulate(0, 0), m.normalize_projection(direct, 0, 0))
    m.diagnostics[0] = [m.diagnostics[0][0], _Moments()]       # a second diagnostic behind view 0, with no weighted form
    m.lagrange_functions[0].append(m.lagrange_functions[0][0])
    m._plan = None
    with pytest.raises(NotImplementedError, match="_Moments"):
        m._simulate_sample(0, 1)
    # the flag checks its sampler when it is set AND when it is used: a sampler swapped in later is caught too
    m.sampler = MetropolisHastingsSampler(2, chains=64).to(backend)
    with pytest.raises(TypeError, match="sample_weighted"):
        m.simulate(0, 0)


def test_weighted_ment_needs_a_weighted_sampler(backend, tmp_path):
    model, _ = build("a", backend)
    kws = dict(ndim=2, transforms=model.transforms, diagnostics=model.diagnostics, measurements=model.measurements,
               prior=model.prior, mode="sample", device=backend)
    with pytest.raises(TypeError, match="sample_weighted"):
        MENT(sampler=MetropolisHastingsSampler(2, chains=64), **kws).weighted = True
    with pytest.raises(TypeError, match="sample_weighted"):
        MENT(sampler=None, **kws).weighted = True
    assert MENT(sampler=None, **kws).weighted is False
    m = MENT(sampler=AnnealedImportanceSampler(2, seed=1, **KWS).to(backend), **kws)
    m.weighted = True
    path = str(tmp_path / "ment.pt")
    m.save(path)
    fresh = MENT(sampler=None, **kws)
    fresh.load(path, device=backend)
    assert fresh.weighted is True and isinstance(fresh.sampler, AnnealedImportanceSampler)
