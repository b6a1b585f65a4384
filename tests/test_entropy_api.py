"""Public interface of the sample-based entropy estimators: the reference's constructor signatures, their place in
harness.build_problem and MENTFlow.loss (generic path, no edit of the fused plan), and a short training run on the GPU."""
import inspect
import math

import numpy as np
import pytest
import torch

import _entropy_fp64 as ref
import mentflow_amd as mf
from mentflow_amd.harness import build_problem


def small_nn_problem(device, estimator):
    return build_problem(ndim=2, num=3, bins=16, xmax=4.5, seed=21, device=device, dist_name="rings", meas_samples=4000,
                         optics="2d_nonlinear", gen_name="nn", hidden_layers=2, hidden_units=16, discrepancy="mae",
                         entropy_estimator=estimator)


def test_signatures_equal_the_references(golden):
    recorded = bytes(golden("ref_entropy_cov")["signatures"].numpy().tobytes()).decode().split("\n")
    assert recorded == ["CovarianceEntropyEstimator(self, prior: Any = None, pad: float = 1e-12) -> None",
                        "KNNEntropyEstimator(self, prior: Any = None, k: int = 5) -> None"]
    for line in recorded:
        name = line.split("(")[0]
        assert f"{name}{inspect.signature(getattr(mf.entropy, name).__init__)}" == line
    est = mf.entropy.KNNEntropyEstimator()
    assert est.k == 5 and est.prior is None and isinstance(est, mf.entropy.EntropyEstimator)
    cov = mf.entropy.CovarianceEntropyEstimator()
    assert cov.pad == 1e-12 and cov.prior is None
    fwd = inspect.signature(mf.entropy.KNNEntropyEstimator.forward)
    assert list(fwd.parameters) == ["self", "x", "log_prob"] and fwd.parameters["log_prob"].default is None
    assert "-3 ln(2 pi e)" in mf.entropy.CovarianceEntropyEstimator.__doc__       # the reference's constant is kept and named


def test_a_prior_is_refused_with_the_references_message():
    for cls in (mf.entropy.KNNEntropyEstimator, mf.entropy.CovarianceEntropyEstimator):
        with pytest.raises(ValueError) as e:
            cls(prior=object())
        assert str(e.value) == "This class cannot estimate relative entropy (prior != None)."


def test_no_cpu_fallback():
    import os
    import __graft_entry__ as g
    from mentflow_amd import _lib
    if not os.path.exists(g.LIB):
        g.build()
    _lib.use_library(g.LIB)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mf.entropy.KNNEntropyEstimator()(torch.randn(64, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mf.entropy.CovarianceEntropyEstimator()(torch.randn(64, 2))


def test_build_problem_estimator_choice(backend):
    """None keeps today's choice exactly; the names mirror get_entropy_estimator (experiments/setup.py:91-97)."""
    kws = dict(ndim=2, num=2, bins=8, xmax=3.5, seed=3, transforms=1, device=backend, meas_samples=500, optics="2d_linear")
    assert type(build_problem(gen_name="nn", **kws).model.entropy_estimator) is mf.entropy.EmptyEntropyEstimator
    flow = build_problem(gen_name="nsf", **kws).model.entropy_estimator
    assert type(flow) is mf.entropy.MonteCarloEntropyEstimator and isinstance(flow.prior, mf.prior.Gaussian)
    want = {"none": mf.entropy.EmptyEntropyEstimator, "mc": mf.entropy.MonteCarloEntropyEstimator,
            "cov": mf.entropy.CovarianceEntropyEstimator, "knn": mf.entropy.KNNEntropyEstimator}
    for name, cls in want.items():
        est = build_problem(gen_name="nn", entropy_estimator=name, **kws).model.entropy_estimator
        assert type(est) is cls
        if name in ("cov", "knn"):
            assert est.prior is None
    with pytest.raises(ValueError, match="Invalid entropy estimator"):
        build_problem(gen_name="nn", entropy_estimator="kde", **kws)


@pytest.mark.parametrize("name", ["knn", "cov"])
def test_loss_takes_the_generic_path_and_differentiates(backend, name):
    prob = small_nn_problem(backend, name)
    model = prob.model
    model.penalty_parameter = 10.0
    assert model._fused_plan() is None                     # neither Monte-Carlo nor empty: the generic loop of loss()
    torch.manual_seed(5)
    L, H, D = model.loss(700)
    assert torch.is_tensor(H) and H.dim() == 0 and H.dtype == torch.float32 and math.isfinite(float(H))
    assert float(L) == pytest.approx(float(H) + 10.0 * float(sum(D) / len(D)), rel=1e-5)
    L.backward()
    params = list(model.parameters())
    assert params and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    assert any(float(p.grad.abs().max()) > 0 for p in params)
    # H is the estimator applied to the same samples
    torch.manual_seed(5)
    x = model.sample(700)
    assert torch.equal(model.entropy_estimator(x, None).detach(), H.detach())
    if name == "knn":
        # the bound of test_entropy_kernels.test_neighbours_value_and_gradient: (d / 2)(d + 2) u from the rounding of rho^2,
        # u |H| from the one rounding of H, 1e-9 for the fp64 logarithm, sum and constant (d = 2, N = 700, u = 2^-24)
        H64 = ref.knn_entropy(x.detach().cpu().numpy(), 5)[0]
        assert abs(float(H.detach()) - H64) <= (2 / 2) * (2 + 2) * 2.0 ** -24 * (1 + 2.0 ** -20) + 2.0 ** -24 * abs(H64) + 1e-9
    # with mu = 0 the gradient is the entropy's alone: it still reaches every parameter through the samples
    model.penalty_parameter = 0.0
    model.zero_grad()
    torch.manual_seed(5)
    L0, H0, _ = model.loss(700)
    assert torch.equal(L0.detach(), H0.detach())
    L0.backward()
    assert any(float(p.grad.abs().max()) > 0 for p in model.parameters())


@pytest.mark.gpu
def test_training_on_the_knn_entropy_alone_raises_the_entropy():
    """mu = 0: the loss is H alone, so a few optimiser steps must raise the entropy of the generator's samples, measured by
    the fp64 restatement on 10 000 fresh samples (a direction check, no threshold on the amount)."""
    from mentflow_amd import _lib
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda", 0)
    prob = small_nn_problem(dev, "knn")
    model = prob.model

    def entropy_now():
        torch.manual_seed(99)
        with torch.no_grad():
            x = model.sample(10000).cpu().numpy()
        return -ref.knn_entropy(x, 5)[0]

    before = entropy_now()
    torch.manual_seed(1)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-2, weight_decay=0.0)
    trainer = mf.train.Trainer(model, opt, verbose=False)
    trainer.train(epochs=1, iterations=30, batch_size=5000, eval_batch_size=5000, penalty_start=0.0, penalty_step=0.0)
    after = entropy_now()
    h = trainer.history
    print(f"k-NN entropy of 10 000 fresh samples: {before:.4f} -> {after:.4f}; H first {h['H'][0]:.4f} last {h['H'][-1]:.4f}")
    assert len(h["L"]) == 30 and all(math.isfinite(v) for v in h["H"])
    assert after > before
