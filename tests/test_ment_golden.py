"""Classical MENT against the reference's own mentflow/ment.py (fixtures from tools/gen_ment_golden.py: scipy's
RegularGridInterpolator, fp32 torch), on the emulator here and on the MI355X with -m gpu.

Gates.  prob: the reference interpolates in fp64 and rounds each factor to fp32, the kernels interpolate in fp32 (~1e-6
relative per factor, see test_ment_kernels.py), products of <= 6 factors: 1e-5 of the largest value.  log_prob must be
log(prob + 1e-12) of that prob, and within 1e-4 of the reference's where prob is at least 1e-2 of its maximum (there a 1e-6
relative error per factor, six factors, is far inside the gate; near a table zero a factor's relative error grows).  Integrate mode draws no random numbers, so the solver's path is exact
data: predictions are fp32 sums of 250 products in the reference (~250 * 2^-24 relative) and fp64 sums here, so 1e-5 of the
largest bin; after an update h = h * (1 + lr (g/g* - 1)) inherits the prediction's relative error amplified by g/g* (<= ~10 on
the populated bins), so the tables are gated at 1e-4 of their largest value."""
import pytest
import torch

import mentflow_amd as mf
from mentflow_amd.ment import MENT


@pytest.mark.parametrize("tag", ["1d", "2d"])
def test_prob_and_log_prob(backend, golden, tag):
    ref = golden("ref_ment_prob")
    mats, tabs = ref[f"mats_{tag}"], ref[f"tables_{tag}"]
    nd = mats.shape[1]
    if tag == "1d":
        diag = mf.diagnostics.Histogram1D(axis=0, edges=ref["edges_1d"]).to(backend)
    else:
        diag = mf.diagnostics.Histogram2D(axis=(0, 2), edges=[ref["edges_2d"], ref["edges_2d"]]).to(backend)
    transforms = [mf.simulate.LinearTransform(m).to(backend) for m in mats]
    model = MENT(ndim=nd, transforms=transforms, diagnostics=[[diag] for _ in transforms],
                 measurements=[[torch.ones_like(t).to(backend)] for t in tabs],
                 prior=mf.prior.Gaussian(ndim=nd, scale=float(ref["prior_scale"])), device=backend)
    assert model.fully_fused()
    for i, t in enumerate(tabs):
        model.lagrange_functions[i][0].set_values(t.to(backend))
    x = ref["x"].to(backend)
    p = model.prob(x).cpu()
    assert float((p - ref[f"prob_{tag}"]).abs().max()) <= 1e-5 * float(ref[f"prob_{tag}"].max())
    lp, lr = model.log_prob(x).cpu(), ref[f"log_prob_{tag}"]
    assert torch.allclose(lp, torch.log(p + 1e-12), rtol=1e-6, atol=1e-6)
    big = ref[f"prob_{tag}"] > 1e-2 * ref[f"prob_{tag}"].max()       # relative error of prob = absolute error of its log
    assert float((lp[big] - lr[big]).abs().max()) <= 1e-4


def test_integrate_gauss_seidel(backend, golden):
    ref = golden("ref_ment_integrate")
    edges = ref["edges"]
    diag = mf.diagnostics.Histogram1D(axis=0, edges=edges).to(backend)
    transforms = [mf.simulate.LinearTransform(m).to(backend) for m in ref["mats"]]
    res = int(ref["res"])
    model = MENT(ndim=2, transforms=transforms, diagnostics=[[diag] for _ in transforms],
                 measurements=[[m.to(backend)] for m in ref["meas"]],
                 prior=mf.prior.Gaussian(ndim=2, scale=float(ref["prior_scale"])), mode="integrate",
                 integration_limits=[[[(-4.0, 4.0)]] for _ in transforms], integration_shape=[[[res]] for _ in transforms],
                 device=backend)
    lr = float(ref["lr"])

    def check_pred(key):
        pred = torch.stack([model.simulate(i, 0).cpu() for i in range(len(transforms))])
        assert float((pred - ref[key]).abs().max()) <= 1e-5 * float(ref[key].max()), key

    def check_h(key):
        h = torch.stack([lf[0].values.cpu() for lf in model.lagrange_functions])
        assert float((h - ref[key]).abs().max()) <= 1e-4 * float(ref[key].max()), key

    check_pred("pred0")
    model.gauss_seidel_update(lr=lr)
    check_h("h1")
    check_pred("pred1")
    model.gauss_seidel_update(lr=lr)
    check_h("h2")
    assert model.epoch == 2
