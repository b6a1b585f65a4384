"""Writes tests/golden/ref_ment_*.npz from the reference's own classical MENT (mentflow/ment.py with scipy).

Needs the reference checkout (REF, as for oracle/gen_golden.py) and scipy; it is not part of any test run.  The fixtures hold
inputs and outputs only:
  ref_ment_prob.npz       prob / log_prob at fixed points: 1-D slots in 4-D (rec_nd_1d-like) and 2-D corner slots in 4-D,
                          tables set to fixed random values, Gaussian prior.
  ref_ment_integrate.npz  2-D linear integrate problem (6 projections, 85 bins, res 250): simulate outputs before the first
                          epoch and after it, and the Lagrange-function tables after 1 and 2 gauss_seidel_update epochs.

    python tools/gen_ment_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import _boot  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def _save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in arrays.items()})
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)")


def main():
    _boot()
    import mentflow.ment as rment
    from mentflow.diagnostics import Histogram1D, Histogram2D
    from mentflow.prior import Gaussian
    from mentflow.simulate import LinearTransform

    g = torch.Generator().manual_seed(20261016)

    # ---- prob / log_prob: 1-D slots in 4-D (rec_nd_1d directions) and 2-D slots (corner transforms) in 4-D
    nd = 4
    dirs = torch.randn(5, nd, generator=g)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    mats1 = []
    for v in dirs:
        M = torch.eye(nd)
        M[0] = v
        mats1.append(M)
    e1 = torch.linspace(-4.0, 4.0, 86)
    tab1 = torch.rand(5, 85, generator=g) * 1.5
    tab1[tab1 < 0.2] = 0.0
    mats2 = []
    for i in range(nd):
        for j in range(i):
            ms = []
            for k, l in zip((0, 2), (j, i)):
                m = torch.eye(nd)
                m[k, k] = m[l, l] = 0.0
                m[k, l] = m[l, k] = 1.0
                ms.append(m)
            mats2.append(torch.linalg.multi_dot(ms[::-1]))
    e2 = torch.linspace(-3.5, 3.5, 31)
    tab2 = torch.rand(len(mats2), 30, 30, generator=g) * 1.5
    x = torch.randn(4000, nd, generator=g) * 1.3
    out = {}
    for tag, mats, diag, tabs in (("1d", mats1, Histogram1D(axis=0, edges=e1), tab1),
                                  ("2d", mats2, Histogram2D(axis=(0, 2), edges=[e2, e2], bandwidth=(0.5, 0.5)), tab2)):
        meas = [[torch.ones_like(t)] for t in tabs]
        model = rment.MENT(ndim=nd, transforms=[LinearTransform(m) for m in mats], diagnostics=[[diag] for _ in mats],
                           measurements=meas, prior=Gaussian(ndim=nd, scale=2.0))
        for i, t in enumerate(tabs):
            model.lagrange_functions[i][0].set_values(t)
        out[f"mats_{tag}"] = torch.stack(mats)
        out[f"tables_{tag}"] = tabs
        out[f"prob_{tag}"] = model.prob(x)
        out[f"log_prob_{tag}"] = model.log_prob(x)
    _save("ref_ment_prob", x=x.numpy(), edges_1d=e1.numpy(), edges_2d=e2.numpy(), prior_scale=np.float32(2.0),
          **{k: v.numpy() for k, v in out.items()})

    # ---- 2-D linear integrate: 6 rotations, 85 bins, res 250, measurements of a two-blob distribution
    angles = np.linspace(0.0, np.pi, 6, endpoint=False)
    mats = [torch.tensor([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]], dtype=torch.float32) for a in angles]
    xt = torch.cat([torch.randn(60000, 2, generator=g) * torch.tensor([0.8, 0.4]) + torch.tensor([0.7, 0.0]),
                    torch.randn(40000, 2, generator=g) * 0.5 - torch.tensor([0.8, 0.6])])
    edges = torch.linspace(-4.0, 4.0, 86)
    diag = Histogram1D(axis=0, edges=edges)
    diag.kde = False
    meas = []
    for m in mats:
        h = diag(xt @ m.T)
        meas.append([h / h.sum() / (edges[1] - edges[0])])
    res = 250
    model = rment.MENT(ndim=2, transforms=[LinearTransform(m) for m in mats], diagnostics=[[diag] for _ in mats],
                       measurements=meas, prior=Gaussian(ndim=2, scale=3.0), mode="integrate",
                       integration_limits=[[[(-4.0, 4.0)]] for _ in mats], integration_shape=[[[res]] for _ in mats])
    pred0 = torch.stack([model.simulate(i, 0) for i in range(len(mats))])
    model.gauss_seidel_update(lr=0.9)
    h1 = torch.stack([lf[0].values for lf in model.lagrange_functions])
    pred1 = torch.stack([model.simulate(i, 0) for i in range(len(mats))])
    model.gauss_seidel_update(lr=0.9)
    h2 = torch.stack([lf[0].values for lf in model.lagrange_functions])
    _save("ref_ment_integrate", mats=torch.stack(mats).numpy(), edges=edges.numpy(),
          meas=torch.stack([m[0] for m in meas]).numpy(), res=np.int64(res), lr=np.float32(0.9), prior_scale=np.float32(3.0),
          pred0=pred0.numpy(), h1=h1.numpy(), pred1=pred1.numpy(), h2=h2.numpy())


if __name__ == "__main__":
    main()
