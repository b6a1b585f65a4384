"""fp64 restatements for the weighted projection tests (tests/test_wproj_*.py), never derived from the code under test.

ref_wkde1d / ref_wkde2d: the dense weighted kernel sums S = sum_n w_n K_n, and for a given gS the gradients of L = sum(gS * S):
gx_n = w_n * (gradient of the unweighted sum) and gw_n = sum gS K_n.  A weight that is not finite and positive counts as 0
(valid64); gw is returned for every row, the tests apply the rule for negative / NaN / infinite weights themselves.
ref_whist1d / ref_whist2d: weighted sums per bin with torch.histogram's rule (out of range ignored, last bin right-inclusive).
normalise_1d / normalise_2d / normalise_hard: the formulas of Histogram1D / Histogram2D with N replaced by W.

The prototype (`python tests/_wproj_fp64.py`): the weighted estimator a MENT with .weighted = True computes in sample mode, in fp64.  The
samplers' prototype of tests/_smc_fp64.py (threshold 0 = annealed importance sampling, 0.5 = sequential Monte Carlo with 8
islands) walks the ladder on cases (a) and (b) of tests/test_ais_api.py with that file's settings; the final states and their
weights w = exp(logw - max logw) go through the weighted 1-D KDE of every view (16 bins on [-4, 4], bandwidth 0.5 bins), and
the result, normalised as MENT.normalize_projection does, is compared with the integrate-mode prediction of the model that
tests/test_ais_api.build makes (mode="integrate" on the grids of integration_grids below: the quantity the test compares with
as well; it is a deterministic quadrature, not the estimator under test).  It prints, per case and sampler, the max-abs
difference over all views and bins for five seeds; tests/test_wproj_api.py gates at about twice the worst."""
import math

import torch


def valid64(w):
    w = w.double()
    return torch.where(torch.isfinite(w) & (w > 0), w, torch.zeros_like(w))


def ref_wkde1d(x, w, V, c, sigma, gS=None, chunk_elems=1 << 23):
    """(S [P,B], gx [n,d] or None, gw [n] or None), fp64 on x's device."""
    x, V, c = x.double(), V.double().to(x.device), c.double().to(x.device)
    wv = valid64(w).to(x.device)
    gS = None if gS is None else gS.double().to(x.device)
    P, B = V.shape[0], c.numel()
    S = torch.zeros(P, B, dtype=torch.float64, device=x.device)
    gx = torch.zeros_like(x) if gS is not None else None
    gw = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device) if gS is not None else None
    step = max(1, chunk_elems // (P * B))
    for a in range(0, x.shape[0], step):
        r = ((x[a:a + step] @ V.T)[:, :, None] - c) / sigma                 # [m, P, B]
        K = torch.exp(-0.5 * r * r)
        K = torch.where(torch.isfinite(K), K, torch.zeros_like(K))          # NaN / inf rows: an empty window
        S += (wv[a:a + step, None, None] * K).sum(0)
        if gS is not None:
            dK = torch.where(K > 0, K * (-r / sigma), torch.zeros_like(K))
            gx[a:a + step] = wv[a:a + step, None] * ((gS * dK).sum(2) @ V)
            gw[a:a + step] = (gS * K).sum((1, 2))
    return S, gx, gw


def ref_wkde2d(x, w, V0, V1, cx, cy, sx, sy, gS=None, chunk_elems=1 << 22):
    x = x.double()
    V0, V1, cx, cy = (t.double().to(x.device) for t in (V0, V1, cx, cy))
    wv = valid64(w).to(x.device)
    gS = None if gS is None else gS.double().to(x.device)
    P, Bx, By = V0.shape[0], cx.numel(), cy.numel()
    S = torch.zeros(P, Bx, By, dtype=torch.float64, device=x.device)
    gx = torch.zeros_like(x) if gS is not None else None
    gw = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device) if gS is not None else None
    step = max(1, chunk_elems // (P * (Bx + By)))
    for a in range(0, x.shape[0], step):
        xa, wa = x[a:a + step], wv[a:a + step]
        rx = ((xa @ V0.T)[:, :, None] - cx) / sx
        ry = ((xa @ V1.T)[:, :, None] - cy) / sy
        Kx, Ky = torch.exp(-0.5 * rx * rx), torch.exp(-0.5 * ry * ry)
        Kx = torch.where(torch.isfinite(rx), Kx, torch.zeros_like(Kx))     # NaN / inf rows: an empty window
        Ky = torch.where(torch.isfinite(ry), Ky, torch.zeros_like(Ky))
        rx, ry = torch.nan_to_num(rx, 0.0, 0.0, 0.0), torch.nan_to_num(ry, 0.0, 0.0, 0.0)
        S += torch.einsum("n,npa,npb->pab", wa, Kx, Ky)
        if gS is not None:
            ax = torch.einsum("npb,pab->npa", Ky, gS)
            du0 = (ax * Kx * (-rx / sx)).sum(2)
            du1 = (torch.einsum("npa,pab->npb", Kx, gS) * Ky * (-ry / sy)).sum(2)
            gx[a:a + step] = wa[:, None] * (du0 @ V0 + du1 @ V1)
            gw[a:a + step] = (ax * Kx).sum((1, 2))
    return S, gx, gw


def _bins(u, e):
    """bin of each u on the edges e (torch.histogram's rule), -1 out of range"""
    B = e.numel() - 1
    k = torch.bucketize(u, e, right=True) - 1
    k = torch.where(u == e[-1], torch.full_like(k, B - 1), k)
    return torch.where((u >= e[0]) & (u <= e[-1]), k, torch.full_like(k, -1))


def ref_whist1d(x, w, V, e):
    """[P,B] fp64.  The projection is formed in fp32 as the kernel forms it (a row on an edge belongs to one side of it)."""
    u = (x.float() @ V.float().T).double()
    wv, e = valid64(w), e.double()
    P, B = V.shape[0], e.numel() - 1
    S = torch.zeros(P, B, dtype=torch.float64)
    for p in range(P):
        k = _bins(u[:, p].contiguous(), e)
        S[p].index_add_(0, k[k >= 0], wv[k >= 0])
    return S


def ref_whist2d(x, w, V0, V1, ex, ey):
    u0, u1 = (x.float() @ V0.float().T).double(), (x.float() @ V1.float().T).double()
    wv, ex, ey = valid64(w), ex.double(), ey.double()
    P, Bx, By = V0.shape[0], ex.numel() - 1, ey.numel() - 1
    S = torch.zeros(P, Bx * By, dtype=torch.float64)
    for p in range(P):
        a, b = _bins(u0[:, p].contiguous(), ex), _bins(u1[:, p].contiguous(), ey)
        ok = (a >= 0) & (b >= 0)
        S[p].index_add_(0, (a * By + b)[ok], wv[ok])
    return S.view(P, Bx, By)


def normalise_1d(S, W, delta):
    prob = S / W
    return prob / (delta * prob.sum(-1, keepdim=True) + 1e-10)


def normalise_2d(S, cell):
    return S / (cell * S.sum((-2, -1), keepdim=True) + 1e-10)


def normalise_hard(S, widths):
    return S / S.sum(tuple(range(1, S.dim())), keepdim=True) / widths


# --------------------------------------------------------------------------------------------------------- the prototype
def weighted_prediction64(x, logw, rows, edges, bandwidth_bins=0.5):
    """[views, B]: the weighted 1-D KDE of every view from states x and log-weights logw, normalised as MENT does."""
    c = 0.5 * (edges[1:] + edges[:-1]).double()
    delta = float(edges[1] - edges[0])
    w = torch.exp(logw - logw.max())
    V = torch.stack([r.double() for r in rows])
    S, _, _ = ref_wkde1d(x, w, V, c, bandwidth_bins * delta)
    g = normalise_1d(S, valid64(w).sum(), delta)
    return g / g.sum(1, keepdim=True) / delta


def integration_grids(model, case):
    """Integrate mode for the models of tests/test_ais_api.build: [-4, 4] on every axis that is integrated out, 257 nodes for
    the one such axis of case (a), 5 per axis for the five of case (b) (its density factorises, so a view's normalised
    prediction does not depend on how finely the other axes are summed: -2, 0 and 2 lie inside the support)."""
    n_int = model.ndim - 1
    shape = (257,) if case == "a" else (5,) * n_int
    model.integration_limits = [[[(-4.0, 4.0)] * n_int] for _ in model.transforms]
    model.integration_shape = [[shape] for _ in model.transforms]
    return model


def _main():
    """Cases (a), (b) of tests/test_ais_api.py: max |weighted estimate - integrate-mode prediction| over five seeds."""
    from _smc_fp64 import SmcPrototype
    from test_ais_api import EDGES, SETTINGS, build, rows_of
    prior = ("gaussian", 3.0)
    for case in ("a", "b"):
        model, slots = build(case, torch.device("cpu"))
        integration_grids(model, case)
        d = 2 if case == "a" else 6
        ref = torch.stack([model._simulate_integrate(i, 0).double() for i in range(len(slots))])
        for name, thr, groups in (("ais", 0.0, 1), ("smc", 0.5, 8)):
            worst = []
            for seed in range(5):
                p = SmcPrototype(slots, prior, d, chains=SETTINGS["chains"], groups=groups, n_temps=SETTINGS["n_temps"],
                                 spt=SETTINGS["steps_per_temp"], step=SETTINGS["step"], clip=SETTINGS["drift_clip"],
                                 base=SETTINGS["base_scale"], threshold=thr, seed=seed)
                p.run()
                pred = weighted_prediction64(p.x, p.logw, rows_of(case), EDGES)
                worst.append(float((pred - ref).abs().max()))
            print(f"case {case}, {name}: max |d prediction| per seed " + " ".join(f"{v:.4f}" for v in worst)
                  + f"   worst {max(worst):.4f}   (largest predicted density {float(ref.max()):.3f})")


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from conftest import EMU_LIB
    from mentflow_amd import _lib
    _lib.use_library(EMU_LIB)            # the integrate-mode reference is the emulated model's own prediction
    _main()
