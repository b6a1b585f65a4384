"""The histogram half of the step, element by element against fp64 on the launch paths of mentflow_amd/csrc/kde.hip:
projection + KDE forward / backward (1-D and 2-D), the fixed-point accumulation, clipped windows and non-finite rows,
hard-binned counts, the normalisation + discrepancy tail, the fused loss with MAE / MSE, the entropy sums and the two
small helpers (mf_scale_rows, mf_gather_f32).  Non-uniform bin edges, which the KDE kernels cannot take, are checked
through Histogram1D / Histogram2D and MENTFlow.loss (dense evaluation, mentflow_amd/diagnostics/diagnostics.py).

Every reference is plain fp64 torch written from the reference's formulas (histogram.py:11-74, loss.py:7-17,
entropy.py:58-62).  Every KDE case carries the launch path it is there for as a literal, which is also its parameter id:
fwd<block>/Pg<projections per group>xG<groups>/w<particles per workgroup>/sh<kde_global_shift>,
bwd<block>/ch<lanes per particle> (1-D) or bwd<block>/npt<particles per thread> (2-D), and the window variant
(fact = factorised radius-4 window, rt<R> = run-time radius R).  Before a case runs its kernels it asserts that the
loaded library plans exactly that path for it (ops.kde_plan -> mf_proj_kde_plan, the host code the launchers themselves
run: mentflow_amd/csrc/kde_plan.h), and test_case_lists_cover_the_launch_paths states what the lists cover: a threshold
that moves in kde_plan.h fails one of the two.

Gates (the suite's): histograms rtol 2e-5 + atol 1e-6; particle gradients rtol 1e-3 + atol 2e-5 max|g| + 1e-6; counts
and a saturated centre bin exact.

The CPU suite runs the emulated build up to 300 000 particles (the emulator takes well under a second per launch
there); `-m gpu` repeats A-C on the MI355X at 70 001 / 300 000 / 2 097 152 particles (and 16 M for the shift-11
accumulator), with the fp64 reference computed on the GPU in chunks.  Only those gpu-marked lists reach forward
workgroups of more particles than threads (the multi-iteration particle loop: w2048 .. w8192), the 1024-thread 2-D
backward with 1, 2 and 4 particles per thread, and shift 11; every emulated forward workgroup takes one particle per
thread."""
import math
import re

import numpy as np
import pytest
import torch

import mentflow_amd as mf
from mentflow_amd import _lib, ops
from mentflow_amd._lib import call, ptr, stream_ptr
from oracle import model as om

RTOL_S, ATOL_S = 2e-5, 1e-6


# ------------------------------------------------------------------------------------------------ launch paths
# The path the LOADED library plans for a case (ops.kde_plan: the launchers' own host code), in the format of the literals
# the case lists carry.
def _path_1d(n, P, B, bw):
    R = ops.kde_radius(bw)
    f, b = ops.kde_plan("kde1d_fwd", n, P, B, radius_x=R), ops.kde_plan("kde1d_bwd", n, P, B, radius_x=R)
    assert f["window"] == b["window"]
    Pg, G = f["Pg"], f["groups"]
    last = P - (G - 1) * Pg
    win = "fact" if f["window"] == 4 else f"rt{R}"
    return (f"fwd{f['block']}/Pg{Pg}x{G}{'' if last == Pg else f'(last{last})'}/w{f['per_wg']}/sh{f['shift']}"
            f"-bwd{b['block']}/ch{b['split']}-{win}")


def _path_2d(n, P, Bx, By, bwx, bwy):
    rx, ry = ops.kde_radius(bwx), ops.kde_radius(bwy)
    f, b = ops.kde_plan("kde2d_fwd", n, P, Bx, By, rx, ry), ops.kde_plan("kde2d_bwd", n, P, Bx, By, rx, ry)
    assert f["window"] == b["window"]
    win = "fact" if f["window"] == 4 else f"rt{rx}x{ry}"
    return (f"fwd{f['block']}/Pg{f['Pg']}x{f['groups']}/w{f['per_wg']}/sh{f['shift']}"
            f"-bwd{b['block']}/npt{b['split']}/Pg{b['Pg']}-{win}")


def _fixed_point_plan(n):
    """Forward plan of _centre_case_1d / _far_tail_case: one projection, 64 bins."""
    return ops.kde_plan("kde1d_fwd", n, 1, 64)


# ------------------------------------------------------------------------------------------------ fp64 references
def _grid(lo, hi, B):
    e = torch.linspace(lo, hi, B + 1)
    return e, 0.5 * (e[1:] + e[:-1]), float(e[1] - e[0])


def _dirs(P, d, gen):
    V = torch.randn(P, d, generator=gen)
    return V / V.norm(dim=1, keepdim=True)


def ref_kde1d(x, V, c, sigma, gS=None, chunk_elems=1 << 23):
    """S[p,k] = sum_n exp(-((x_n.V_p - c_k) / sigma)^2 / 2) and, with gS, dL/dx for L = sum(gS * S): fp64 on x's device."""
    x, V, c = x.double(), V.double().to(x.device), c.double().to(x.device)
    gS = None if gS is None else gS.double().to(x.device)
    P, B = V.shape[0], c.numel()
    S = torch.zeros(P, B, dtype=torch.float64, device=x.device)
    gx = torch.zeros_like(x) if gS is not None else None
    step = max(1, chunk_elems // (P * B))
    for a in range(0, x.shape[0], step):
        r = ((x[a:a + step] @ V.T)[:, :, None] - c) / sigma                 # [m, P, B]
        K = torch.exp(-0.5 * r * r)
        S += K.sum(0)
        if gS is not None:
            gx[a:a + step] = (gS * K * (-r / sigma)).sum(2) @ V
    return S, gx


def ref_kde2d(x, V0, V1, cx, cy, sx, sy, gS=None, chunk_elems=1 << 22):
    x = x.double()
    V0, V1, cx, cy = (t.double().to(x.device) for t in (V0, V1, cx, cy))
    gS = None if gS is None else gS.double().to(x.device)
    P, Bx, By = V0.shape[0], cx.numel(), cy.numel()
    S = torch.zeros(P, Bx, By, dtype=torch.float64, device=x.device)
    gx = torch.zeros_like(x) if gS is not None else None
    step = max(1, chunk_elems // (P * (Bx + By)))
    for a in range(0, x.shape[0], step):
        xa = x[a:a + step]
        rx = ((xa @ V0.T)[:, :, None] - cx) / sx
        ry = ((xa @ V1.T)[:, :, None] - cy) / sy
        Kx, Ky = torch.exp(-0.5 * rx * rx), torch.exp(-0.5 * ry * ry)
        S += torch.einsum("npa,npb->pab", Kx, Ky)
        if gS is not None:
            du0 = (torch.einsum("npb,pab->npa", Ky, gS) * Kx * (-rx / sx)).sum(2)
            du1 = (torch.einsum("npa,pab->npb", Kx, gS) * Ky * (-ry / sy)).sum(2)
            gx[a:a + step] = du0 @ V0 + du1 @ V1
    return S, gx


def assert_hist(S, So):
    torch.testing.assert_close(S.detach().double().cpu(), So.detach().cpu(), rtol=RTOL_S, atol=ATOL_S)


def assert_grad(g, go):
    go = go.detach().cpu()
    torch.testing.assert_close(g.detach().double().cpu(), go, rtol=1e-3, atol=2e-5 * float(go.abs().max()) + 1e-6)


# ------------------------------------------------------------------------------------------------ C ABI calls
def kde1d_fwd(x, V, c, sigma, R):
    return ops.ProjKde1dFn.apply(x, V, c, sigma, R)


def kde1d_bwd(x, V, c, sigma, R, gS, gx, accumulate):
    call("mf_proj_kde1d_bwd", ptr(x), x.shape[0], x.shape[1], ptr(V), V.shape[0], ptr(c), c.numel(), float(sigma), int(R),
         ptr(gS.contiguous()), ptr(gx), int(accumulate), stream_ptr(x))
    return gx


def kde2d_bwd(x, V0, V1, cx, cy, sx, sy, rx, ry, gS, gx, accumulate):
    call("mf_proj_kde2d_bwd", ptr(x), x.shape[0], x.shape[1], ptr(V0), ptr(V1), V0.shape[0], ptr(cx), cx.numel(),
         float(sx), int(rx), ptr(cy), cy.numel(), float(sy), int(ry), ptr(gS.contiguous()), ptr(gx), int(accumulate),
         stream_ptr(x))
    return gx


# ================================================================================================ A. 1-D KDE
def _run_1d(dev, n, d, P, B, bw, path, seed, lo=-3.0, hi=3.0):
    assert _path_1d(n, P, B, bw) == path
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=gen) * 1.2
    V = _dirs(P, d, gen)
    _, c, delta = _grid(lo, hi, B)
    sigma, R = bw * delta, ops.kde_radius(bw)
    gS = torch.randn(P, B, generator=gen)
    g0 = torch.randn(n, d, generator=gen)
    xd, Vd, cd = x.to(dev), V.to(dev), c.to(dev)
    S = kde1d_fwd(xd, Vd, cd, sigma, R)
    So, go = ref_kde1d(xd, V, c, sigma, gS)
    assert_hist(S, So)
    for acc in (0, 1):
        gx = g0.to(dev).clone() if acc else torch.full((n, d), float("nan")).to(dev)
        kde1d_bwd(xd, Vd, cd, sigma, R, gS.to(dev), gx, acc)
        assert_grad(gx, go + g0.double().to(go.device) if acc else go)


# (n, d, P, B, bandwidth in bins, launch path): every window variant (bw 0.5: radius-4 factorised; 0.3 / 0.6: run-time
# radius 3 / 5; 0.12: radius 1), CH 1 / 2 / 4 / 8 through P, several projection groups with an uneven last one (P = 5, 9,
# 101), d = 1 .. 8
CASES_1D = [
    (300, 1, 1, 64, 0.5, "fwd256/Pg1x1/w256/sh0-bwd256/ch1-fact"),
    (257, 2, 2, 33, 0.3, "fwd256/Pg2x1/w256/sh0-bwd256/ch2-rt3"),
    (300, 3, 5, 40, 0.6, "fwd256/Pg4x2(last1)/w256/sh0-bwd256/ch4-rt5"),
    (150, 4, 9, 50, 0.12, "fwd256/Pg4x3(last1)/w256/sh0-bwd256/ch8-rt1"),
    (200, 5, 101, 85, 0.5, "fwd256/Pg4x26(last1)/w256/sh0-bwd256/ch8-fact"),
    (400, 6, 101, 85, 0.3, "fwd256/Pg4x26(last1)/w256/sh0-bwd256/ch8-rt3"),
    (129, 7, 3, 17, 0.45, "fwd256/Pg3x1/w256/sh0-bwd256/ch2-fact"),
    (513, 8, 16, 128, 0.6, "fwd256/Pg4x4/w256/sh0-bwd256/ch8-rt5"),
    # large-batch branch on the emulator: 1024-thread forward, one particle per thread (w1024: workgroups of more
    # particles than threads run in GPU_1D only), shift > 0 and two groups of 51 / 50 projections; 512-thread backward
    # blocks at 300 000
    (70001, 6, 101, 85, 0.5, "fwd1024/Pg51x2(last50)/w1024/sh4-bwd256/ch4-fact"),
    (300000, 6, 4, 85, 0.3, "fwd1024/Pg4x1/w1024/sh6-bwd512/ch2-rt3"),
]


def _params_1d(cases):
    return [pytest.param(*c, id=f"n{c[0]}-d{c[1]}-P{c[2]}-B{c[3]}-bw{c[4]}:{c[5]}") for c in cases]


@pytest.mark.parametrize("n,d,P,B,bw,path", _params_1d(CASES_1D))
def test_kde1d_vs_fp64(backend, n, d, P, B, bw, path):
    _run_1d(backend, n, d, P, B, bw, path, seed=n + 7 * d)


# ================================================================================================ B. 2-D KDE
def _run_2d(dev, n, d, P, Bx, By, bwx, bwy, path, seed):
    assert _path_2d(n, P, Bx, By, bwx, bwy) == path
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=gen)
    V0, V1 = _dirs(P, d, gen), _dirs(P, d, gen)
    _, cx, dx = _grid(-3.0, 3.0, Bx)
    _, cy, dy = _grid(-2.5, 2.7, By)
    sx, sy, rx, ry = bwx * dx, bwy * dy, ops.kde_radius(bwx), ops.kde_radius(bwy)
    gS = torch.randn(P, Bx, By, generator=gen)
    g0 = torch.randn(n, d, generator=gen)
    xd = x.to(dev)
    args = (V0.to(dev), V1.to(dev), cx.to(dev), cy.to(dev))
    S = ops.ProjKde2dFn.apply(xd, *args, sx, sy, rx, ry)
    So, go = ref_kde2d(xd, V0, V1, cx, cy, sx, sy, gS)
    assert_hist(S, So)
    for acc in (0, 1):
        gx = g0.to(dev).clone() if acc else torch.full((n, d), float("nan")).to(dev)
        kde2d_bwd(xd, *args, sx, sy, rx, ry, gS.to(dev), gx, acc)
        assert_grad(gx, go + g0.double().to(go.device) if acc else go)


# (n, d, P, Bx, By, bwx, bwy, launch path): Bx != By; both axes factorised (s = 2 and 2.22); one axis factorised, the
# other at a run-time radius (3 or 5); 85 x 85 images (one projection per group); d = 1 .. 8
CASES_2D = [
    (300, 3, 3, 40, 24, 0.5, 0.5, "fwd1024/Pg3x1/w1024/sh0-bwd256/npt1/Pg3-fact"),
    (257, 2, 2, 31, 45, 0.45, 0.5, "fwd1024/Pg2x1/w1024/sh0-bwd256/npt1/Pg2-fact"),
    (200, 4, 3, 33, 20, 0.5, 0.3, "fwd1024/Pg3x1/w1024/sh0-bwd256/npt1/Pg3-rt4x3"),
    (150, 5, 2, 24, 36, 0.6, 0.5, "fwd1024/Pg2x1/w1024/sh0-bwd256/npt1/Pg2-rt5x4"),
    (120, 6, 3, 85, 85, 0.5, 0.5, "fwd1024/Pg1x3/w1024/sh0-bwd256/npt1/Pg1-fact"),
    (100, 1, 2, 85, 85, 0.3, 0.6, "fwd1024/Pg1x2/w1024/sh0-bwd256/npt1/Pg1-rt3x5"),
    (90, 7, 5, 16, 11, 0.5, 0.5, "fwd1024/Pg5x1/w1024/sh0-bwd256/npt1/Pg5-fact"),
    (77, 8, 4, 12, 29, 0.45, 0.3, "fwd1024/Pg4x1/w1024/sh0-bwd256/npt1/Pg4-rt4x3"),
    # the large-batch launch shapes of the backward on the emulator: 512-thread blocks at 300 000 particles
    (70001, 6, 3, 85, 85, 0.5, 0.5, "fwd1024/Pg1x3/w1024/sh4-bwd256/npt1/Pg1-fact"),
    (300000, 4, 2, 40, 24, 0.5, 0.3, "fwd1024/Pg2x1/w1024/sh6-bwd512/npt1/Pg2-rt4x3"),
]


def _params_2d(cases):
    return [pytest.param(*c, id=f"n{c[0]}-d{c[1]}-P{c[2]}-{c[3]}x{c[4]}-bw{c[5]}x{c[6]}:{c[7]}") for c in cases]


@pytest.mark.parametrize("n,d,P,Bx,By,bwx,bwy,path", _params_2d(CASES_2D))
def test_kde2d_vs_fp64(backend, n, d, P, Bx, By, bwx, bwy, path):
    _run_2d(backend, n, d, P, Bx, By, bwx, bwy, path, seed=n + 11 * d)


# ================================================================================================ C. fixed point
def _centre_case_1d(dev, n, B=64, k0=20):
    _, c, delta = _grid(-4.0, 4.0, B)
    sigma = 0.5 * delta
    x = c[k0].repeat(n, 1).to(dev)                                       # d = 1, V = [1]: u is the bin centre exactly
    S = kde1d_fwd(x, torch.ones(1, 1).to(dev), c.to(dev), sigma, 4)[0].cpu()
    assert float(S[k0]) == float(n), (float(S[k0]), n)                   # weight 1 = 2^50 units: exact at every level
    c64 = c.double()
    for k in (k0 - 1, k0 + 1, k0 - 2, k0 + 2):         # n e^-2 and n e^-8 (bin width 1/8: every centre exact)
        want = n * math.exp(-0.5 * ((float(c64[k]) - float(c64[k0])) / sigma) ** 2)
        assert abs(float(S[k]) - want) <= 2e-6 * want, (k, float(S[k]), want)


def _centre_case_2d(dev, n, Bx=40, By=24, ka=17, kb=9):
    _, cx, dx = _grid(-3.0, 3.0, Bx)
    _, cy, dy = _grid(-2.0, 2.0, By)
    sx, sy = 0.5 * dx, 0.5 * dy
    x = torch.tensor([[float(cx[ka]), float(cy[kb])]]).repeat(n, 1).to(dev)
    V0, V1 = torch.tensor([[1.0, 0.0]]).to(dev), torch.tensor([[0.0, 1.0]]).to(dev)
    S = ops.ProjKde2dFn.apply(x, V0, V1, cx.to(dev), cy.to(dev), sx, sy, 4, 4)[0].cpu()
    assert float(S[ka, kb]) == float(n)
    for i, j in ((1, 0), (0, 1), (-1, -1), (1, -1), (-1, 0)):
        want = n * math.exp(-0.5 * (((float(cx[ka + i]) - float(cx[ka])) / sx) ** 2 + ((float(cy[kb + j]) - float(cy[kb])) / sy) ** 2))
        assert abs(float(S[ka + i, kb + j]) - want) <= 2e-6 * want, (i, j, float(S[ka + i, kb + j]), want)


def _far_tail_case(dev, n, seed):
    """Every bin whose fp64 value is >= 1e-10 of the peak within 1e-4 relative (its log enters the KL loss); the grid
    reaches 8 sigma of the cloud so that the outer bins hold only far-tail weights."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 1, generator=gen)
    _, c, delta = _grid(-8.0, 8.0, 64)
    S = kde1d_fwd(x.to(dev), torch.ones(1, 1).to(dev), c.to(dev), 0.5 * delta, 4)[0]
    So, _ = ref_kde1d(x.to(dev), torch.ones(1, 1), c, 0.5 * delta)
    So = So[0].cpu()
    keep = So >= 1e-10 * So.max()
    assert int(keep.sum()) < 64                                          # some bins do fall below the cut
    rel = ((S.cpu().double() - So).abs() / So)[keep]
    assert float(rel.max()) <= 1e-4, (float(rel.max()), So[keep].min())


FIXED_POINT = [(8192, "sh0"), (8193, "sh1")]


@pytest.mark.parametrize("n,path", [pytest.param(n, p, id=f"n{n}-{p}") for n, p in FIXED_POINT])
def test_fixed_point_centre_bin_exact(backend, n, path):
    assert f"sh{_fixed_point_plan(n)['shift']}" == path
    _centre_case_1d(backend, n)
    _centre_case_2d(backend, n)
    _far_tail_case(backend, n, seed=n)


# ================================================================================================ D. input edges
def test_clipped_windows_at_both_ends(backend):
    """Particles on, just inside and far beyond the first and last bin centres (windows clipped at either end), 1-D and
    2-D, forward and backward, against the dense fp64 sum."""
    _, c, delta = _grid(-3.0, 3.0, 40)
    c0, c1 = float(c[0]), float(c[-1])
    vals = [c0, c0 + 1e-3 * delta, c0 + 0.49 * delta, c0 - 0.51 * delta, c0 - 2 * delta, c0 - 4.4 * delta, c0 - 6 * delta,
            c0 - 1e6, c1, c1 - 1e-3 * delta, c1 - 0.5 * delta, c1 + 0.5 * delta, c1 + 3.7 * delta, c1 + 5 * delta, 1e6, 0.0]
    u = torch.tensor(vals)
    gen = torch.Generator().manual_seed(3)
    for bw in (0.5, 0.3):
        x = torch.stack([u, u.flip(0)], dim=1)
        V = torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.6, 0.8]])
        gS = torch.randn(3, 40, generator=gen)
        xd = x.to(backend)
        S = kde1d_fwd(xd, V.to(backend), c.to(backend), bw * delta, ops.kde_radius(bw))
        So, go = ref_kde1d(xd, V, c, bw * delta, gS)
        assert_hist(S, So)
        gx = kde1d_bwd(xd, V.to(backend), c.to(backend), bw * delta, ops.kde_radius(bw), gS.to(backend),
                       torch.empty_like(xd), 0)
        assert_grad(gx, go)
        gS2 = torch.randn(3, 40, 40, generator=gen)
        args = (V.to(backend), V.flip(0).to(backend), c.to(backend), c.to(backend))
        S2 = ops.ProjKde2dFn.apply(xd, *args, bw * delta, bw * delta, ops.kde_radius(bw), ops.kde_radius(bw))
        S2o, g2o = ref_kde2d(xd, V, V.flip(0), c, c, bw * delta, bw * delta, gS2)
        assert_hist(S2, S2o)
        g2 = kde2d_bwd(xd, *args, bw * delta, bw * delta, ops.kde_radius(bw), ops.kde_radius(bw), gS2.to(backend),
                       torch.empty_like(xd), 0)
        assert_grad(g2, g2o)


def test_nonfinite_rows_contribute_nothing_to_the_forward(backend):
    """centre_bin (kde.hip) clamps a NaN / +-inf projection so that its window is empty: such a row adds nothing to any
    bin, the finite rows match fp64 exactly as without it (the backward's counterpart is tested elsewhere)."""
    gen = torch.Generator().manual_seed(9)
    n, d, P = 300, 4, 5
    x = torch.randn(n, d, generator=gen)
    bad = [0, 17, 64, 150, 299]
    x[0, 1], x[17, 0], x[64, 3], x[150, :] = float("nan"), float("inf"), float("-inf"), float("nan")
    x[299, 2] = float("inf")
    x[299, 0] = float("-inf")
    good = torch.ones(n, dtype=torch.bool)
    good[bad] = False
    V0, V1 = _dirs(P, d, gen), _dirs(P, d, gen)
    _, c, delta = _grid(-3.0, 3.0, 48)
    for bw in (0.5, 0.3):
        R = ops.kde_radius(bw)
        S = kde1d_fwd(x.to(backend), V0.to(backend), c.to(backend), bw * delta, R)
        So, _ = ref_kde1d(x[good].to(backend), V0, c, bw * delta)
        assert torch.isfinite(S).all()
        assert_hist(S, So)
        S2 = ops.ProjKde2dFn.apply(x.to(backend), V0.to(backend), V1.to(backend), c.to(backend), c.to(backend), bw * delta,
                                   bw * delta, R, R)
        S2o, _ = ref_kde2d(x[good].to(backend), V0, V1, c, c, bw * delta, bw * delta)
        assert torch.isfinite(S2).all()
        assert_hist(S2, S2o)


# non-uniform probe grids: 6 coarse bins on [-3, 0] then 24 fine ones on [0, 3]; a cubic grid
def _graded_1d():
    return torch.cat([torch.linspace(-3.0, 0.0, 7)[:-1], torch.linspace(0.0, 3.0, 25)])


def _cubic():
    return torch.linspace(-3.0, 3.0, 9) ** 3 / 9.0


def _ref_hist1d(u, edges, bw):
    """kde_histogram_1d (histogram.py:77-86, marginal_pdf :11-44) in fp64."""
    e = edges.double()
    c = 0.5 * (e[1:] + e[:-1])
    sigma = bw * (e[1] - e[0])
    prob = torch.exp(-0.5 * ((u.double()[:, None] - c) / sigma) ** 2).mean(0)
    return prob / ((prob * (c[1] - c[0])).sum() + 1e-10)


def _ref_hist2d(ux, uy, ex, ey, bwx, bwy):
    """kde_histogram_2d (histogram.py:89-101, joint_pdf :47-74) in fp64."""
    ex, ey = ex.double(), ey.double()
    cx, cy = 0.5 * (ex[1:] + ex[:-1]), 0.5 * (ey[1:] + ey[:-1])
    kx = torch.exp(-0.5 * ((ux.double()[:, None] - cx) / (bwx * (ex[1] - ex[0]))) ** 2)
    ky = torch.exp(-0.5 * ((uy.double()[:, None] - cy) / (bwy * (ey[1] - ey[0]))) ** 2)
    prob = kx.T @ ky
    return prob / ((prob * (cx[1] - cx[0]) * (cy[1] - cy[0])).sum() + 1e-10)


def test_uniform_axis_detection():
    """fp32 linspace grids far from the origin are uniform (the kernels take them); the graded probes are not."""
    from mentflow_amd.diagnostics.diagnostics import is_uniform_axis
    assert is_uniform_axis(torch.linspace(997.0, 1003.0, 65))
    assert is_uniform_axis(torch.linspace(996.7, 1003.1, 86))
    assert is_uniform_axis(torch.linspace(-3.3, 2.9, 86))
    assert not is_uniform_axis(_graded_1d())
    assert not is_uniform_axis(_cubic())
    assert mf.diagnostics.Histogram1D(edges=torch.linspace(997.0, 1003.0, 65)).uniform
    assert not mf.diagnostics.Histogram1D(edges=_graded_1d()).uniform
    assert not mf.diagnostics.Histogram2D(axis=(0, 1), edges=(torch.linspace(-3, 3, 33), _cubic())).uniform


@pytest.mark.parametrize("offset", [0.0, 1000.0])
def test_histograms_on_uniform_grids_far_from_the_origin(backend, offset):
    """Uniform fp32 grids at the origin and 1000 away take the kernels and match the dense fp64 formula."""
    gen = torch.Generator().manual_seed(4)
    u = torch.randn(400, 2, generator=gen) + offset
    e = torch.linspace(offset - 3.0, offset + 3.0, 65)
    h = mf.diagnostics.Histogram1D(edges=e, bandwidth=0.5, axis=0).to(backend)
    out = h(u.to(backend))
    ref = _ref_hist1d(u[:, 0], e, 0.5)
    assert float((out.cpu().double() - ref).abs().max() / ref.max()) < 1e-6


def test_nonuniform_grid_histogram1d(backend):
    gen = torch.Generator().manual_seed(1)
    u = torch.randn(400, 1, generator=gen)
    e = _graded_1d()
    h = mf.diagnostics.Histogram1D(edges=e, bandwidth=0.5, axis=0).to(backend)
    ud = u.to(backend).clone().requires_grad_(True)
    out = h(ud)
    w = torch.randn(e.numel() - 1, generator=gen)
    (out * w.to(backend)).sum().backward()
    uo = u.double().clone().requires_grad_(True)
    ref = _ref_hist1d(uo[:, 0], e, 0.5)
    (ref * w.double()).sum().backward()
    err = float((out.detach().cpu().double() - ref.detach()).abs().max() / ref.detach().max())
    assert err < 1e-5, err
    assert_grad(ud.grad, uo.grad)


def test_nonuniform_grid_histogram2d(backend):
    gen = torch.Generator().manual_seed(2)
    u = torch.randn(400, 3, generator=gen)
    ex, ey = torch.linspace(-3.0, 3.0, 33), _cubic()
    h = mf.diagnostics.Histogram2D(axis=(0, 2), edges=(ex, ey), bandwidth=(0.5, 0.5)).to(backend)
    ud = u.to(backend).clone().requires_grad_(True)
    out = h(ud)
    w = torch.randn(32, 8, generator=gen)
    (out * w.to(backend)).sum().backward()
    uo = u.double().clone().requires_grad_(True)
    ref = _ref_hist2d(uo[:, 0], uo[:, 2], ex, ey, 0.5, 0.5)
    (ref * w.double()).sum().backward()
    err = float((out.detach().cpu().double() - ref.detach()).abs().max() / ref.detach().max())
    assert err < 1e-5, err
    assert_grad(ud.grad, uo.grad)


def _loss_vs_oracle(backend, diags_mf, diags_om, disc_mf, disc_om, n=600, d=4, T=3, seed=0, expect_fused=True):
    """MENTFlow.loss (L, H, D, dL/dx, dL/dlog_prob) vs oracle.model.mentflow_loss in fp64, gates of _loss_case
    (tests/test_kernels_golden.py)."""
    from test_kernels_golden import Injected, close
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.randn(n, d, generator=gen)
    lp0 = torch.randn(n, generator=gen) - 3.0
    mats = [torch.linalg.qr(torch.randn(d, d, generator=gen))[0] for _ in range(T)]
    xm = torch.randn(5000, d, generator=gen) * 0.8 + 0.2
    meas = []
    for M in mats:
        h = diags_om(xm @ M.T)
        meas.append([h.float()])
    prior = mf.prior.Gaussian(d, 1.0)
    for mu in (0.0, 50.0):
        x = x0.to(backend).clone().requires_grad_(True)
        lp = lp0.to(backend).clone().requires_grad_(True)
        transforms = [mf.simulate.LinearTransform(M).to(backend) for M in mats]
        model = mf.MENTFlow(transforms=transforms, diagnostics=[[diags_mf] for _ in mats],
                            measurements=[[m[0].to(backend)] for m in meas], generator=Injected(x, lp), prior=prior,
                            entropy_estimator=mf.entropy.MonteCarloEntropyEstimator(prior=prior),
                            discrepancy_function=disc_mf, penalty_parameter=mu)
        L, H, D = model.loss(n)
        L.backward()
        xo = x0.double().clone().requires_grad_(True)
        lo = lp0.double().clone().requires_grad_(True)
        Lo, Ho, Do = om.mentflow_loss(xo, lo, [om.LinearTransform(M.double()) for M in mats],
                                      [[diags_om] for _ in mats], [[m[0].double()] for m in meas],
                                      om.GaussianPrior(d, 1.0, dtype=torch.float64), mu, disc_om)
        Lo.backward()
        close(H, Ho.detach().float(), 1e-5, 1e-6)
        close(torch.stack(D), torch.stack(Do).detach().float(), 2e-4, 1e-7)
        close(L, Lo.detach().float(), 2e-5, 1e-5 + mu * 1e-6)
        gmax = float(xo.grad.abs().max())
        close(x.grad, xo.grad.float(), 1e-3, 2e-5 * gmax)
        close(lp.grad, lo.grad.float(), 1e-6, 1e-9)
        assert (model._fused_plan() is not None) == expect_fused


def test_nonuniform_grids_through_mentflow_loss(backend):
    """Non-uniform edges leave the fused plan (generic loop, dense sums) and the loss matches the oracle."""
    e1 = _graded_1d()
    _loss_vs_oracle(backend, mf.diagnostics.Histogram1D(edges=e1, bandwidth=0.5, axis=0).to(backend),
                    om.Histogram1D(edges=e1.double(), bandwidth=0.5, axis=0), mf.loss.kl_divergence, om.kl_divergence,
                    expect_fused=False)
    ex, ey = torch.linspace(-3.0, 3.0, 33), _cubic()
    _loss_vs_oracle(backend, mf.diagnostics.Histogram2D(axis=(0, 2), edges=(ex, ey)).to(backend),
                    om.Histogram2D(axis=(0, 2), edges=(ex.double(), ey.double())), mf.loss.kl_divergence,
                    om.kl_divergence, expect_fused=False, seed=1)


# ================================================================================================ E. hard counts
def _edge_values(e):
    """Every edge, one ulp either side of it, one ulp outside both ends, and the midpoints."""
    e = e.float()
    inf = torch.tensor(float("inf"))
    vals = [e, torch.nextafter(e, inf), torch.nextafter(e, -inf), 0.5 * (e[1:] + e[:-1])]
    return torch.cat(vals)


@pytest.mark.parametrize("kind", ["uniform", "graded", "cubic"])
def test_hard_counts_bit_exact(backend, kind):
    e = {"uniform": torch.linspace(-3.0, 3.0, 25), "graded": _graded_1d(), "cubic": _cubic()}[kind]
    v = _edge_values(e)
    gen = torch.Generator().manual_seed(5)
    v = torch.cat([v, torch.randn(500, generator=gen) * 2.0])
    d = 3
    x = torch.randn(v.numel(), d, generator=gen)
    x[:, 1] = v
    V = torch.zeros(2, d)
    V[0, 1] = 1.0                                  # u = x[:, 1] exactly (fma with zeros)
    V[1, 2] = 1.0
    counts = ops.proj_hist_counts_1d(x.to(backend), V.to(backend), e.to(backend)).cpu()
    for p, col in ((0, 1), (1, 2)):
        ref = torch.histogram(x[:, col], e).hist
        assert torch.equal(counts[p].to(torch.float32), ref), (p, counts[p], ref)
    assert int(counts[0].sum()) == int(((v >= e[0]) & (v <= e[-1])).sum())
    # 2-D: against np.histogramdd on the same projections
    ey = torch.linspace(-2.0, 2.5, 12) if kind == "uniform" else _cubic()
    x[:, 2] = torch.cat([_edge_values(ey), torch.randn(v.numel() - _edge_values(ey).numel(), generator=gen)])
    V0 = torch.zeros(1, d)
    V1 = torch.zeros(1, d)
    V0[0, 1], V1[0, 2] = 1.0, 1.0
    c2 = ops.proj_hist_counts_2d(x.to(backend), V0.to(backend), V1.to(backend), e.to(backend), ey.to(backend)).cpu()
    ref2, _ = np.histogramdd(x[:, 1:3].numpy(), bins=[e.numpy(), ey.numpy()])
    assert np.array_equal(c2[0].numpy(), ref2.astype(np.int32))


# ================================================================================================ F. tail kernel
def _ref_tail(S, meas, normalize, pre_scale, cell, eps, kind, pad, div):
    S = S.double()
    if normalize:
        t = S * pre_scale
        g = t / (t.sum(1, keepdim=True) * cell + eps)
    else:
        g = S
    if meas is None:
        return g, None
    m = meas.double()
    if kind == 0:
        term = torch.special.xlogy(m, m) - m * torch.log(g + pad)
    elif kind == 1:
        term = (g - m).abs()
    else:
        term = (g - m) ** 2
    return g, term.sum(1) / div


@pytest.mark.parametrize("bins", [7, 256, 257, 7225])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("kind", ["kld", "mae", "mse"])
def test_norm_discrepancy_tail_vs_fp64(backend, kind, P, bins):
    k = ops.DISCREPANCY_KINDS[kind]
    gen = torch.Generator().manual_seed(bins + P)
    S = torch.rand(P, bins, generator=gen) * 50.0
    S[:, ::5] = 0.0
    meas = torch.rand(P, bins, generator=gen)
    meas[:, ::3] = 0.0                                                   # measured zeros: the xlogy branch
    if P > 1:
        S[1] = 0.0                                                       # all mass off the grid: norm = eps
    pad = 1e-12 if kind == "kld" else 0.0
    for normalize, pre_scale, cell in ((0, 1.0, 1.0), (1, 1.0 / 700.0, 0.37), (1, 1.0, 0.0123)):
        if kind == "mae" and not normalize:
            meas[:, 1::4] = S[:, 1::4]                                   # exact ties g == m: zero subgradient
        div = float(bins) if kind != "kld" else 2.0
        args = (bool(normalize), pre_scale, cell, 1e-10, k, pad, div)
        Sd = S.to(backend).clone().requires_grad_(True)
        ghat, D = ops.HistNormDiscFn.apply(Sd, meas.to(backend), *args)
        So = S.double().clone().requires_grad_(True)
        go, Do = _ref_tail(So, meas, normalize, pre_scale, cell, 1e-10, k, pad, div)
        torch.testing.assert_close(ghat.detach().cpu().double(), go.detach(), rtol=2e-5, atol=1e-6 * float(go.abs().max()))
        torch.testing.assert_close(D.detach().cpu().double(), Do.detach(), rtol=2e-4, atol=1e-7 * max(1.0, float(Do.abs().max())))
        wD, wg = torch.randn(P, generator=gen), torch.randn(P, bins, generator=gen)
        for use_D, use_g in ((True, False), (False, True), (True, True)):
            Sd.grad = None
            So.grad = None
            ghat, D = ops.HistNormDiscFn.apply(Sd, meas.to(backend), *args)
            lo = 0.0
            lk = 0.0
            if use_D:
                lk = lk + (D * wD.to(backend)).sum()
                lo = lo + (Do * wD.double()).sum()
            if use_g:
                lk = lk + (ghat * wg.to(backend)).sum()
                lo = lo + (go * wg.double()).sum()
            lk.backward()
            lo.backward(retain_graph=True)
            for p in range(P):                   # per row: an all-zero row's gradient is ~1/eps larger than the others
                ref = So.grad[p]
                torch.testing.assert_close(Sd.grad[p].cpu().double(), ref, rtol=1e-3,
                                           atol=2e-5 * float(ref.abs().max()) + 1e-30)


@pytest.mark.parametrize("name", ["kl_divergence", "mean_absolute_error", "mean_square_error"])
def test_losses_on_a_2d_prediction(backend, name):
    """mf.loss on a [Bx, By] prediction: batchmean (kl) divides by pred.shape[0], mae / mse by the element count."""
    gen = torch.Generator().manual_seed(6)
    pred = torch.rand(24, 17, generator=gen) + 0.01
    targ = torch.rand(24, 17, generator=gen)
    targ[::4, ::3] = 0.0
    pd = pred.to(backend).clone().requires_grad_(True)
    out = getattr(mf.loss, name)(pd, targ.to(backend))
    out.backward()
    po = pred.double().clone().requires_grad_(True)
    ref = getattr(om, name)(po, targ.double())
    ref.backward()
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach(), rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(pd.grad.cpu().double(), po.grad, rtol=1e-5, atol=1e-8 * float(po.grad.abs().max()))


# ================================================================================================ G. fused MAE / MSE
@pytest.mark.parametrize("disc", ["mean_absolute_error", "mean_square_error"])
@pytest.mark.parametrize("ndim", [1, 2])
def test_fused_loss_mae_mse_vs_oracle(backend, disc, ndim):
    if ndim == 1:
        e = torch.linspace(-3.5, 3.5, 65)
        dm = mf.diagnostics.Histogram1D(edges=e, bandwidth=0.5, axis=1).to(backend)
        do = om.Histogram1D(edges=e.double(), bandwidth=0.5, axis=1)
    else:
        ex, ey = torch.linspace(-3.5, 3.5, 41), torch.linspace(-3.0, 3.0, 25)
        dm = mf.diagnostics.Histogram2D(axis=(0, 2), edges=(ex, ey)).to(backend)
        do = om.Histogram2D(axis=(0, 2), edges=(ex.double(), ey.double()))
    _loss_vs_oracle(backend, dm, do, getattr(mf.loss, disc), getattr(om, disc), seed=ndim)


# ================================================================================================ H. entropy and helpers
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6, 7, 8])
def test_entropy_sums_vs_fp64(backend, n, d):
    _entropy_case(backend, n, d)


def _entropy_case(dev, n, d):
    gen = torch.Generator().manual_seed(n * 10 + d)
    x = torch.randn(n, d, generator=gen)
    lp = torch.randn(n, generator=gen) - 2.0
    xd = x.to(dev).clone().requires_grad_(True)
    ld = lp.to(dev).clone().requires_grad_(True)
    out = ops.EntropySumsFn.apply(xd, ld)
    want = torch.stack([lp.double().sum(), (x.double() ** 2).sum()])
    torch.testing.assert_close(out.detach().cpu().double(), want, rtol=1e-6, atol=1e-6)
    w = torch.tensor([0.7, -1.3])
    (out * w.to(dev)).sum().backward()
    torch.testing.assert_close(xd.grad.cpu().double(), 2.0 * w[1].double() * x.double(), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(ld.grad.cpu().double(), torch.full((n,), 0.7, dtype=torch.float64), rtol=0, atol=1e-7)


def _scale_rows_case(dev, n, d):
    gen = torch.Generator().manual_seed(n + d)
    x = torch.randn(n, d, generator=gen)
    g0 = torch.randn(n, d, generator=gen)
    xd, coef = x.to(dev), torch.tensor([0.37]).to(dev)     # bound: a temporary freed before the launch is reused
    for acc in (0, 1):
        gx = g0.to(dev).clone()
        call("mf_scale_rows", ptr(xd), n, d, ptr(coef), 2.0, ptr(gx), acc, stream_ptr(gx))
        want = 0.74 * x.double() + (g0.double() if acc else 0.0)
        torch.testing.assert_close(gx.cpu().double(), want, rtol=1e-6, atol=1e-7)


def _gather_case(dev, n):
    gen = torch.Generator().manual_seed(n)
    src = torch.randn(1000, generator=gen)
    idx = torch.randint(-3, 1000, (n,), generator=gen, dtype=torch.int32)
    dst0 = torch.randn(n, generator=gen)
    srcd, idxd = src.to(dev), idx.to(dev)
    for acc in (0, 1):
        dst = dst0.to(dev).clone()
        call("mf_gather_f32", ptr(srcd), ptr(idxd), ptr(dst), n, acc, stream_ptr(dst))
        want = torch.where(idx >= 0, src[idx.clamp(min=0).long()], torch.zeros(()))
        if acc:
            want = want + dst0
        assert torch.equal(dst.cpu(), want)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_scale_rows_and_gather(backend, n):
    for d in range(1, 9):
        _scale_rows_case(backend, n, d)
    _gather_case(backend, n)


# ================================================================================================ GPU-only sizes
@pytest.fixture
def hip():
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    _lib.use_library(_lib.DEFAULT_PATH)
    return torch.device("cuda", 0)


GPU_1D = [
    (70001, 6, 101, 85, 0.5, "fwd1024/Pg51x2(last50)/w1024/sh4-bwd256/ch4-fact"),
    (300000, 6, 101, 85, 0.3, "fwd1024/Pg51x2(last50)/w1024/sh6-bwd512/ch2-rt3"),
    (2097152, 6, 101, 85, 0.5, "fwd1024/Pg51x2(last50)/w4096/sh8-bwd512/ch1-fact"),
    (2097152, 4, 25, 64, 0.6, "fwd1024/Pg25x1/w2048/sh8-bwd512/ch1-rt5"),
    (300000, 1, 1, 64, 0.12, "fwd1024/Pg1x1/w1024/sh6-bwd512/ch1-rt1"),
    (70001, 8, 3, 85, 0.45, "fwd1024/Pg3x1/w1024/sh4-bwd256/ch2-fact"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,P,B,bw,path", _params_1d(GPU_1D))
def test_gpu_kde1d_vs_fp64(hip, n, d, P, B, bw, path):
    _run_1d(hip, n, d, P, B, bw, path, seed=n + d)


GPU_2D = [
    (70001, 6, 3, 85, 85, 0.5, 0.5, "fwd1024/Pg1x3/w1024/sh4-bwd256/npt1/Pg1-fact"),
    (300000, 6, 3, 85, 85, 0.5, 0.3, "fwd1024/Pg1x3/w1024/sh6-bwd512/npt1/Pg2-rt4x3"),
    (600000, 5, 2, 40, 24, 0.5, 0.3, "fwd1024/Pg2x1/w1024/sh7-bwd1024/npt1/Pg2-rt4x3"),
    (1048576, 6, 4, 40, 24, 0.5, 0.5, "fwd1024/Pg4x1/w1024/sh7-bwd1024/npt2/Pg4-fact"),
    (2097152, 6, 3, 85, 85, 0.5, 0.5, "fwd1024/Pg1x3/w6144/sh8-bwd1024/npt4/Pg3-fact"),
    (2097152, 4, 4, 31, 45, 0.45, 0.6, "fwd1024/Pg4x1/w2048/sh8-bwd1024/npt4/Pg4-rt4x5"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,P,Bx,By,bwx,bwy,path", _params_2d(GPU_2D))
def test_gpu_kde2d_vs_fp64(hip, n, d, P, Bx, By, bwx, bwy, path):
    _run_2d(hip, n, d, P, Bx, By, bwx, bwy, path, seed=n + d)


GPU_FIXED_POINT = [(70001, "w1024-sh4"), (2097152, "w2048-sh8"), (16777216, "w8192-sh11")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,path", [pytest.param(n, p, id=f"n{n}-{p}") for n, p in GPU_FIXED_POINT])
def test_gpu_fixed_point_centre_bin_exact(hip, n, path):
    plan = _fixed_point_plan(n)
    assert f"w{plan['per_wg']}-sh{plan['shift']}" == path
    _centre_case_1d(hip, n)
    _centre_case_2d(hip, n)
    _far_tail_case(hip, n, seed=n)


_PATH_1D = re.compile(r"fwd(?P<fwd>\d+)/Pg(?P<Pg>\d+)x(?P<G>\d+)(\(last(?P<last>\d+)\))?/w(?P<w>\d+)/sh(?P<sh>\d+)"
                      r"-bwd(?P<bwd>\d+)/ch(?P<ch>\d+)-(?P<win>fact|rt)\d*")
_PATH_2D = re.compile(r"fwd(?P<fwd>\d+)/Pg(?P<Pg>\d+)x(?P<G>\d+)/w(?P<w>\d+)/sh(?P<sh>\d+)"
                      r"-bwd(?P<bwd>\d+)/npt(?P<npt>\d+)/Pg(?P<bPg>\d+)-(?P<win>fact|rt)[\dx]*")


def test_case_lists_cover_the_launch_paths():
    """What the literals of the case lists cover, emulated and gpu-marked; no kernel runs here.  With the per-case equality of
    _run_1d / _run_2d (literal == the library's plan) a removed case or a moved threshold fails instead of passing quietly."""
    def fields(cases, pattern):
        return [{k: v if k == "win" or v is None else int(v) for k, v in pattern.fullmatch(c[-1]).groupdict().items()}
                for c in cases]

    e1, e2, g1, g2 = fields(CASES_1D, _PATH_1D), fields(CASES_2D, _PATH_2D), fields(GPU_1D, _PATH_1D), fields(GPU_2D, _PATH_2D)
    # the emulated lists
    assert {f["fwd"] for f in e1} == {256, 1024}
    assert {f["bwd"] for f in e1} == {256, 512}
    assert {f["ch"] for f in e1} == {1, 2, 4, 8}
    assert {"fwd": 256, "Pg": 4, "G": 2, "last": 1} in [{k: f[k] for k in ("fwd", "Pg", "G", "last")} for f in e1]     # small branch
    assert {"fwd": 1024, "Pg": 51, "G": 2, "last": 50} in [{k: f[k] for k in ("fwd", "Pg", "G", "last")} for f in e1]  # large branch
    assert {(f["bwd"], f["npt"]) for f in e2} == {(256, 1), (512, 1)}
    for e in (e1, e2):
        assert {f["sh"] for f in e} == {0, 4, 6}                                       # shift 0 and > 0
        assert {f["win"] for f in e} == {"fact", "rt"}                                 # both windows, forward and backward
        assert all(f["w"] == f["fwd"] for f in e)                                      # one particle per forward thread
    assert {p for _, p in FIXED_POINT} == {"sh0", "sh1"}
    # the gpu-marked lists, in addition
    assert {(f["bwd"], f["npt"]) for f in g2} >= {(1024, 1), (1024, 2), (1024, 4)}
    assert {f["w"] for f in g1 + g2 if f["w"] > f["fwd"]} == {2048, 4096, 6144}        # particles per workgroup above the block
    assert {p for _, p in GPU_FIXED_POINT} >= {"w8192-sh11"}


@pytest.mark.gpu
def test_gpu_entropy_and_helpers_past_the_grid_cap(hip):
    """Past the grid caps the kernels' stride loops wrap: entropy 4 workgroups per CU (256 CUs) x 1024 particles, scale_rows
    4096 x 1024 elements, gather 2048 x 256."""
    _entropy_case(hip, 256 * 4 * 1024 + 3, 6)
    _entropy_case(hip, 256 * 4 * 1024 + 3, 1)
    _scale_rows_case(hip, 4096 * 1024 // 6 + 5, 6)
    _scale_rows_case(hip, 4096 * 1024 + 5, 1)
    _gather_case(hip, 2048 * 256 + 7)
