"""The weighted projection kernels (mentflow_amd/csrc/wproj.hip) through their C ABI, against the fp64 dense evaluation of
tests/_wproj_fp64.py, on the emulator here and on the MI355X with -m gpu.

Gates (those tests/test_kde_launch_paths.py holds the unweighted kernels to): S / W at rtol 2e-5 + atol 1e-6 with W the sum of
the valid weights; gx and gw at rtol 1e-3 + atol 2e-5 max|g| + 1e-6.

Shapes, the smallest that reach every path: n in {1, 255, 257, 8 193} (8 193 crosses one workgroup's 8 192 particles and the
first non-zero shift), d in {1, 2, 6, 8}, P in {1, 3, 101} (101 needs several projection groups), 1-D bins {16, 64, 85}, 2-D
17 x 13 with radii (5, 3) and 85 x 85 with radii (4, 4) at P = 2, bandwidth 0.5 (factorised window) and 0.6 (run-time radius),
weights exp(2 randn), the same with 10 % zeros, and a set with one negative, one NaN and one +inf.  A NaN row and an inf row
ride along where n >= 255.

Exact properties (no tolerance): weights 1 reproduce the unweighted kernels bit for bit (S, gx, and the hard-binned sums as the
integer counts); weights 0.25 give exactly a quarter; permuting rows with their weights leaves S bitwise unchanged for
n <= 8 192 and two runs agree bitwise for any n; replacing every invalid weight by 0 changes no bit of S and gx; all weights
invalid give S == 0; gw is 0 exactly at the negative, NaN and inf rows; accumulate adds."""
import pytest
import torch

from _wproj_fp64 import ref_whist1d, ref_whist2d, ref_wkde1d, ref_wkde2d, valid64
from mentflow_amd import ops
from mentflow_amd._lib import call, ptr, stream_ptr

RTOL_S, ATOL_S = 2e-5, 1e-6


def assert_hist(S, So, W):
    torch.testing.assert_close(S.detach().double().cpu() / W, So.detach().cpu() / W, rtol=RTOL_S, atol=ATOL_S)


def assert_grad(g, go):
    go = go.detach().cpu()
    torch.testing.assert_close(g.detach().double().cpu(), go, rtol=1e-3, atol=2e-5 * float(go.abs().max()) + 1e-6)


def _grid(B, lo=-4.0, hi=4.0):
    e = torch.linspace(lo, hi, B + 1)
    return e, 0.5 * (e[1:] + e[:-1]), float(e[1] - e[0])


def _dirs(P, d, gen):
    V = torch.randn(P, d, generator=gen)
    return V / V.norm(dim=1, keepdim=True)


def _weights(n, kind, gen):
    w = torch.exp(2.0 * torch.randn(n, generator=gen))
    if kind == "zeros":
        w[torch.rand(n, generator=gen) < 0.1] = 0.0
        if n > 1:
            w[0] = 0.0                                          # at least one
    if kind == "bad":
        w[n // 5], w[n // 3], w[n // 2] = -1.5, float("nan"), float("inf")
        w[n - 1] = 0.0
    return w


def _rows(n, d, gen):
    x = 1.3 * torch.randn(n, d, generator=gen)
    if n >= 255:
        x[7, d - 1] = float("nan")
        x[11, 0] = float("inf")
    return x


def wkde1d_bwd(x, w, V, c, sigma, R, gS, gx, gw, accumulate):
    call("mf_proj_wkde1d_bwd", ptr(x), ptr(w), x.shape[0], x.shape[1], ptr(V), V.shape[0], ptr(c), c.numel(), float(sigma), int(R),
         ptr(gS.contiguous()), ptr(gx), ptr(gw), int(accumulate), stream_ptr(x))
    return gx, gw


def wkde2d_bwd(x, w, V0, V1, cx, cy, sx, sy, rx, ry, gS, gx, gw, accumulate):
    call("mf_proj_wkde2d_bwd", ptr(x), ptr(w), x.shape[0], x.shape[1], ptr(V0), ptr(V1), V0.shape[0], ptr(cx), cx.numel(),
         float(sx), int(rx), ptr(cy), cy.numel(), float(sy), int(ry), ptr(gS.contiguous()), ptr(gx), ptr(gw), int(accumulate),
         stream_ptr(x))
    return gx, gw


def kde1d_bwd(x, V, c, sigma, R, gS):
    gx = torch.empty_like(x)
    call("mf_proj_kde1d_bwd", ptr(x), x.shape[0], x.shape[1], ptr(V), V.shape[0], ptr(c), c.numel(), float(sigma), int(R),
         ptr(gS.contiguous()), ptr(gx), 0, stream_ptr(x))
    return gx


def kde2d_bwd(x, V0, V1, cx, cy, sx, sy, rx, ry, gS):
    gx = torch.empty_like(x)
    call("mf_proj_kde2d_bwd", ptr(x), x.shape[0], x.shape[1], ptr(V0), ptr(V1), V0.shape[0], ptr(cx), cx.numel(),
         float(sx), int(rx), ptr(cy), cy.numel(), float(sy), int(ry), ptr(gS.contiguous()), ptr(gx), 0, stream_ptr(x))
    return gx


def _check_gw(gw, gwo, w):
    """fp64 value where the weight is valid or zero, exactly 0 at a negative, NaN or infinite one"""
    grows = (torch.isfinite(w) & (w >= 0)).cpu()
    assert bool((gw.cpu()[~grows] == 0).all())
    assert_grad(gw.cpu() * grows, gwo.cpu() * grows)


# ------------------------------------------------------------------------------------------------ against fp64
CASES_1D = [  # n, d, P, B, bandwidth (bins), weights
    (1, 1, 1, 16, 0.5, "rand"),
    (255, 2, 3, 64, 0.5, "zeros"),
    (257, 6, 101, 85, 0.6, "rand"),
    (257, 8, 1, 85, 0.5, "bad"),
    (8193, 8, 3, 64, 0.5, "bad"),
    (8193, 6, 101, 16, 0.6, "zeros"),
    (8193, 1, 3, 85, 0.5, "rand"),
]


@pytest.mark.parametrize("n,d,P,B,bw,kind", CASES_1D, ids=lambda v: str(v))
def test_wkde1d_against_fp64(backend, n, d, P, B, bw, kind):
    gen = torch.Generator().manual_seed(n + 7 * d + P)
    x, w, V = _rows(n, d, gen), _weights(n, kind, gen), _dirs(P, d, gen)
    _, c, delta = _grid(B)
    sigma, R = bw * delta, ops.kde_radius(bw)
    gS = torch.randn(P, B, generator=gen)
    So, gxo, gwo = ref_wkde1d(x, w, V, c, sigma, gS)
    xd, wd, Vd, cd = (t.to(backend) for t in (x, w, V, c))
    S = ops.ProjWKde1dFn.apply(xd, wd, Vd, cd, sigma, R)
    assert_hist(S, So, float(valid64(w).sum()))
    gx, gw = wkde1d_bwd(xd, wd, Vd, cd, sigma, R, gS.to(backend), torch.empty_like(xd), torch.empty_like(wd), 0)
    assert_grad(gx, gxo)
    _check_gw(gw, gwo, w)
    assert bool((gx.cpu()[~(torch.isfinite(w) & (w > 0))] == 0).all()), "an invalid or zero weight has gx = 0"


CASES_2D = [  # n, d, P, Bx, By, bandwidths (bins): 0.6 -> radius 5, 0.38 -> radius 3, 0.5 -> radius 4 (factorised)
    (1, 2, 1, 17, 13, 0.6, 0.38, "rand"),
    (255, 6, 3, 17, 13, 0.6, 0.38, "zeros"),
    (257, 2, 101, 17, 13, 0.6, 0.38, "bad"),
    (257, 8, 2, 85, 85, 0.5, 0.5, "bad"),
    (8193, 6, 2, 85, 85, 0.5, 0.5, "zeros"),
    (8193, 1, 3, 17, 13, 0.6, 0.38, "rand"),
]


@pytest.mark.parametrize("n,d,P,Bx,By,bwx,bwy,kind", CASES_2D, ids=lambda v: str(v))
def test_wkde2d_against_fp64(backend, n, d, P, Bx, By, bwx, bwy, kind):
    gen = torch.Generator().manual_seed(n + 7 * d + P + Bx)
    x, w = _rows(n, d, gen), _weights(n, kind, gen)
    V0, V1 = _dirs(P, d, gen), _dirs(P, d, gen)
    (_, cx, dx), (_, cy, dy) = _grid(Bx), _grid(By, -3.0, 3.5)
    sx, sy, rx, ry = bwx * dx, bwy * dy, ops.kde_radius(bwx), ops.kde_radius(bwy)
    assert (rx, ry) in ((5, 3), (4, 4))
    gS = torch.randn(P, Bx, By, generator=gen)
    So, gxo, gwo = ref_wkde2d(x, w, V0, V1, cx, cy, sx, sy, gS)
    xd, wd, V0d, V1d, cxd, cyd = (t.to(backend) for t in (x, w, V0, V1, cx, cy))
    S = ops.ProjWKde2dFn.apply(xd, wd, V0d, V1d, cxd, cyd, sx, sy, rx, ry)
    assert_hist(S, So, float(valid64(w).sum()))
    gx, gw = wkde2d_bwd(xd, wd, V0d, V1d, cxd, cyd, sx, sy, rx, ry, gS.to(backend), torch.empty_like(xd), torch.empty_like(wd), 0)
    assert_grad(gx, gxo)
    _check_gw(gw, gwo, w)


@pytest.mark.parametrize("n,d,P,kind", [(1, 1, 1, "rand"), (257, 6, 101, "bad"), (8193, 8, 3, "zeros")], ids=lambda v: str(v))
def test_whist_sums_against_fp64(backend, n, d, P, kind):
    gen = torch.Generator().manual_seed(3 * n + d)
    x, w = _rows(n, d, gen), _weights(n, kind, gen)
    V0, V1 = _dirs(P, d, gen), _dirs(P, d, gen)
    (e, _, _), (ey, _, _) = _grid(16), _grid(13, -3.0, 3.5)
    W = float(valid64(w).sum())
    xd, wd = x.to(backend), w.to(backend)
    assert_hist(ops.proj_whist_sums_1d(xd, wd, V0.to(backend), e.to(backend)), ref_whist1d(x, w, V0, e), W)
    assert_hist(ops.proj_whist_sums_2d(xd, wd, V0.to(backend), V1.to(backend), e.to(backend), ey.to(backend)),
                ref_whist2d(x, w, V0, V1, e, ey), W)


# ------------------------------------------------------------------------------------------------ exact properties
def _setup_1d(n, d, P, B, bw, backend, seed=5):
    gen = torch.Generator().manual_seed(seed)
    x, V = _rows(n, d, gen), _dirs(P, d, gen)
    _, c, delta = _grid(B)
    gS = torch.randn(P, B, generator=gen)
    return x.to(backend), V.to(backend), c.to(backend), bw * delta, ops.kde_radius(bw), gS.to(backend), gen


def _setup_2d(n, d, P, Bx, By, bwx, bwy, backend, seed=6):
    gen = torch.Generator().manual_seed(seed)
    x, V0, V1 = _rows(n, d, gen), _dirs(P, d, gen), _dirs(P, d, gen)
    (_, cx, dx), (_, cy, dy) = _grid(Bx), _grid(By, -3.0, 3.5)
    gS = torch.randn(P, Bx, By, generator=gen)
    args = (V0.to(backend), V1.to(backend), cx.to(backend), cy.to(backend), bwx * dx, bwy * dy, ops.kde_radius(bwx),
            ops.kde_radius(bwy))
    return x.to(backend), args, gS.to(backend), gen


@pytest.mark.parametrize("n,bw", [(257, 0.5), (8193, 0.5), (8193, 0.6)])
def test_unit_and_quarter_weights_1d(backend, n, bw):
    x, V, c, sigma, R, gS, _ = _setup_1d(n, 6, 3, 64, bw, backend)
    ones = torch.ones(n, device=backend)
    S0 = ops.ProjKde1dFn.apply(x, V, c, sigma, R)
    S1 = ops.ProjWKde1dFn.apply(x, ones, V, c, sigma, R)
    assert torch.equal(S1, S0), "weights 1: the unweighted sums bit for bit"
    gx, _ = wkde1d_bwd(x, ones, V, c, sigma, R, gS, torch.empty_like(x), torch.empty_like(ones), 0)
    assert torch.equal(gx, kde1d_bwd(x, V, c, sigma, R, gS)), "weights 1: the unweighted gx bit for bit"
    assert torch.equal(ops.ProjWKde1dFn.apply(x, 0.25 * ones, V, c, sigma, R), 0.25 * S0), "a power of two passes through w_max"


@pytest.mark.parametrize("n,Bx,By,bwx,bwy", [(257, 17, 13, 0.6, 0.38), (8193, 85, 85, 0.5, 0.5)])
def test_unit_and_quarter_weights_2d(backend, n, Bx, By, bwx, bwy):
    x, args, gS, _ = _setup_2d(n, 6, 2, Bx, By, bwx, bwy, backend)
    ones = torch.ones(n, device=backend)
    S0 = ops.ProjKde2dFn.apply(x, *args)
    assert torch.equal(ops.ProjWKde2dFn.apply(x, ones, *args), S0)
    gx, _ = wkde2d_bwd(x, ones, *args, gS, torch.empty_like(x), torch.empty_like(ones), 0)
    assert torch.equal(gx, kde2d_bwd(x, *args, gS))
    assert torch.equal(ops.ProjWKde2dFn.apply(x, 0.25 * ones, *args), 0.25 * S0)


@pytest.mark.parametrize("n", [257, 8193])
def test_unit_weights_give_the_counts(backend, n):
    gen = torch.Generator().manual_seed(9)
    x, V0, V1 = _rows(n, 6, gen).to(backend), _dirs(101, 6, gen).to(backend), _dirs(101, 6, gen).to(backend)
    (e, _, _), (ey, _, _) = _grid(16), _grid(13, -3.0, 3.5)
    e, ey, ones = e.to(backend), ey.to(backend), torch.ones(n, device=backend)
    s1, c1 = ops.proj_whist_sums_1d(x, ones, V0, e), ops.proj_hist_counts_1d(x, V0, e)
    assert torch.equal(s1.to(torch.int32), c1) and torch.equal(s1, c1.to(torch.float32))
    s2, c2 = ops.proj_whist_sums_2d(x, ones, V0, V1, e, ey), ops.proj_hist_counts_2d(x, V0, V1, e, ey)
    assert torch.equal(s2.to(torch.int32), c2) and torch.equal(s2, c2.to(torch.float32))
    assert int(c1.sum()) > 0 and int(c2.sum()) > 0


@pytest.mark.parametrize("n", [257, 8000, 8193])
def test_order_independence_and_reproducibility(backend, n):
    x, V, c, sigma, R, _, gen = _setup_1d(n, 6, 3, 64, 0.5, backend)
    w = _weights(n, "zeros", gen).to(backend)
    S = ops.ProjWKde1dFn.apply(x, w, V, c, sigma, R)
    assert torch.equal(ops.ProjWKde1dFn.apply(x, w, V, c, sigma, R), S), "two runs agree bitwise"
    x2, args, _, _ = _setup_2d(n, 6, 2, 17, 13, 0.6, 0.38, backend)
    S2 = ops.ProjWKde2dFn.apply(x2, w, *args)
    assert torch.equal(ops.ProjWKde2dFn.apply(x2, w, *args), S2)
    e = _grid(16)[0].to(backend)
    H = ops.proj_whist_sums_1d(x, w, V, e)
    assert torch.equal(ops.proj_whist_sums_1d(x, w, V, e), H)
    if n <= 8192:                                       # shift 0: every flush is exact, so the order of the rows is immaterial
        perm = torch.randperm(n, generator=gen).to(backend)
        assert torch.equal(ops.ProjWKde1dFn.apply(x[perm], w[perm], V, c, sigma, R), S)
        assert torch.equal(ops.ProjWKde2dFn.apply(x2[perm], w[perm], *args), S2)
        assert torch.equal(ops.proj_whist_sums_1d(x[perm], w[perm], V, e), H)


@pytest.mark.parametrize("n", [257, 8193])
def test_invalid_weights_count_as_zero(backend, n):
    x, V, c, sigma, R, gS, gen = _setup_1d(n, 6, 3, 64, 0.5, backend)
    w = _weights(n, "bad", gen)
    wz = torch.where(torch.isfinite(w) & (w > 0), w, torch.zeros_like(w))
    w, wz = w.to(backend), wz.to(backend)
    assert torch.equal(ops.ProjWKde1dFn.apply(x, w, V, c, sigma, R), ops.ProjWKde1dFn.apply(x, wz, V, c, sigma, R))
    gx, _ = wkde1d_bwd(x, w, V, c, sigma, R, gS, torch.empty_like(x), torch.empty_like(w), 0)
    gxz, _ = wkde1d_bwd(x, wz, V, c, sigma, R, gS, torch.empty_like(x), torch.empty_like(w), 0)
    assert torch.equal(gx, gxz)
    x2, args, gS2, _ = _setup_2d(n, 6, 2, 17, 13, 0.6, 0.38, backend)
    assert torch.equal(ops.ProjWKde2dFn.apply(x2, w, *args), ops.ProjWKde2dFn.apply(x2, wz, *args))
    gx, _ = wkde2d_bwd(x2, w, *args, gS2, torch.empty_like(x2), torch.empty_like(w), 0)
    gxz, _ = wkde2d_bwd(x2, wz, *args, gS2, torch.empty_like(x2), torch.empty_like(w), 0)
    assert torch.equal(gx, gxz)
    e = _grid(16)[0].to(backend)
    assert torch.equal(ops.proj_whist_sums_1d(x, w, V, e), ops.proj_whist_sums_1d(x, wz, V, e))
    # no valid weight at all: everything is exactly zero
    none = torch.tensor([0.0, -1.0, float("nan"), float("inf"), float("-inf")]).repeat(n // 5 + 1)[:n].to(backend)
    assert bool((ops.ProjWKde1dFn.apply(x, none, V, c, sigma, R) == 0).all())
    assert bool((ops.ProjWKde2dFn.apply(x2, none, *args) == 0).all())
    assert bool((ops.proj_whist_sums_1d(x, none, V, e) == 0).all())


def test_accumulate_adds_to_both_gradients(backend):
    n = 257
    x, V, c, sigma, R, gS, gen = _setup_1d(n, 6, 3, 64, 0.5, backend)
    w = _weights(n, "zeros", gen).to(backend)
    gx0, gw0 = wkde1d_bwd(x, w, V, c, sigma, R, gS, torch.empty_like(x), torch.empty_like(w), 0)
    bx, bw_ = torch.randn(n, 6, generator=gen).to(backend), torch.randn(n, generator=gen).to(backend)
    gx1, gw1 = wkde1d_bwd(x, w, V, c, sigma, R, gS, bx.clone(), bw_.clone(), 1)
    assert torch.equal(gx1, bx + gx0) and torch.equal(gw1, bw_ + gw0)
    # either output alone
    only_w = wkde1d_bwd(x, w, V, c, sigma, R, gS, None, torch.empty_like(w), 0)[1]
    only_x = wkde1d_bwd(x, w, V, c, sigma, R, gS, torch.empty_like(x), None, 0)[0]
    assert torch.equal(only_w, gw0) and torch.equal(only_x, gx0)
    x2, args, gS2, _ = _setup_2d(n, 6, 2, 17, 13, 0.6, 0.38, backend)
    gx0, gw0 = wkde2d_bwd(x2, w, *args, gS2, torch.empty_like(x2), torch.empty_like(w), 0)
    gx1, gw1 = wkde2d_bwd(x2, w, *args, gS2, bx.clone(), bw_.clone(), 1)
    assert torch.equal(gx1, bx + gx0) and torch.equal(gw1, bw_ + gw0)


def test_refusals(backend):
    x, V, c, sigma, R, gS, _ = _setup_1d(16, 6, 3, 64, 0.5, backend)
    w = torch.ones(16, device=backend)
    with pytest.raises(RuntimeError, match="sigma"):
        ops.ProjWKde1dFn.apply(x, w, V, c, 0.0, R)
    with pytest.raises(RuntimeError, match="at least one of gx and gw"):
        wkde1d_bwd(x, w, V, c, sigma, R, gS, None, None, 0)
    with pytest.raises(RuntimeError, match="d="):
        ops.ProjWKde1dFn.apply(torch.zeros(4, 9, device=backend), w[:4], torch.zeros(3, 9, device=backend), c, sigma, R)
    with pytest.raises(ValueError, match="weights"):
        ops.ProjWKde1dFn.apply(x, w[:5], V, c, sigma, R)
    x2, args, _, _ = _setup_2d(16, 6, 2, 17, 13, 0.6, 0.38, backend)
    with pytest.raises(RuntimeError, match="radius"):
        ops.ProjWKde2dFn.apply(x2, w, *args[:6], 6, 3)
