"""fp64 restatement of classical MENT's log-density and of its gradient, in torch: the yardstick of tests/test_ment_logp_*.py.

    logp(x) = sum_s log clamp(h_s(u_s(x)), 0, 1e10) + log prior(x)

on tests/_ment_fp64.interp64, the gradient by fp64 autograd.  interp64 takes the cell searchsorted(right=True) - 1 clamped to
B - 2, so the derivative is the right one at an interior centre and the left one at the last centre, as in the kernel.  The
conventions of include/mentflow_hip.h are restated too: the first zero factor makes the row -inf (gradient 0), the first NaN
factor makes it NaN (gradient NaN), a factor on the upper clamp is a constant.

A point is AMBIGUOUS when some slot's fp64 grid position s = (u - c_0) / delta lies within BAND = 1e-4 of an integer in
[0, B - 1] (both hull ends included): there fp32 and fp64 may pick different cells, so values (at the hull) and one-sided
derivatives (at every centre) may legitimately differ.  u carries ~d ulp of fp32 rounding and s = (u - c_0) / delta, at most 64,
an error of ~1e-5; the band is 10 times that."""
import math

import torch

from _ment_fp64 import interp64

BAND = 1.0e-4


def ambiguous(coords, u):
    amb = torch.zeros(u.shape[0], dtype=torch.bool)
    for k, c in enumerate(coords):
        c = c.double().cpu()
        B = c.numel()
        s = (u[:, k].detach().double().cpu() - c[0]) / ((c[-1] - c[0]) / (B - 1))
        r = torch.round(s)
        amb |= ((s - r).abs() < BAND) & (r >= 0) & (r <= B - 1)
    return amb


def logp64(x, slots, prior=None, extra=None):
    """slots: [(rows [k][d], coords [k], values)]; prior: None, ("gaussian", scale) or ("uniform", half_width);
    extra(x) -> [(coords, values, u)]: further factors at coordinates that are a differentiable function of x (pre-transforms).
    Returns (logp [n], grad [n, d], ambiguous [n]) in fp64 on the CPU."""
    x = x.detach().double().cpu().requires_grad_(True)
    n, d = x.shape
    total = torch.zeros(n, dtype=torch.float64)
    dead = torch.zeros(n, dtype=torch.bool)
    nan = torch.zeros(n, dtype=torch.bool)
    amb = torch.zeros(n, dtype=torch.bool)
    factors = [(coords, values, torch.stack([x @ r.double().cpu() for r in rows], dim=1)) for rows, coords, values in slots]
    if extra is not None:
        factors += extra(x)
    for coords, values, u in factors:
        h = interp64(coords, values, u)
        amb |= ambiguous(coords, u)
        zero, top = h <= 0.0, h >= 1.0e10
        nan |= torch.isnan(h) & ~dead                    # whichever comes first decides the row
        dead |= zero & ~nan
        t = torch.log(torch.where(zero | top, torch.ones_like(h), h))
        total = total + torch.where(top, torch.full_like(t, math.log(1.0e10)), t)
    if prior is not None and prior[0] == "gaussian":
        s = prior[1]
        total = total - d * (math.log(s) + 0.5 * math.log(2 * math.pi)) - 0.5 * (x * x).sum(1) / s ** 2
    elif prior is not None and prior[0] == "uniform":
        a = prior[1]
        total = total - d * math.log(2 * a)
        dead |= ~(x.detach().abs() <= a).all(1) & ~nan
    nan |= torch.isnan(total.detach()) & ~dead
    dead |= torch.isneginf(total.detach()) & ~nan            # a Gaussian prior at an infinite coordinate
    (grad,) = torch.autograd.grad(total.sum(), x)
    value = total.detach().clone()
    value[dead] = float("-inf")
    value[nan] = float("nan")
    grad[dead] = 0.0
    grad[nan] = float("nan")
    return value, grad, amb


def check_gates(lp, g, ref, gref, amb, cap, tol=3.0e-4):
    """The gates of the log-density tests.  Non-ambiguous points: -inf and NaN rows where the reference has them (gradient rows 0
    and NaN), elsewhere |l - l64| <= tol (1 + |l64|) and max_j |g - g64| <= tol (1 + |g64|_inf) per point.  Ambiguous points:
    no NaN (unless the reference row is NaN), at most `cap` of all points.  Returns the measured figures."""
    lp, ref = lp.detach().cpu().double(), ref.cpu().double()
    clear = ~amb
    nan, dead = torch.isnan(ref), torch.isneginf(ref)
    fin = clear & ~nan & ~dead
    stats = {"ambiguous": float(amb.double().mean()), "finite": int(fin.sum()), "dead": int((dead & clear).sum())}
    assert stats["ambiguous"] <= cap, stats
    assert torch.equal(torch.isnan(lp)[clear], nan[clear]) and not torch.isnan(lp[amb & ~nan]).any()
    assert torch.equal(torch.isneginf(lp)[clear], dead[clear])
    assert stats["finite"] > 0
    stats["value"] = float(((lp[fin] - ref[fin]).abs() / (1 + ref[fin].abs())).max())
    if g is not None:
        g, gref = g.detach().cpu().double(), gref.cpu().double()
        assert torch.isnan(g[clear & nan]).all() and not torch.isnan(g[~nan]).any()
        assert (g[clear & dead] == 0).all()
        stats["grad"] = float(((g[fin] - gref[fin]).abs().amax(1) / (1 + gref[fin].abs().amax(1))).max())
    print(stats)
    assert stats["value"] <= tol, stats
    assert g is None or stats["grad"] <= tol, stats
    return stats
