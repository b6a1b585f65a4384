"""fp64 NumPy gradient of the sliced Wasserstein distance of tests/_swd_fp64.py, written out term by term (test infrastructure).

For projections u[P, n], v[P, m] (any order within a row)

    dist = M^(1/p),   M = mean_s wpp[s],   wpp[s] = sum_pieces width |u_(i) - v_(j)|^p / (n m)

over the quantile pieces of tests/_swd_fp64.wasserstein_1d_pp (equal sizes: n pieces of width 1, divided by n).  A piece is
constant in the ranks (i, j) it pairs, so away from ties

    d dist / d u_(i) = coef * sum_{pieces with i} width phi'(u_(i) - v_(j)) / (n m),    d dist / d v_(j) = the same with a minus sign,
    coef = (1/p) M^(1/p - 1) / P,    phi'(t) = p |t|^(p-1) sign(t),  sign(0) = 0.

Ranks come from a stable argsort, which is also how torch.sort(stable=True) breaks ties.  M == 0 gives zero gradients: the
library's documented choice (include/mentflow_hip.h), where the composed formula has 0 * inf for p > 1.

Every function returns, next to each gradient entry, the sum of the absolute values of its terms (times |coef| / (n m)): the
scale against which a rounding error of that entry is measured.  tests/test_swd_grad_kernels.py pins this module to torch's
fp64 autograd through sort + gather and to central differences."""
import math

import numpy as np


def pieces(n: int, m: int):
    """(width, iu, iv, denom): the quantile pieces in units of 1 / denom and the ranks of u and v each one pairs."""
    if n == m:
        r = np.arange(n, dtype=np.int64)
        return np.ones(n, dtype=np.int64), r, r, float(n)
    bu = np.arange(1, n + 1, dtype=np.int64) * m
    bv = np.arange(1, m + 1, dtype=np.int64) * n
    b = np.union1d(bu, bv)
    width = np.diff(np.concatenate([np.zeros(1, dtype=np.int64), b]))
    return width, (b - 1) // m, (b - 1) // n, float(n) * float(m)


def dphi(t: np.ndarray, p: float) -> np.ndarray:
    if p == 1.0:
        return np.sign(t)
    with np.errstate(invalid="ignore"):
        return np.where(t == 0.0, 0.0, p * np.abs(t) ** (p - 1.0) * np.sign(t))


def dist_and_grad(u, v, p=2.0):
    """u[P, n], v[P, m] -> dist, gu[P, n], au[P, n], gv[P, m], av[P, m] (fp64; a* = sums of absolute terms), in input order."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    P, n = u.shape
    m = v.shape[1]
    width, iu, iv, denom = pieces(n, m)
    w = width.astype(np.float64)
    wpp = np.empty(P)
    gu, au, gv, av = np.zeros((P, n)), np.zeros((P, n)), np.zeros((P, m)), np.zeros((P, m))
    for s in range(P):
        ou, ov = np.argsort(u[s], kind="stable"), np.argsort(v[s], kind="stable")
        t = u[s][ou][iu] - v[s][ov][iv]
        wpp[s] = math.fsum(w * np.abs(t) ** p) / denom
        term = w * dphi(t, p) / denom
        gu[s, ou] = np.bincount(iu, weights=term, minlength=n)
        gv[s, ov] = -np.bincount(iv, weights=term, minlength=m)
        au[s, ou] = np.bincount(iu, weights=np.abs(term), minlength=n)
        av[s, ov] = np.bincount(iv, weights=np.abs(term), minlength=m)
    M = math.fsum(wpp) / P
    if M == 0.0:
        coef = 0.0
    else:
        coef = (1.0 / p) * M ** (1.0 / p - 1.0) / P
    dist = M ** (1.0 / p)
    return dist, coef * gu, abs(coef) * au, coef * gv, abs(coef) * av


def back_project(g, directions):
    """gx[N, d] = g[P, N].T @ directions[d, P].T in fp64."""
    return np.asarray(g, dtype=np.float64).T @ np.asarray(directions, dtype=np.float64).T
