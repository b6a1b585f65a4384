"""fp64 NumPy restatement of the sliced Wasserstein distance, written from its definition (test infrastructure).

The reference computes the per-projection cost with POT's ``ot.lp.wasserstein_1d`` (mentflow/loss.py:40).  POT is not
available where this suite runs, so no golden file can be produced from the reference; this module restates the definition
instead and tests/test_swd_kernels.py pins it to ``scipy.stats.wasserstein_distance`` for p = 1:

    W_p^p(u, v) = int_0^1 |F_u^-1(q) - F_v^-1(q)|^p dq      for the uniform-weight empirical measures of u[n] and v[m].

Equal sizes: mean_i |u_(i) - v_(i)|^p.  Unequal sizes: in units of 1 / (n m) the quantile function of u steps at the integers
m, 2m, ..., nm and that of v at n, 2n, ..., nm; the union of both (exact int64) cuts (0, nm] into intervals on which both
quantile functions are constant.  Inputs are the fp32 arrays the kernels see, promoted exactly to fp64.
"""
import math

import numpy as np


def wasserstein_1d_pp(u, v, p=2.0) -> float:
    """W_p^p of two 1-D samples (any order)."""
    u = np.sort(np.asarray(u, dtype=np.float64))
    v = np.sort(np.asarray(v, dtype=np.float64))
    n, m = int(u.size), int(v.size)
    if n == m:
        return math.fsum(np.abs(u - v) ** p) / n
    bu = np.arange(1, n + 1, dtype=np.int64) * m
    bv = np.arange(1, m + 1, dtype=np.int64) * n
    b = np.union1d(bu, bv)                                    # sorted, unique; the last one is n * m
    width = np.diff(np.concatenate([np.zeros(1, dtype=np.int64), b]))
    iu = (b - 1) // m                                         # the interval (b[k-1], b[k]] lies in (iu m, (iu + 1) m]
    iv = (b - 1) // n
    return math.fsum(width.astype(np.float64) * np.abs(u[iu] - v[iv]) ** p) / (float(n) * float(m))


def project(x, directions) -> np.ndarray:
    """[P, N] fp64 projections of the fp32 inputs."""
    return (np.asarray(x, dtype=np.float64) @ np.asarray(directions, dtype=np.float64)).T


def swd_wpp(x1, x2, directions, p=2.0) -> np.ndarray:
    """wpp[P]: the per-projection costs."""
    u1, u2 = project(x1, directions), project(x2, directions)
    return np.array([wasserstein_1d_pp(a, b, p) for a, b in zip(u1, u2)])


def swd(x1, x2, directions, p=2.0) -> float:
    return float(np.mean(swd_wpp(x1, x2, directions, p)) ** (1.0 / p))


def delta(x1, x2) -> float:
    """Rounding bound of one fp32 projection onto a unit direction: (d + 2) 2^-24 max_n |x_n|_2 over both clouds."""
    d = np.asarray(x1).shape[1]
    r = max(float(np.linalg.norm(np.asarray(x, dtype=np.float64), axis=1).max()) for x in (x1, x2))
    return (d + 2) * 2.0 ** -24 * r


def wpp_bound_p2(x1, x2, directions) -> np.ndarray:
    """Per projection, the most the p = 2 cost computed from fp32 projections may differ from the exact one.  Sorting is
    1-Lipschitz in the sup norm, so every sorted fp32 projection is within delta of its exact value, each difference
    u_(i) - v_(j) within 2 delta, each square within 4 delta |u_(i) - v_(j)| + 4 delta^2; averaged: 4 delta W_1 + 4 delta^2."""
    dl = delta(x1, x2)
    return 4.0 * dl * swd_wpp(x1, x2, directions, 1.0) + 4.0 * dl * dl
