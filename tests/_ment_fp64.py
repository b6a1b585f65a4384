"""fp64 restatement of classical MENT's density, in torch (the yardstick of tests/test_ment_*.py; no scipy needed).

h is scipy.interpolate.RegularGridInterpolator(method="linear", bounds_error=False, fill_value=0) as mentflow/ment.py uses it:
linear / bilinear between the stored centres, 0 outside [c_0, c_{B-1}] on any axis, NaN for a NaN coordinate."""
import math

import torch


def interp64(coords, values, u):
    """coords: list of 1 or 2 centre vectors; values [B] or [Bx, By]; u [n, len(coords)] -> [n] fp64."""
    u = u.double()
    v = values.double().cpu()
    idx, w, inside, nan = [], [], torch.ones(u.shape[0], dtype=torch.bool), torch.zeros(u.shape[0], dtype=torch.bool)
    for k, c in enumerate(coords):
        c = c.double().cpu()
        uk = u[:, k].cpu()
        i = (torch.searchsorted(c, uk.contiguous(), right=True) - 1).clamp(0, c.numel() - 2)
        idx.append(i)
        w.append((uk - c[i]) / (c[i + 1] - c[i]))
        inside &= (uk >= c[0]) & (uk <= c[-1])
        nan |= torch.isnan(uk)
    if len(coords) == 1:
        h = v[idx[0]] * (1 - w[0]) + v[idx[0] + 1] * w[0]
    else:
        i, k, a, b = idx[0], idx[1], w[0], w[1]
        h = v[i, k] * (1 - a) * (1 - b) + v[i, k + 1] * (1 - a) * b + v[i + 1, k] * a * (1 - b) + v[i + 1, k + 1] * a * b
    h = torch.where(inside, h, torch.zeros_like(h))
    return torch.where(nan, torch.full_like(h, float("nan")), h)


def prob64(x, slots, prior=None):
    """slots: [(rows [k][d], coords [k], values)]; prior: None, ("gaussian", scale) or ("uniform", half_width)."""
    x = x.double().cpu()
    p = torch.ones(x.shape[0], dtype=torch.float64)
    for rows, coords, values in slots:
        u = torch.stack([x @ r.double().cpu() for r in rows], dim=1)
        p = p * interp64(coords, values, u).clamp(0.0, 1e10)
    d = x.shape[1]
    if prior is not None and prior[0] == "gaussian":
        s = prior[1]
        p = p * torch.exp(-d * (math.log(s) + 0.5 * math.log(2 * math.pi)) - 0.5 * (x * x).sum(1) / s ** 2)
    elif prior is not None and prior[0] == "uniform":
        a = prior[1]
        p = p * torch.where((x.abs() <= a).all(1), torch.full_like(p, (2 * a) ** -d), torch.zeros_like(p))
    return p
