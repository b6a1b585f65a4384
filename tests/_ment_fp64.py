"""fp64 restatement of classical MENT's density and of its inverse-CDF grid sampler, in torch (the yardstick of
tests/test_ment_*.py; no scipy needed).

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


def place64(cell, shape, edges, rnd, noise):
    """The point of each draw in the given flat cell (row-major, last axis fastest): the sampler's own fp32 arithmetic,
    lb + (ub - lb) * rnd[:, 1 + j], with noise + 0.5 * (-delta + 2 delta * rnd[:, 1 + d + j])."""
    d = len(shape)
    rnd = rnd.float().cpu()
    q = cell.clone()
    x = torch.empty(cell.numel(), d, dtype=torch.float32)
    for j in range(d - 1, -1, -1):
        k = q % shape[j]
        q = q // shape[j]
        e = edges[j].float().cpu()
        lb, ub = e[k], e[k + 1]
        v = lb + (ub - lb) * rnd[:, 1 + j]
        if noise:
            delta = ub - lb
            v = v + 0.5 * (-delta + (delta + delta) * rnd[:, 1 + d + j])
        x[:, j] = v
    return x


def cdf64(p):
    """fp64 cumulative sum of the sampling weights: p + 1e-15 added in fp32, as the kernel's cell_weight and the reference's
    hist + 1e-15 on an fp32 histogram."""
    return torch.cumsum((p.float().cpu().reshape(-1) + 1e-15).double(), 0)


def sample64(p, shape, edges, rnd, noise):
    """Inverse-CDF draws of the gridded density p: the cell from the fp64 cumulative sum of the fp32 weights p + 1e-15 at
    target = rnd[:, 0] * total, the point by place64 -> (cell[size], x[size, d], gap[size], total).  gap is the distance
    from the target to the nearer end of the cell's CDF interval: a draw whose gap is within the summation-order error of
    the total may land in a neighbouring cell."""
    cdf = cdf64(p)
    total = cdf[-1]
    target = rnd[:, 0].double().cpu() * total
    cell = torch.searchsorted(cdf, target.contiguous(), right=True).clamp(max=cdf.numel() - 1)
    below = torch.where(cell > 0, cdf[(cell - 1).clamp(min=0)], torch.zeros_like(target))
    gap = torch.minimum((target - below).abs(), (cdf[cell] - target).abs())
    return cell, place64(cell, shape, edges, rnd, noise), gap, float(total)


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
