"""fp64 restatement of the gradient of classical MENT's log-density with respect to its Lagrange tables: the yardstick of
tests/test_ment_tabgrad_*.py.

In the log-parametrisation the gradient is a histogram of responsibilities,

    L64[e] = d (sum_n weight_n logp_n) / d log tables[e] = sum_n weight_n rho_e(x_n),

with, in the cell (i, w) that tests/_ment_fp64.interp64 selects for a 1-D slot, h = a (1 - w) + b w and rho = a (1 - w) / h at
node i, b w / h at node i + 1 (four bilinear terms for a 2-D slot).  A factor on the upper clamp (h >= 1e10) is a constant and a
factor h <= 0 cannot occur on a live row; both contribute nothing.  LIVE rows are taken from the kernel's own logp (finite) and
from weight != 0, as the MALA verifier takes the kernel's accept decisions: which side of a hull end an fp32 point falls on is
the forward's decision, and the tests give the rows near a hull end weight 0.

`autograd64` is the same quantity from fp64 autograd with the tables as leaves.  _ment_logp_fp64.logp64 differentiates its sum
in x itself and returns detached values, so its sum (log of interp64's factors, the clamp's constants masked out) is restated
here on the same interp64 and pinned to logp64's values by tests/test_ment_tabgrad_kernels.py."""
import math

import torch

from _ment_fp64 import interp64


def _cell(c, u):
    c = c.double().cpu()
    i = (torch.searchsorted(c, u.contiguous(), right=True) - 1).clamp(0, c.numel() - 2)
    inside = (u >= c[0]) & (u <= c[-1])
    return i, (u - c[i]) / (c[i + 1] - c[i]), inside


def closed_form64(x, slots, live, weight):
    """slots: [(rows [k][d], coords [k], values)] in the order of the kernel's concatenated tables; live [n] bool; weight [n].
    Returns (L64, A), both [sum of table sizes] fp64: the gradient in the log-tables and A[e] = sum |weight_n| over the live
    points whose cell has e as a node."""
    x = x.detach().double().cpu()
    wt = torch.where(live.cpu(), weight.detach().double().cpu(), torch.zeros(x.shape[0], dtype=torch.float64))
    out, reach = [], []
    for rows, coords, values in slots:
        v = values.detach().double().cpu()
        L = torch.zeros(v.numel(), dtype=torch.float64)
        A = torch.zeros(v.numel(), dtype=torch.float64)
        if len(coords) == 1:
            i, w, inside = _cell(coords[0], x @ rows[0].double().cpu())
            nodes = [(i, v[i] * (1 - w)), (i + 1, v[i + 1] * w)]
        else:
            By = v.shape[1]
            i, a, in0 = _cell(coords[0], x @ rows[0].double().cpu())
            k, b, in1 = _cell(coords[1], x @ rows[1].double().cpu())
            inside = in0 & in1
            nodes = [(i * By + k, v[i, k] * (1 - a) * (1 - b)), (i * By + k + 1, v[i, k + 1] * (1 - a) * b),
                     ((i + 1) * By + k, v[i + 1, k] * a * (1 - b)), ((i + 1) * By + k + 1, v[i + 1, k + 1] * a * b)]
        h = sum(term for _, term in nodes)
        ok = inside & (h > 0.0) & (h < 1.0e10) & (wt != 0)
        for e, term in nodes:
            L.index_add_(0, e[ok], (wt * term / h)[ok])
            A.index_add_(0, e[ok], wt.abs()[ok])
        out.append(L)
        reach.append(A)
    return torch.cat(out), torch.cat(reach)


def autograd64(x, slots, live, weight):
    """(d S / d tables [sum of table sizes], logp [n]) for S = sum over live rows of weight_n logp_n, by fp64 autograd with the
    tables as leaves; logp is the restated sum of _ment_logp_fp64.logp64 without a prior (-inf where a factor is <= 0)."""
    x = x.detach().double().cpu()
    leaves = [values.detach().double().cpu().clone().requires_grad_(True) for _, _, values in slots]
    total = torch.zeros(x.shape[0], dtype=torch.float64)
    dead = torch.zeros(x.shape[0], dtype=torch.bool)
    for (rows, coords, _), leaf in zip(slots, leaves):
        u = torch.stack([x @ r.double().cpu() for r in rows], dim=1)
        h = interp64(coords, leaf, u)
        zero, top = h <= 0.0, h >= 1.0e10
        dead |= zero.detach()
        t = torch.log(torch.where(zero | top, torch.ones_like(h), h))
        total = total + torch.where(top, torch.full_like(t, math.log(1.0e10)), t)
    keep = live.cpu() & ~dead
    wt = torch.where(keep, weight.detach().double().cpu(), torch.zeros_like(total))
    grads = torch.autograd.grad((wt * total).sum(), leaves)
    value = total.detach().clone()
    value[dead] = float("-inf")
    return torch.cat([g.reshape(-1) for g in grads]), value
