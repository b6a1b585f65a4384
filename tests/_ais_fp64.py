"""fp64 verifier of the transitions of annealed importance sampling on the MENT log-density (tests/test_ais_*.py):
_mala_fp64.verify generalised to a temperature per transition.

With lp, g the MENT log-density and its gradient, the base q0 = N(m, diag b^2) with lq(x) = c0 - 0.5 sum ((x_j - m_j) / b_j)^2 and
gq_j = -(x_j - m_j) / b_j^2, the tempered density at temperature B is
    l_B = B > 0 ? lq + B (lp - lq) : lq,        g_B = l_B == -inf ? 0 : (B > 0 ? gq + B (g - gq) : gq),
and a transition is mala.hip's with l -> l_B and g -> g_B (mentflow_amd/csrc/ment_langevin.h, ais.hip), so _mala_fp64.verify
judges it, given below what stands in the place of l, g, the band and the clamp error.  Every transition is judged from the
sampler's OWN previous state (the `out` rows of ops.ais_ment_steps), so an fp32 chain and the fp64 yardstick cannot drift apart.

Proposal.  The kernel and mf_ment_logprob call one device function, so the fp32 lp32 and g32 that ops.ment_logprob returns for x
on the same backend are the ones the kernel used, bit for bit.  g_B is restated in fp32 in the order the header of ais.hip gives
(ib = 1 / b; t = (x - m) * ib; gq = -(t * ib); g_B = gq + B * (g32 - gq); one rounding per operation, nothing fused, so torch's
fp32 operations give the kernel's bits), then as in _mala_fp64: base = fp32(x + fp32 clamp(fp32(a g_B), -c, c)) and y = s z + base
in fp64.  An accepted state lies within 2 ulp per component of y (_mala_fp64's tolerance: the kernel fuses nothing that is not
restated here), a rejected one is bitwise x, anything else is malformed.

Decision, in fp64 at that y, by _mala_fp64's rule on l_B and g_B, within the band
    b = B [3e-4 (2 + |l64(x)| + |l64(y)|) + sum_j |r_j| 0.5 s_j 3e-4 (1 + |g64(y)|_inf)]
      + 2e-6 [(2 + |lq(x)| + |lq(y)| + B (|l64(x)| + |l64(y)|)) + sum_j |r_j| 0.5 s_j (1 + |gq(y)|_inf)].
The first line is _mala_fp64's band scaled by B where it multiplies lp.  The second is fp32 rounding of what the kernel adds to
lp: lq takes at most d + 4 <= 12 operations and l_B three more, each within 2^-24 = 6e-8 of its operands' magnitude, and terms of
one sign in lq (c0 < 0 for b >= 1 is not assumed: the magnitudes are added), so 15 * 6e-8 < 1e-6 per unit of magnitude; 2e-6
leaves a factor 2.  gq takes three operations; its error enters r as the gradient error does in _mala_fp64.
Ambiguity rules are _mala_fp64's, with the clamp test made on g_B and its error B 3e-4 (1 + |g64|_inf) + 2e-6 (1 + |gq|_inf)."""
import math

import torch

from _mala_fp64 import TOL, assert_transitions  # noqa: F401  (assert_transitions is re-exported)
from _mala_fp64 import verify as _mala_verify

EPS = 2.0e-6


def base_lognorm(base_scale):
    """c0 as the library forms it: fp64, rounded once to fp32."""
    c0 = -0.5 * len(base_scale) * 1.8378770664093453
    for b in base_scale:
        c0 -= math.log(float(torch.tensor(b, dtype=torch.float32)))
    return torch.tensor(c0, dtype=torch.float64).float()


def base32(x, mean, base_scale):
    """(lq, gq) at x in fp32, operation for operation as ais.hip forms them."""
    x = x.detach().float().cpu()
    m = torch.tensor(mean, dtype=torch.float32)
    ib = 1.0 / torch.tensor(base_scale, dtype=torch.float32)
    t = (x - m) * ib
    q = torch.zeros(x.shape[0])
    for j in range(x.shape[1]):
        q = q + t[:, j] * t[:, j]
    return base_lognorm(base_scale) - 0.5 * q, -(t * ib)


def temper32(beta, lp, g, lq, gq):
    """(l_B, g_B) in fp32 from fp32 inputs; beta [n] fp32."""
    hot = beta > 0
    lb = torch.where(hot, lq + beta * (lp - lq), lq)
    gb = torch.where(hot[:, None], gq + beta[:, None] * (g - gq), gq)
    return lb, torch.where(torch.isneginf(lb)[:, None], torch.zeros_like(gb), gb)


def _base64(x, mean, base_scale):
    m = torch.tensor(mean, dtype=torch.float32).double()
    b = torch.tensor(base_scale, dtype=torch.float32).double()
    t = (x.double() - m) / b
    c0 = -torch.log(b).sum() - 0.5 * len(base_scale) * math.log(2 * math.pi)
    return c0 - 0.5 * (t * t).sum(1), -t / b


def _temper64(beta, l, g, lq, gq):
    hot = beta > 0
    safe = torch.where(torch.isneginf(l), torch.zeros_like(l), l)
    lb = torch.where(hot, lq + beta * (safe - lq), lq)
    lb = torch.where(hot & torch.isneginf(l), torch.full_like(lb, float("-inf")), lb)
    gb = torch.where(hot[:, None], gq + beta[:, None] * (g - gq), gq)
    return lb, torch.where(torch.isneginf(lb)[:, None], torch.zeros_like(gb), gb)


class _Tempered:
    """The `base` of _mala_fp64.verify: what the tempered target puts in the place of the plain one's l and g, and of its band and
    clamp errors.  betas [T]: the temperature of each transition; mean, base_scale: d floats."""

    def __init__(self, betas, mean, base_scale):
        self.betas, self.mean, self.base_scale = betas, mean, base_scale

    def per_transition(self, T, C):
        assert tuple(self.betas.shape) == (T,)
        return self.betas.float().cpu()[:, None].expand(T, C).reshape(T * C).contiguous()

    def grad32(self, b32, x, lp32, g32):
        """g_B at x from the backend's own fp32 value and gradient, in the kernel's operation order."""
        lq32, gq32 = base32(x, self.mean, self.base_scale)
        return temper32(b32, lp32.float().cpu(), g32.float().cpu(), lq32, gq32)[1]

    def target64(self, b32, x, y, lx, gx, ly, gy):
        """(l_B, g_B, l, g, lq, gq) at x and at y."""
        B = b32.double()
        lqx, gqx = _base64(x, self.mean, self.base_scale)
        lqy, gqy = _base64(y, self.mean, self.base_scale)
        lbx, gbx = _temper64(B, lx, gx, lqx, gqx)
        lby, gby = _temper64(B, torch.nan_to_num(ly, nan=0.0, neginf=float("-inf")), torch.nan_to_num(gy), lqy, gqy)
        return (lbx, gbx, lx, gx, lqx, gqx), (lby, gby, ly, gy, lqy, gqy)

    def errors(self, b32, tx, ty, rs):
        """(band, gradient error at x, at y) from what target64 returned and rs = sum_j |r_j| 0.5 s_j."""
        B = b32.double()
        (_, _, lx, gx, lqx, gqx), (_, _, ly, gy, lqy, gqy) = tx, ty
        gy_inf, gqy_inf = torch.nan_to_num(gy).abs().amax(1), gqy.abs().amax(1)
        lmag = torch.where(B > 0, lx.abs() + torch.nan_to_num(ly, nan=0.0).abs(), torch.zeros_like(B))    # at B == 0 lp plays no part
        band = B * (TOL * (2 + lmag) + rs * TOL * (1 + gy_inf)) + EPS * ((2 + lqx.abs() + lqy.abs() + B * lmag) + rs * (1 + gqy_inf))
        err_x = B * TOL * (1 + gx.abs().amax(1)) + EPS * (1 + gqx.abs().amax(1))
        return band, err_x, B * TOL * (1 + gy_inf) + EPS * (1 + gqy_inf)


def verify(start, noise, traj, betas, scale, drift_clip, slots, prior64, logp32, mean, base_scale):
    """start [C, d], noise [T, d + 1, C], traj [T, C, d] (the state after every transition), betas [T] (the temperature of
    each transition), scale [d] or float; logp32(x [n, d]) -> (lp32 [n], g32 [n, d]) of mf_ment_logprob at x on the backend
    under test (CPU tensors); mean, base_scale: d floats.  Returns _mala_fp64.verify's dict of counts."""
    return _mala_verify(start, noise, traj, scale, drift_clip, slots, prior64, logp32, base=_Tempered(betas, mean, base_scale))
