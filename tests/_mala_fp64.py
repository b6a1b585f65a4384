"""fp64 verifier of Metropolis-adjusted Langevin transitions on the MENT log-density (tests/test_mala_*.py), built on
_ment_logp_fp64.logp64 in the spirit of _mcmc_fp64.

Every transition is judged from the sampler's OWN previous state x (the trajectory with keep_from=0, keep_every=1), so an fp32
chain and the fp64 yardstick cannot drift apart.  With s = scale, a = s^2 / 2, c = drift_clip s and
drift(p) = clamp(a grad logp(p), -c, c):

Proposal.  The kernel and mf_ment_logprob call one device function, so the fp32 gradient g32 that ops.ment_logprob returns for x
on the same backend is the gradient the kernel used, bit for bit.  y is formed in fp64 from fp32 inputs in the kernel's
operation order: base = fp32(x + fp32 clamp(fp32(a g32), -c, c)), y = s z + base.  An accepted state lies within 2 ulp (fp32
spacing at |y|) per component of y, a rejected one is bitwise x, anything else is malformed.

Decision, in fp64 at that y: r = ((x - y) - drift64(y)) / s, D = (l64(y) - l64(x)) + (sum z^2 - sum r^2) / 2 and the band
    b = 3e-4 (2 + |l64(x)| + |l64(y)|) + sum_j |r_j| 0.5 s_j 3e-4 (1 + |g64(y)|_inf).
3e-4 is the gate _ment_logp_fp64.check_gates holds mf_ment_logprob to, relative to 1 + |l| in value and to 1 + |g|_inf in the
gradient; the first term is that value error of l(x) and l(y), the second the gradient error carried through r (d(r^2 / 2) =
|r| dr, dr = a dg / s = 0.5 s dg).  The band is only valid where the gate is: tables bounded away from zero.
  must accept:  l(y) > -inf ? (l(x) == -inf or log u < D - b) : l(x) == -inf
  must reject:  l(y) > -inf ? (l(x) > -inf and log u > D + b) : l(x) > -inf;  also whenever l(y), u or a z is NaN
  ambiguous:    log u inside the band; or logp64 flags y as ambiguous (a slot within 1e-4 of a bin centre, hull ends included:
                fp32 may pick the neighbouring cell, whose slope enters drift(y), or the other side of the hull); or x lies
                within 1e-4 of a hull end of a slot; or the unclamped drift of x or y lies within the gradient error
                a 3e-4 (1 + |g64|_inf) of +-c (fp32 and fp64 may clamp differently).
x at an INTERIOR bin centre is not ambiguous, which makes the verifier stricter than flagging every point logp64 flags: log p is
continuous there, so the cell fp32 picks changes l(x) by no more than the rounding of any other point, and the one-sided
derivative it picks is not compared at all, since the proposal is rebuilt from the backend's own fp32 gradient.

The transition is the one of mentflow_amd/csrc/ment_langevin.h, which ais.hip restates on a tempered target: `verify` judges that
one too when it is given a `base` (tests/_ais_fp64.py, which states what the base adds to the band and to the clamp test).
Without a base nothing of it is evaluated: no factor 1 and no term 0 enters the plain target's arithmetic."""
import torch

from _mcmc_fp64 import _ulp32
from _ment_logp_fp64 import BAND, logp64

TOL = 3.0e-4


def _near_hull(x, slots):
    """Some slot's projection of x lies within BAND bin widths of the slot's first or last centre."""
    near = torch.zeros(x.shape[0], dtype=torch.bool)
    for rows, coords, _ in slots:
        for r, c in zip(rows, coords):
            c = c.double().cpu()
            s = (x.double() @ r.double().cpu() - c[0]) / ((c[-1] - c[0]) / (c.numel() - 1))
            near |= (s.abs() < BAND) | ((s - (c.numel() - 1)).abs() < BAND)
    return near


def _drift_edge(g, err, c, a):
    """The unclamped drift a g lies within err, the gradient error times a, of the clamp +-c (never with c == 0: the drift is 0
    either way)."""
    return (((a * g).abs() - c).abs() <= err).logical_and(c > 0).any(1)


def verify(start, noise, traj, scale, drift_clip, slots, prior64, grad32, pick=None, base=None):
    """start [C, d], noise [T, d + 1, C], traj [T, C, d] (the state after every step), scale [d] or float; grad32(x [n, d]) ->
    the fp32 gradient of mf_ment_logprob at x on the backend under test (CPU tensor); pick: indices into the T * C transitions
    to judge (default all); base: None, or the tempered target of _ais_fp64 (then grad32 returns (lp32, g32)).  Returns a dict
    of counts."""
    start, noise, traj = start.detach().cpu(), noise.detach().cpu(), traj.detach().cpu()
    T, C, d = traj.shape
    assert tuple(noise.shape) == (T, d + 1, C) and tuple(start.shape) == (C, d)
    b32 = None if base is None else base.per_transition(T, C)
    s32 = torch.as_tensor(scale, dtype=torch.float32).cpu().reshape(-1).expand(d).contiguous()
    prev = torch.cat([start[None], traj[:-1]]).reshape(T * C, d)
    nxt = traj.reshape(T * C, d)
    z = noise[:, :d].permute(0, 2, 1).reshape(T * C, d)
    u = noise[:, d].reshape(T * C)
    if pick is not None:
        prev, nxt, z, u = prev[pick], nxt[pick], z[pick], u[pick]
        b32 = None if base is None else b32[pick]
    n = prev.shape[0]
    # the proposal, from the backend's own fp32 gradient, in the kernel's operation order
    a32, c32 = (0.5 * s32) * s32, torch.tensor(float(drift_clip), dtype=torch.float32) * s32
    g32 = grad32(prev.contiguous())
    g32 = g32.float().cpu() if base is None else base.grad32(b32, prev, *g32)
    y = s32.double() * z.double() + (prev + torch.minimum(torch.maximum(a32 * g32, -c32), c32)).double()
    nan = torch.isnan(y).any(1) | torch.isnan(u)
    y_clean = torch.where(nan[:, None], torch.zeros_like(y), y)
    # the decision in fp64
    s, a, c = s32.double(), a32.double(), c32.double()
    lx, gx, _ = logp64(prev, slots, prior64)
    ly, gy, amb_y = logp64(y_clean, slots, prior64)
    nan |= torch.isnan(ly)
    if base is not None:                                   # the target's value and gradient: l_B and g_B for l and g
        tx, ty = base.target64(b32, prev, y_clean, lx, gx, ly, gy)
        (lx, gx), (ly, gy) = tx[:2], ty[:2]
    r = ((prev.double() - y_clean) - torch.minimum(torch.maximum(a * gy, -c), c)) / s
    delta = (ly - lx) + 0.5 * ((z.double() ** 2).sum(1) - (r ** 2).sum(1))
    rs = (r.abs() * 0.5 * s).sum(1)
    if base is None:
        band = TOL * (2 + lx.abs() + ly.abs()) + rs * TOL * (1 + gy.abs().amax(1))
        err_x = a * TOL * (1 + gx.abs().amax(1, keepdim=True))
        err_y = a * TOL * (1 + torch.nan_to_num(gy).abs().amax(1, keepdim=True))
    else:
        band, err_x, err_y = base.errors(b32, tx, ty, rs)
        err_x, err_y = a * err_x[:, None], a * err_y[:, None]
    log_u = torch.log(u.double())
    x_out, y_in = torch.isneginf(lx), ly > float("-inf")
    must_accept = torch.where(y_in, x_out | (log_u < delta - band), x_out)
    must_reject = torch.where(y_in, ~x_out & (log_u > delta + band), ~x_out)
    edge = _near_hull(prev, slots) | amb_y | _drift_edge(gx, err_x, c, a) | _drift_edge(torch.nan_to_num(gy), err_y, c, a)
    must_accept &= ~edge & ~nan
    must_reject = (must_reject & ~edge) | nan
    in_band = y_in & ~x_out & ~nan & ~(log_u < delta - band) & ~(log_u > delta + band)
    stayed = (nxt.view(torch.int32) == prev.view(torch.int32)).all(1)
    moved_to_y = ((nxt.double() - y).abs() <= 2 * _ulp32(y)).all(1)
    in_band &= ~edge
    return dict(total=n, ambiguous=int((~must_accept & ~must_reject).sum()), in_band=int(in_band.sum()),
                must_accept=int(must_accept.sum()),
                accept_wrong=int((must_accept & ~moved_to_y).sum()), reject_wrong=int((must_reject & ~stayed).sum()),
                malformed=int((~stayed & ~moved_to_y).sum()), accepted=int((~stayed).sum()))


def assert_transitions(stats, cap=0.04):
    """No wrong accept, no wrong reject, nothing malformed; at most `cap` ambiguous: 4 %, the cap of the log-density tests' densest
    case (an fp64 run of the rule alone measured 0.3 .. 1.6 % on the inputs of tests/test_mala_kernels.py)."""
    assert stats["accept_wrong"] == 0 and stats["reject_wrong"] == 0 and stats["malformed"] == 0, stats
    assert stats["ambiguous"] <= cap * stats["total"], stats
