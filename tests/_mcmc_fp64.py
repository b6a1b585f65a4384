"""fp64 verifier of Metropolis-Hastings transitions on the MENT density (tests/test_mcmc_*.py), built on _ment_fp64.prob64.

Every transition is judged from the sampler's OWN previous state (the trajectory with keep_from=0, keep_every=1), so an fp32
chain and the fp64 yardstick cannot drift apart.  With y = x_t + scale * z, p = prob64 and the band m:
  must accept:  p(y) > 0 ? u p(x_t) < p(y) (1 - m) : p(x_t) == 0
  must reject:  p(y) > 0 ? u p(x_t) > p(y) (1 + m) : p(x_t) > 0;  also whenever p(y) or u is NaN (a NaN proposal is rejected)
  else ambiguous; ambiguous too when a slot's projection of y or x_t lies within 1e-4 bin widths of the slot's first or last
  centre: the hull edge is the density's only discontinuity, and fp32 may put such a point on its other side.
m = 1e-3: three times the 3e-4 at which tests/test_ment_kernels.py gates products of 100 fp32 factors against prob64, so an
fp32 density within that gate can never flip a transition outside the band.

An accepted state must lie within 2 ulp (fp32 spacing at |y|) per component of y formed in fp64 from the fp32 inputs, a
rejected one must be bitwise x_t."""
import torch

from _ment_fp64 import prob64

BAND = 1.0e-3
EDGE_BINS = 1.0e-4


def _ulp32(y):
    """fp32 spacing at |y| (fp64 tensor), not below the subnormal spacing."""
    _, e = torch.frexp(y.abs().float().clamp_min(1.1754944e-38))
    return torch.ldexp(torch.ones_like(y), (e - 24).to(torch.int32)).clamp_min(2.0 ** -149)


def _near_edge(x, slots):
    near = torch.zeros(x.shape[0], dtype=torch.bool)
    for rows, coords, _ in slots:
        for r, c in zip(rows, coords):
            c = c.double().cpu()
            u = x @ r.double().cpu()
            tol = EDGE_BINS * float(c[1] - c[0])
            near |= ((u - c[0]).abs() <= tol) | ((u - c[-1]).abs() <= tol)
    return near


def verify(start, noise, traj, scale, slots, prior=None, band=BAND):
    """start [C, d], noise [T, d + 1, C], traj [T, C, d] (the state after every step), scale [d] or float.
    Returns a dict of counts: total, ambiguous, accept_wrong, reject_wrong, malformed (a state that is neither x_t nor y)."""
    start, noise, traj = start.detach().cpu(), noise.detach().cpu(), traj.detach().cpu()
    T, C, d = traj.shape
    assert tuple(noise.shape) == (T, d + 1, C) and tuple(start.shape) == (C, d)
    scale = torch.as_tensor(scale, dtype=torch.float32).cpu().reshape(-1).expand(d)
    prev = torch.cat([start[None], traj[:-1]]).reshape(T * C, d)
    nxt = traj.reshape(T * C, d)
    z = noise[:, :d].permute(0, 2, 1).reshape(T * C, d)
    u = noise[:, d].reshape(T * C).double()
    y = prev.double() + scale.double() * z.double()
    px, py = prob64(prev, slots, prior), prob64(y, slots, prior)
    nan = torch.isnan(py) | torch.isnan(u)
    pos = py > 0
    must_accept = torch.where(pos, u * px < py * (1 - band), px == 0) & ~nan
    must_reject = torch.where(pos, u * px > py * (1 + band), px > 0) | nan
    edge = _near_edge(torch.nan_to_num(y), slots) | _near_edge(prev.double(), slots)
    must_accept &= ~edge
    must_reject = (must_reject & ~edge) | nan
    stayed = (nxt.view(torch.int32) == prev.view(torch.int32)).all(1)
    moved_to_y = ((nxt.double() - y).abs() <= 2 * _ulp32(y)).all(1)
    return dict(total=T * C, ambiguous=int((~must_accept & ~must_reject).sum()),
                accept_wrong=int((must_accept & ~moved_to_y).sum()), reject_wrong=int((must_reject & ~stayed).sum()),
                malformed=int((~stayed & ~moved_to_y).sum()), accepted=int((~stayed).sum()))


def assert_transitions(stats, cap=0.005):
    assert stats["accept_wrong"] == 0 and stats["reject_wrong"] == 0 and stats["malformed"] == 0, stats
    assert stats["ambiguous"] <= cap * stats["total"], stats
