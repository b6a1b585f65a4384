"""fp64 restatements for the sequential Monte Carlo tests (tests/test_smc_*.py), on the CPU, never derived from the code under
test.

resample64 restates the resampling rule of mf_smc_resample (include/mentflow_hip.h) with plain cumsum; it does not mirror the
kernel's summation order.  Per island of S chains, with m = max logw and w = exp(logw - m) (a logw that is not finite: weight 0):
S1 = sum w, S2 = sum w^2, ess = S1^2 / S2, log mean weight = m + log(S1 / S); the island resamples iff S1 > 0 and ess <
threshold * S; positions pos_j = (u + j) S1 / S, parent = searchsorted(P, pos_j, right), and the last state of weight > 0 where
that finds none.  Because the kernel sums in another order, and compares P_i - j c with u c instead of P_i with (u + j) c, a
position within TOL * S1 of a prefix boundary may fall either side of it: `lo` and `hi` are the parents of pos_j -+ TOL * S1,
a row is ambiguous where they differ, and the kernel's parent must lie in [lo, hi].

SmcPrototype restates the sampler (ladder, islands, bridge, collection) in fp64 torch on logp64 for the statistical gates of
tests/test_smc_api.py.  `python tests/_smc_fp64.py` re-runs it on the configurations of that file and prints the figures
quoted in its docstring and in DESIGN.md 6j."""
import math

import numpy as np
import torch

TOL = 1.0e-11


def _last_positive(w):
    nz = np.nonzero(w > 0)[0]
    return int(nz[-1]) if nz.size else 0


def _parents(P, w, pos):
    S = P.shape[0]
    idx = np.searchsorted(P, pos, side="right")
    return np.where(idx >= S, _last_positive(w), idx)


def resample64(logw, u, groups, threshold):
    """logw [chains] float64, u [groups] float64 in [0, 1).  Returns a dict of numpy arrays: parents, lo, hi [chains] (global
    indices; identity where the island does not resample), weight [chains] (w of each state in its island), stats [groups, 4]
    (log mean weight, ess, resampled, max logw), logw_out [chains] and margin [groups] = |ess - threshold S| / S (inf for an
    island whose weights are all 0)."""
    logw = np.asarray(logw, dtype=np.float64)
    chains = logw.shape[0]
    S = chains // groups
    thr = float(np.float32(threshold))
    out = dict(parents=np.arange(chains), lo=np.arange(chains), hi=np.arange(chains), weight=np.zeros(chains),
               stats=np.zeros((groups, 4)), logw_out=logw.copy(), margin=np.zeros(groups))
    for g in range(groups):
        lw = logw[g * S:(g + 1) * S]
        ok = np.isfinite(lw)
        m = lw[ok].max() if ok.any() else -np.inf
        w = np.where(ok, np.exp(np.where(ok, lw, 0.0) - (m if ok.any() else 0.0)), 0.0)
        P = np.cumsum(w)
        S1, S2 = float(P[-1]), float((w * w).sum())
        ess = S1 * S1 / S2 if S1 > 0 else 0.0
        lmw = m + math.log(S1 / S) if S1 > 0 else -np.inf
        go = S1 > 0 and ess < thr * S
        out["weight"][g * S:(g + 1) * S] = w
        out["stats"][g] = (lmw, ess, float(go), m)
        out["margin"][g] = abs(ess - thr * S) / S if S1 > 0 else np.inf      # an island of weight 0 never resamples
        if not go:
            continue
        pos = (float(u[g]) + np.arange(S, dtype=np.float64)) * (S1 / S)
        for key, shift in (("parents", 0.0), ("lo", -TOL * S1), ("hi", TOL * S1)):
            out[key][g * S:(g + 1) * S] = g * S + _parents(P, w, pos + shift)
        out["logw_out"][g * S:(g + 1) * S] = lmw
    return out


# --------------------------------------------------------------------------------------------------------- the sampler
class SmcPrototype:
    """The sampler in fp64: Langevin transitions of sample.LangevinSampler's docstring on the tempered density
    l_B = lq + B (lp - lq) (lq: the Gaussian base N(0, base^2)), weights logw += (B_k - B_{k-1}) (lp - lq) on reaching
    temperature k, one resampling decision per island after every temperature but the last."""

    def __init__(self, slots, prior, d, chains, groups, n_temps, spt, step, clip, base, threshold, seed):
        from _ment_logp_fp64 import logp64
        self.logp = lambda x: logp64(x, slots, prior)[:2]
        self.d, self.chains, self.groups, self.spt = d, chains, groups, spt
        self.betas = torch.linspace(0.0, 1.0, n_temps + 1, dtype=torch.float64)
        self.step, self.clip, self.base, self.threshold = step, clip, base, threshold
        self.gen = torch.Generator().manual_seed(seed)
        self.rng = np.random.default_rng(seed)
        self.accepted = self.moves = 0

    def set_slots(self, slots, prior):
        from _ment_logp_fp64 import logp64
        self.logp = lambda x: logp64(x, slots, prior)[:2]

    def _tempered(self, x, beta):
        lp, g = self.logp(x)
        t = x / self.base
        lq = -self.d * math.log(self.base) - 0.5 * self.d * math.log(2 * math.pi) - 0.5 * (t * t).sum(1)
        gq = -t / self.base
        out = torch.isneginf(lp)
        safe = torch.where(out, torch.zeros_like(lp), lp)
        lb = lq + beta * (safe - lq)
        gb = gq + beta * (g - gq)
        if beta > 0:
            lb = torch.where(out, torch.full_like(lb, float("-inf")), lb)
            gb = torch.where(out[:, None], torch.zeros_like(gb), gb)
        return lb, gb, lp, lq

    def _moves(self, x, beta, n):
        s, a, c = self.step, 0.5 * self.step ** 2, self.clip * self.step
        lb, gb, lp, lq = self._tempered(x, beta)
        for _ in range(n):
            z = torch.randn(x.shape, dtype=torch.float64, generator=self.gen)
            u = torch.rand(x.shape[0], dtype=torch.float64, generator=self.gen)
            y = x + (a * gb).clamp(-c, c) + s * z
            lby, gby, lpy, lqy = self._tempered(y, beta)
            r = (x - y - (a * gby).clamp(-c, c)) / s
            delta = (lby - lb) + 0.5 * ((z * z).sum(1) - (r * r).sum(1))
            outside = torch.isneginf(lb)
            acc = torch.where(lby > float("-inf"), outside | (torch.log(u) < delta), torch.isneginf(lby) & outside)
            x = torch.where(acc[:, None], y, x)
            gb = torch.where(acc[:, None], gby, gb)
            lb, lp, lq = torch.where(acc, lby, lb), torch.where(acc, lpy, lp), torch.where(acc, lqy, lq)
            self.accepted += int(acc.sum())
            self.moves += x.shape[0]
        return x, lp, lq

    def _resample(self, x, logw, threshold):
        r = resample64(logw.numpy(), self.rng.random(self.groups), self.groups, threshold)
        idx = torch.from_numpy(r["parents"])
        return x[idx], torch.from_numpy(r["logw_out"]), idx

    def run(self):
        x = self.base * torch.randn(self.chains, self.d, dtype=torch.float64, generator=self.gen)
        logw = torch.zeros(self.chains, dtype=torch.float64)
        _, _, lp, lq = self._tempered(x, 0.0)
        K = self.betas.numel() - 1
        for k in range(1, K + 1):
            inc = (self.betas[k] - self.betas[k - 1]) * (torch.where(torch.isneginf(lp), torch.zeros_like(lp), lp) - lq)
            logw = logw + torch.where(torch.isneginf(lp), torch.full_like(inc, float("-inf")), inc)
            x, lp, lq = self._moves(x, float(self.betas[k]), self.spt)
            if k < K and self.threshold > 0:
                x, logw, idx = self._resample(x, logw, self.threshold)
                lp, lq = lp[idx], lq[idx]
        self.x, self.logw, self.lp = x, logw, lp
        return self.figures()

    def bridge(self, bridge_steps):
        """Reweight the kept population to the density now set, resample once, move; returns the smallest island ess / S seen
        before the resampling."""
        lp_new, _ = self.logp(self.x)
        dead = torch.isneginf(self.logw) | torch.isneginf(lp_new)
        inc = torch.where(dead, torch.zeros_like(lp_new), lp_new) - torch.where(dead, torch.zeros_like(lp_new), self.lp)
        logw = torch.where(dead, torch.full_like(inc, float("-inf")), self.logw + inc)
        worst = float(resample64(logw.numpy(), np.zeros(self.groups), self.groups, 0.0)["stats"][:, 1].min()) * self.groups / self.chains
        x, lp = self.x, lp_new
        if self.threshold > 0:
            x, logw, idx = self._resample(x, logw, self.threshold)
            lp = lp[idx]
        if bridge_steps:
            x, lp, _ = self._moves(x, 1.0, bridge_steps)
        self.x, self.logw, self.lp = x, logw, lp
        return worst

    def collect(self, size, thin):
        x, logw, idx = self._resample(self.x, self.logw, 2.0)
        lp = self.lp[idx]
        rows = []
        for _ in range(max(1, math.ceil(size / self.chains))):
            x, lp, _ = self._moves(x, 1.0, thin)
            rows.append(x)
        self.x, self.logw, self.lp = x, logw, lp
        return torch.cat(rows)[:size]

    def figures(self):
        """log_z, log_z_se (the spread of the islands), ess / C and the entropy from the current weights."""
        per = self.logw.view(self.groups, -1)
        lzg = torch.logsumexp(per, 1) - math.log(per.shape[1])
        log_z = float(torch.logsumexp(lzg, 0)) - math.log(self.groups)
        se = float(torch.exp(lzg - log_z).std(unbiased=True)) / math.sqrt(self.groups) if self.groups > 1 else float("nan")
        wt = torch.exp(self.logw - torch.logsumexp(self.logw, 0))
        ess = float(1.0 / (wt * wt).sum())
        h = log_z - float(torch.where(wt > 0, wt * self.lp, torch.zeros_like(wt)).sum())
        return dict(log_z=log_z, log_z_se=se, ess_over_c=ess / self.chains, entropy=h,
                    accept=self.accepted / max(1, self.moves))


def _main():
    """The prototype on the configurations of tests/test_smc_api.py, five seeds each (ten for the bridge)."""
    from test_ais_api import CENTRES, build, reference
    common = dict(chains=2048, groups=8, spt=2, step=0.5, clip=1.0, base=1.5)
    prior = ("gaussian", 3.0)
    for case, n_temps, thr in (("b", 8, 0.5), ("b", 8, 1.1), ("a", 32, 1.1), ("b", 8, 0.0)):
        _, slots = build(case, torch.device("cpu"))
        ref_z, ref_h = reference(case)
        rows = []
        for seed in range(5):
            f = SmcPrototype(slots, prior, 2 if case == "a" else 6, n_temps=n_temps, threshold=thr, seed=seed, **common).run()
            rows.append((abs(f["log_z"] - ref_z), abs(f["entropy"] - ref_h), f["ess_over_c"], f["accept"], f["log_z_se"]))
        r = np.array(rows)
        print(f"case {case}, {n_temps} temperatures, threshold {thr}: |d log Z| <= {r[:, 0].max():.3f}, |d H| <= {r[:, 1].max():.3f}, "
              f"ess / C {r[:, 2].min():.3f} .. {r[:, 2].max():.3f}, accept {r[:, 3].min():.3f} .. {r[:, 3].max():.3f}, "
              f"island se {r[:, 4].min():.4f} .. {r[:, 4].max():.4f}, |d log Z| / se <= {(r[:, 0] / r[:, 4]).max():.1f}")
    # the bridge: table 0 of case (b) changes by the factor exp(sin(1.3 centres)); every axis by 1-D quadrature
    _, slots = build("b", torch.device("cpu"))
    factor = torch.exp(torch.sin(1.3 * CENTRES))
    new = [(slots[0][0], slots[0][1], slots[0][2] * factor)] + slots[1:]
    new_z, new_mean = bridge_reference(new)
    rows = []
    for seed in range(10):
        p = SmcPrototype(slots, prior, 6, n_temps=8, threshold=0.5, seed=100 + seed, **common)
        p.run()
        p.collect(2048, 2)
        p.set_slots(new, prior)
        worst = p.bridge(4)
        dz = abs(p.figures()["log_z"] - new_z)
        pts = p.collect(65536, 2)
        rows.append((dz, float((pts.mean(0) - new_mean).abs().max()), worst))
    r = np.array(rows)
    print(f"bridge (factor in [{float(factor.min()):.2f}, {float(factor.max()):.2f}]): |d log Z| <= {r[:, 0].max():.3f}, "
          f"|d mean| over the six axes <= {r[:, 1].max():.3f}, island ess / S before resampling >= {r[:, 2].min():.2f}")


def bridge_reference(slots):
    """(log Z, mean [6]) of the factorised 6-D density of case (b) with the given slots, by 1-D trapezoid rules."""
    from _ment_logp_fp64 import logp64
    from test_ais_api import CENTRES, _trapezoid_weights
    lo, hi, n = float(CENTRES[0]), float(CENTRES[-1]), 65537
    t = torch.linspace(lo, hi, n, dtype=torch.float64)
    w = _trapezoid_weights(n, (hi - lo) / (n - 1))
    log_z, mean = 0.0, []
    for rows, coords, values in slots:
        p = torch.exp(logp64(t[:, None], [([torch.ones(1)], coords, values)], ("gaussian", 3.0))[0])
        z = float((w * p).sum())
        log_z += math.log(z)
        mean.append(float((w * p * t).sum()) / z)
    return log_z, torch.tensor(mean, dtype=torch.float64)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from conftest import EMU_LIB
    from mentflow_amd import _lib
    _lib.use_library(EMU_LIB)                     # test_ais_api.build makes a MENT; nothing here computes with the library
    _main()
