"""Time the log-density kernel of classical MENT (mentflow_amd/csrc/ment_logp.hip) on the C4 shape — 6-D, 100 one-D slots x 64
bins, 2 097 152 points — for DESIGN.md §6f.

Protocol of tools/bench_mcmc.py: per configuration an untimed warm-up (every op has then run once), then `--repeats` timed
runs, each a device-synchronised wall time (median, min, max recorded); the kernel configurations add the HIP-event time of
the launch itself.  Each configuration is one process that merges its record into <out>/ment_logp_bench.json, so that every
GPU step can run under a time limit of its own and a failing step ends the chain:

    timeout -k 10 300 python tools/bench_ment_logp.py --out profiles --only kernel_fwd && \
    timeout -k 10 300 python tools/bench_ment_logp.py --out profiles --only kernel_fwd_grad && \
    timeout -k 10 300 python tools/bench_ment_logp.py --out profiles --only torch_fwd && \
    timeout -k 10 300 python tools/bench_ment_logp.py --out profiles --only torch_fwd_grad && \
    timeout -k 10 600 python tools/bench_ment_logp.py --out profiles --only loss_gaussian && \
    timeout -k 10 600 python tools/bench_ment_logp.py --out profiles --only loss_ment_prior

kernel_*: ops.ment_logprob without / with the gradient.  torch_*: the torch composition on the same GPU — one x @ rows.T, a
gather of the two neighbouring table values per slot, log, sum (and autograd for the gradient) — in chunks of 262 144 points
so that its [n, 100] temporaries fit.  loss_*: zero_grad + MENTFlow.loss + backward of the C4 workload of bench.py
(2 097 152 particles) with prior.Gaussian and with prior.MENTPrior over a 100-slot MENT on the same optics."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mentflow_amd as mf  # noqa: E402
from mentflow_amd import ops  # noqa: E402
from mentflow_amd.harness import build_problem  # noqa: E402
from mentflow_amd.ment import MENT, _slot_rows  # noqa: E402
from mentflow_amd.utils import coords_from_edges  # noqa: E402

NDIM, SLOTS, BINS, XMAX, N = 6, 100, 64, 3.5, 2_097_152
CHUNK = 262_144
CONFIGS = ("kernel_fwd", "kernel_fwd_grad", "torch_fwd", "torch_fwd_grad", "loss_gaussian", "loss_ment_prior")
C4 = dict(ndim=NDIM, num=SLOTS, bins=BINS, xmax=XMAX, seed=0, transforms=5, prior_scale=3.0, dist_name="gaussian_mixture",
          optics="nd_1d")


def spread(values):
    v = sorted(values)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4), n=len(v))


def make_slots(dev):
    gen = torch.Generator().manual_seed(64)
    rows = torch.randn(SLOTS, NDIM, generator=gen)
    rows = rows / rows.norm(dim=1, keepdim=True)
    centres = coords_from_edges(torch.linspace(-XMAX, XMAX, BINS + 1))
    tables = 0.25 + 1.75 * torch.rand(SLOTS, BINS, generator=gen)
    desc, meta = [], []
    for k in range(SLOTS):
        dsc, m = _slot_rows([rows[k]], [centres], NDIM)
        desc.append(dsc)
        meta.append(m + [k * BINS])
    x = 1.2 * torch.randn(N, NDIM, generator=gen)
    return (x.to(dev), rows.to(dev), centres.to(dev), tables.to(dev), torch.tensor(desc, dtype=torch.float32).to(dev),
            torch.tensor(meta, dtype=torch.int32).to(dev))


def torch_logp(x, rows, centres, tables, scale):
    """The composition a user would write: projections, cell and weight, a gather of the neighbouring values, log, sum."""
    c0, step = centres[0], (centres[-1] - centres[0]) / (BINS - 1)
    u = x @ rows.T                                                        # [n, slots]
    s = (u - c0) / step
    i = s.floor().clamp(0, BINS - 2).long()
    w = (s - i).clamp(max=1.0)
    base = torch.arange(SLOTS, device=x.device)[None, :] * BINS + i
    flat = tables.reshape(-1)
    h = flat[base] * (1.0 - w) + flat[base + 1] * w
    inside = (u >= c0) & (u <= centres[-1])
    logh = torch.where(inside, torch.log(h.clamp(1e-30, 1e10)), torch.full_like(h, float("-inf")))
    return logh.sum(1) - 0.5 * x.square().sum(1) / scale ** 2


def timed(fn, repeats, events=False):
    fn()                                                                  # warm-up, untimed
    torch.cuda.synchronize()
    wall, dev_ms = [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(e0.elapsed_time(e1))
    rec = dict(wall_ms=spread(wall))
    if events:
        rec["hip_event_ms"] = spread(dev_ms)
    return rec


def run(name, dev, repeats):
    rec = dict(config=name, ndim=NDIM, slots=SLOTS, bins=BINS, points=N)
    if name.startswith(("kernel", "torch")):
        x, rows, centres, tables, desc, meta = make_slots(dev)
        scale = 3.0
        prior = (1, scale, 0.0)
        grad = name.endswith("grad")
        if name.startswith("kernel"):
            tab = tables.reshape(-1).contiguous()
            rec.update(timed(lambda: ops.ment_logprob(x, desc, meta, tab, prior, want_grad=grad), repeats, events=True))
        else:
            def step():
                for a in range(0, N, CHUNK):
                    xc = x[a:a + CHUNK].detach().requires_grad_(grad)
                    lp = torch_logp(xc, rows, centres, tables, scale)
                    if grad:
                        finite = torch.where(torch.isfinite(lp), lp, torch.zeros_like(lp))
                        torch.autograd.grad(finite.sum(), xc)
            rec.update(timed(step, repeats, events=True), chunk=CHUNK)
    else:
        prob = build_problem(device=dev, penalty_parameter=500.0, meas_samples=1_000_000, **C4)
        model = prob.model
        if name == "loss_ment_prior":
            ment = MENT(ndim=NDIM, transforms=prob.transforms, diagnostics=prob.diagnostics, measurements=prob.measurements,
                        prior=mf.prior.Gaussian(ndim=NDIM, scale=3.0), mode="sample", device=dev)
            gen = torch.Generator().manual_seed(1)
            for lf in mf.utils.unravel(ment.lagrange_functions):
                lf.set_values((0.25 + 1.75 * torch.rand(lf.values.shape, generator=gen)).to(dev))
            assert ment.fully_fused()
            model.entropy_estimator = mf.entropy.MonteCarloEntropyEstimator(mf.prior.MENTPrior(ment, pad=1e-12))
        params = list(model.parameters())

        def step():
            for p in params:
                if p.grad is not None:
                    p.grad.zero_()
            L, H, D = model.loss(N)
            L.backward()
        rec.update(timed(step, repeats), workload="c4 of bench.py: zero_grad + MENTFlow.loss + backward (no optimizer step)",
                   prior="MENTPrior(100 slots x 64 bins, pad 1e-12)" if name == "loss_ment_prior" else "Gaussian(scale 3)")
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="", help="one of " + ", ".join(CONFIGS) + " (default: all, in one process)")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    from mentflow_amd import _lib
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda", 0)
    names = [args.only] if args.only else list(CONFIGS)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "ment_logp_bench.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.setdefault("configs", {})
    out["device"] = torch.cuda.get_device_name(0)
    for name in names:
        out["configs"][name] = run(name, dev, args.repeats)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
