"""Time one Gauss-Seidel epoch of classical MENT (mentflow_amd.ment) on the GPU for the shapes of DESIGN.md "Classical MENT".

Per shape: one untimed Gauss-Seidel epoch first (every op of the epoch, the table update included, has then run once: code
objects loaded, allocator warm), then `--repeats` timed epochs (device-synchronised wall time; median, min, max) and
`--repeats` timed sub-steps (simulate of slot (0, 0)), and the HIP-event time of each new kernel family per epoch
(torch.cuda.Event around the ops.ment_* calls; median over the timed epochs).  Problems are built with
mentflow_amd.harness.  Writes <out>/ment_bench.json and prints one line per shape.

    python tools/bench_ment.py --out profiles [--only nd1d] [--repeats 3]
"""
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
from mentflow_amd.ment import MENT  # noqa: E402
from mentflow_amd.sample import GridSampler  # noqa: E402

KERNELS = ("ment_prob", "ment_prob_grid", "ment_block_sums", "ment_sample", "ment_integrate")


class KernelTimer:
    """Wraps the ops.ment_* entry points with HIP events for the duration of a `with` block."""

    def __init__(self):
        self.events = {k: [] for k in KERNELS}
        self.saved = {}

    def __enter__(self):
        for name in KERNELS:
            fn = getattr(ops, name)
            self.saved[name] = fn

            def wrapped(*a, _fn=fn, _name=name, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = _fn(*a, **k)
                e1.record()
                self.events[_name].append((e0, e1))
                return out
            setattr(ops, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(ops, name, fn)

    def report(self):
        torch.cuda.synchronize()
        return {k: {"ms": round(sum(a.elapsed_time(b) for a, b in v), 3), "launches": len(v)} for k, v in self.events.items()
                if v}


def shapes(dev):
    out = {}
    out["2d_linear_integrate_res250"] = lambda: (dict(ndim=2, num=6, bins=85, xmax=4.0, optics="2d_linear", dist_name="rings",
                                                       prior_scale=3.0), dict(mode="integrate", res=250))
    out["nd1d_sample_4d_res33"] = lambda: (dict(ndim=4, num=50, bins=85, xmax=4.0, optics="nd_1d", dist_name="gaussian_mixture",
                                                prior_scale=3.0), dict(mode="sample", res=33, n=1_000_000))
    out["nd2d_corner_sample_4d_res33"] = lambda: (dict(ndim=4, num=6, bins=85, xmax=4.0, optics="nd_2d_corner",
                                                       dist_name="gaussian_mixture", prior_scale=3.0),
                                                  dict(mode="sample", res=33, n=1_000_000))
    for res in (25, 33):
        out[f"c4_sample_6d_res{res}"] = (lambda r=res: (dict(ndim=6, num=100, bins=64, xmax=3.5, optics="nd_1d",
                                                            dist_name="gaussian_mixture", prior_scale=3.0),
                                                       dict(mode="sample", res=r, n=1_000_000)))
    return out


def make_model(pkw, mkw, dev):
    p = build_problem(device=dev, seed=2, meas_samples=500_000, hidden_units=64, **pkw)
    nd = pkw["ndim"]
    lim = pkw["xmax"]
    res = mkw["res"]
    meas_nd = p.diagnostics[0][0].ndim
    kw = dict(ndim=nd, transforms=p.transforms, diagnostics=p.diagnostics, measurements=p.measurements,
              prior=mf.prior.Gaussian(ndim=nd, scale=pkw["prior_scale"]), mode=mkw["mode"], device=dev)
    if mkw["mode"] == "integrate":
        kw.update(integration_limits=[[(nd - meas_nd) * [(-lim, lim)]] for _ in p.transforms],
                  integration_shape=[[(nd - meas_nd) * [res]] for _ in p.transforms])
    else:
        kw.update(sampler=GridSampler(limits=nd * [(-lim, lim)], shape=nd * [res]).to(dev), n_samples=mkw["n"])
    return MENT(**kw)


def spread(values):
    v = sorted(values)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4), n=len(v))


def run(name, factory, dev, repeats):
    pkw, mkw = factory()
    model = make_model(pkw, mkw, dev)
    torch.manual_seed(0)
    model.gauss_seidel_update(lr=0.99)                     # warm-up epoch: every op of an epoch runs once untimed
    torch.cuda.synchronize()
    subs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        model.simulate(0, 0)
        torch.cuda.synchronize()
        subs.append((time.perf_counter() - t0) * 1e3)
    epochs, kernels = [], {}
    for _ in range(repeats):
        with KernelTimer() as kt:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.gauss_seidel_update(lr=0.99)
            torch.cuda.synchronize()
            epochs.append(time.perf_counter() - t0)
        for k, v in kt.report().items():
            kernels.setdefault(k, []).append(v)
    kernels = {k: dict(ms_per_epoch=spread([r["ms"] for r in v]), launches_per_epoch=v[0]["launches"])
               for k, v in kernels.items()}
    preds = model.simulate_all() if mkw["mode"] == "integrate" else None
    kl = float(torch.stack([d.float() for d in model.discrepancy_vector(preds)]).mean()) if preds is not None else None
    nslots = sum(len(d) for d in model.diagnostics)
    rec = dict(shape=name, mode=mkw["mode"], ndim=pkw["ndim"], slots=nslots, bins=pkw["bins"], res=mkw["res"],
               n_samples=mkw.get("n"), substep_ms=spread(subs), epoch_s=spread(epochs), kernels=kernels,
               fully_fused=model.fully_fused(), mean_kl_after_epochs=kl)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from mentflow_amd import _lib
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda", 0)
    recs = []
    for name, factory in shapes(dev).items():
        if args.only and args.only not in name:
            continue
        recs.append(run(name, factory, dev, args.repeats))
    os.makedirs(args.out, exist_ok=True)
    out = dict(device=torch.cuda.get_device_name(0), reference_cpu={"nd1d_sample_4d_res33_substep_s": 4.0,
               "note": "reference MENT._simulate_sample, 8-core CPU, torch + scipy (issue measurement)"}, shapes=recs)
    with open(os.path.join(args.out, "ment_bench.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
