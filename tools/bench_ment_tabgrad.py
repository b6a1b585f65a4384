"""Time the table-gradient kernel of classical MENT (mentflow_amd/csrc/ment_tabgrad.hip) on the C4 shape — 6-D, 100 one-D slots x
64 bins, 2 097 152 points — for DESIGN.md §6h.

Protocol of tools/bench_ment_logp.py: per configuration an untimed warm-up (every op has then run once), then `--repeats` timed
runs, each a device-synchronised wall time and the HIP-event time around it (median, min, max recorded).  Each configuration is
one process that merges its record into <out>/ment_tabgrad_bench.json, so that every GPU step can run under a time limit of its
own and a failing step ends the chain:

    timeout -k 10 300 python tools/bench_ment_tabgrad.py --out profiles --only kernel_tables && \
    timeout -k 10 300 python tools/bench_ment_tabgrad.py --out profiles --only kernel_fwd_both && \
    timeout -k 10 300 python tools/bench_ment_tabgrad.py --out profiles --only torch_tables && \
    timeout -k 10 300 python tools/bench_ment_tabgrad.py --out profiles --only torch_fwd_both

kernel_tables: ops.ment_logprob_table_grad alone (zeroing, accumulation and finishing launches plus the wrapper's wmax
reduction and poison select), logp given.  kernel_fwd_both: MentLogProbFn forward and one backward into x and tables.
torch_tables: the torch composition on the same GPU — projections, cell and weight, a gather of the two neighbouring table
values per slot, the two responsibilities, two index_add_ into the flat table — in chunks of 262 144 points so that its [n, 100]
temporaries fit.  torch_fwd_both: that composition's log-density with autograd into x and tables."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ment_logp import BINS, CHUNK, N, NDIM, SLOTS, make_slots, timed, torch_logp  # noqa: E402
from mentflow_amd import ops  # noqa: E402

CONFIGS = ("kernel_tables", "kernel_fwd_both", "torch_tables", "torch_fwd_both")


def torch_table_grad(x, rows, centres, tables, logp, weight):
    """sum_n weight_n rho_e(n) for every table entry, the way a user would write it."""
    c0, step = centres[0], (centres[-1] - centres[0]) / (BINS - 1)
    flat = tables.reshape(-1)
    out = torch.zeros_like(flat)
    for a in range(0, x.shape[0], CHUNK):
        xc, wc = x[a:a + CHUNK], weight[a:a + CHUNK]
        wc = torch.where(torch.isfinite(logp[a:a + CHUNK]), wc, torch.zeros_like(wc))[:, None]
        s = (xc @ rows.T - c0) / step
        i = s.floor().clamp(0, BINS - 2).long()
        w = (s - i).clamp(0.0, 1.0)
        base = torch.arange(SLOTS, device=x.device)[None, :] * BINS + i
        lo, hi = flat[base] * (1.0 - w), flat[base + 1] * w
        r = wc / (lo + hi)
        out.index_add_(0, base.reshape(-1), (lo * r).reshape(-1))
        out.index_add_(0, (base + 1).reshape(-1), (hi * r).reshape(-1))
    return out


def run(name, dev, repeats):
    rec = dict(config=name, ndim=NDIM, slots=SLOTS, bins=BINS, points=N)
    x, rows, centres, tables, desc, meta = make_slots(dev)
    scale = 3.0
    prior = (1, scale, 0.0)
    tab = tables.reshape(-1).contiguous()
    weight = torch.randn(N, generator=torch.Generator().manual_seed(5)).to(dev)
    if name == "kernel_tables":
        logp = ops.ment_logprob(x, desc, meta, tab, prior)[0]
        rec.update(timed(lambda: ops.ment_logprob_table_grad(x, desc, meta, tab, logp, weight), repeats, events=True))
        rec["live_rows"] = int(torch.isfinite(logp).sum())
    elif name == "kernel_fwd_both":
        def step():
            xr, tr = x.detach().requires_grad_(True), tab.detach().requires_grad_(True)
            lp = ops.MentLogProbFn.apply(xr, desc, meta, tr, prior)
            torch.autograd.grad(lp, (xr, tr), weight)
        rec.update(timed(step, repeats, events=True))
    elif name == "torch_tables":
        logp = ops.ment_logprob(x, desc, meta, tab, prior)[0]
        rec.update(timed(lambda: torch_table_grad(x, rows, centres, tables, logp, weight), repeats, events=True), chunk=CHUNK)
    else:
        def step():
            tr = tables.detach().requires_grad_(True)
            for a in range(0, N, CHUNK):
                xc = x[a:a + CHUNK].detach().requires_grad_(True)
                lp = torch_logp(xc, rows, centres, tr, scale)
                finite = torch.where(torch.isfinite(lp), lp, torch.zeros_like(lp))
                torch.autograd.grad((finite * weight[a:a + CHUNK]).sum(), (xc, tr))
        rec.update(timed(step, repeats, events=True), chunk=CHUNK)
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
    path = os.path.join(args.out, "ment_tabgrad_bench.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.setdefault("configs", {})
    out["device"] = torch.cuda.get_device_name(0)
    for name in names:
        out["configs"][name] = run(name, dev, args.repeats)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
