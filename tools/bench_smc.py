"""Time the resampling stage of the sequential Monte Carlo sampler (mf_smc_resample) beside one temperature's moves
(mf_ais_ment_steps) on the C4 measurement set in 6-D (100 one-D projections x 64 bins) with 65 536 chains, and a bridge call of
sample.SequentialMonteCarloSampler beside a full-ladder call.  For DESIGN.md section 6j; nothing here is a pass/fail threshold.

Protocol of tools/bench_ais.py.  Each configuration is one process that merges its record into <out>/smc_bench.json, so that
every GPU step can run under a time limit of its own and a failing step ends the chain:

    timeout -k 10 600 python tools/bench_smc.py --out profiles --only stage && \
    timeout -k 10 600 python tools/bench_smc.py --out profiles --only bridge

Every process builds bench_mala.py's problem (seeded) and runs its one untimed Gauss-Seidel epoch with the random-walk sampler:
Lagrange tables with structure and 65 536 chains burnt in inside the support; the tables then stay fixed.
  * stage: `--repeats` timings, each of 20 back-to-back calls between two device events (the first batch is untimed), in
    microseconds per call, of ops.smc_resample on those states in 8 islands with log-weights 3 N(0, 1) (its three output
    allocations included): every island resampling (threshold 1.1) and none (threshold 0: the island pass and a plain copy);
    then of one ops.ais_ment_steps launch of one temperature x 2 transitions on pre-drawn noise, the samplers' default step and
    drift_clip.  The ratio of the medians is what a resampling decision adds to a temperature.
  * bridge: SequentialMonteCarloSampler(65 536 chains, 8 islands, 32 temperatures x 2 transitions, threshold 0.5), wall time
    with a device synchronisation on both sides of sampler(model.prob, 65 536): a first call (the whole ladder and the
    collection), then table 0 is multiplied by exp(0.5 sin(1.3 centres)) and the second call (bridge and collection) is timed;
    `--repeats` times from reset(), after one untimed pair.  log_z before and after and the islands' ess / S in the bridge are
    recorded."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_mala import CHAINS, NDIM, draw_noise, make_model, spread  # noqa: E402
from mentflow_amd import ops  # noqa: E402
from mentflow_amd.sample import SequentialMonteCarloSampler  # noqa: E402

GROUPS, TEMPS, SPT, BATCH = 8, 32, 2, 20
CONFIGS = ("stage", "bridge")


def time_batches(fn, repeats):
    """Microseconds per call: `repeats` batches of BATCH calls between two events, after one untimed batch."""
    times = []
    for i in range(repeats + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(BATCH):
            fn()
        t1.record()
        torch.cuda.synchronize()
        if i:
            times.append(t0.elapsed_time(t1) * 1e3 / BATCH)
    return times


def run_stage(model, dev, repeats, base_scale):
    args = model.fused_args()
    x = model.sampler.state.clone()
    gen = torch.Generator(device=dev).manual_seed(0)
    logw0 = 3.0 * torch.randn(CHAINS, dtype=torch.float64, device=dev, generator=gen)
    u = torch.rand(GROUPS, dtype=torch.float64, device=dev, generator=gen)
    default = SequentialMonteCarloSampler(NDIM, chains=CHAINS, groups=GROUPS, n_temps=TEMPS, steps_per_temp=SPT)
    scale = torch.tensor(default.step, dtype=torch.float32, device=dev)
    betas = default.betas.to(dev)
    noise = draw_noise(SPT, CHAINS, dev)
    mean, base = [0.0] * NDIM, [base_scale] * NDIM
    logw = logw0.clone()
    acc = torch.zeros(CHAINS, dtype=torch.int32, device=dev)
    xm = x.clone()

    def resample(threshold):
        def fn():
            logw.copy_(logw0)
            ops.smc_resample(x, logw, u, GROUPS, threshold)
        return fn

    def restore():
        logw.copy_(logw0)

    def moves():
        ops.ais_ment_steps(xm, *args[:3], args[3], noise, betas, SPT, scale, mean, base, logw, acc, drift_clip=default.drift_clip,
                           temp_offset=TEMPS // 2, ntemps=1)

    t_copy = time_batches(restore, repeats)                # the logw restore that both resampling timings include
    t_all = time_batches(resample(1.1), repeats)
    t_none = time_batches(resample(0.0), repeats)
    stats = ops.smc_resample(x, logw0.clone(), u, GROUPS, 1.1)[2]
    t_moves = time_batches(moves, repeats)
    med = lambda v: sorted(v)[len(v) // 2]
    return dict(config="stage", ndim=NDIM, slots=100, bins=64, chains=CHAINS, groups=GROUPS, steps_per_temp=SPT, step=default.step,
                drift_clip=default.drift_clip, calls_per_timing=BATCH, logw_restore_us=spread(t_copy, 2),
                resample_all_islands_us=spread(t_all, 2), resample_no_island_us=spread(t_none, 2),
                islands_resampled=int(stats[:, 2].sum()), ess_over_island=round(float(stats[:, 1].mean()) * GROUPS / CHAINS, 5),
                one_temperature_moves_us=spread(t_moves, 2),
                resample_over_moves=round((med(t_all) - med(t_copy)) / med(t_moves), 4))


def run_bridge(model, dev, repeats, base_scale, seed):
    s = SequentialMonteCarloSampler(NDIM, chains=CHAINS, groups=GROUPS, n_temps=TEMPS, steps_per_temp=SPT, base_scale=base_scale,
                                    seed=seed).to(dev)
    lf = model.lagrange_functions[0][0]
    old = lf.values.clone()
    centres = torch.linspace(-1.0, 1.0, old.numel(), device=dev) * 3.5
    new = old * torch.exp(0.5 * torch.sin(1.3 * centres))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    full, bridge, rows = [], [], []
    for i in range(repeats + 1):                           # the first pair is untimed
        s.reset()
        lf.set_values(old)
        t_full = timed(lambda: s(model.prob, CHAINS))
        z_old = float(s.log_z)
        lf.set_values(new)
        t_bridge = timed(lambda: s(model.prob, CHAINS))
        if i:
            full.append(t_full)
            bridge.append(t_bridge)
            rows.append(dict(log_z_ladder=round(z_old, 4), log_z_bridge=round(float(s.log_z), 4),
                             bridge_min_ess_over_island=round(float(s.last["ess_groups"].min()) * GROUPS / CHAINS, 4),
                             bridge_islands_resampled=int(s.last["resampled"])))
    lf.set_values(new)
    fresh = SequentialMonteCarloSampler(NDIM, chains=CHAINS, groups=GROUPS, n_temps=TEMPS, steps_per_temp=SPT,
                                        base_scale=base_scale, seed=seed + 1).to(dev)
    fresh(model.prob, CHAINS)
    lf.set_values(old)
    med = lambda v: sorted(v)[len(v) // 2]
    return dict(config="bridge", ndim=NDIM, slots=100, bins=64, chains=CHAINS, groups=GROUPS, n_temps=TEMPS, steps_per_temp=SPT,
                base_scale=base_scale, seed=seed, ess_threshold=s.ess_threshold, bridge_steps=s.bridge_steps, thin=s.thin,
                full_ladder_call_ms=spread(full, 3), bridge_call_ms=spread(bridge, 3),
                full_over_bridge=round(med(full) / med(bridge), 2), log_z_new_tables_fresh_ladder=round(float(fresh.log_z), 4),
                calls=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="", help="one of " + ", ".join(CONFIGS) + " (default: all, in one process)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--base-scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from mentflow_amd import _lib
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda", 0)
    names = [args.only] if args.only else list(CONFIGS)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "smc_bench.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.setdefault("configs", {})
    out["device"] = torch.cuda.get_device_name(0)
    for name in names:
        model = make_model(dev)
        torch.manual_seed(0)
        model.gauss_seidel_update(lr=0.99)                 # untimed: structured tables, chains burnt in inside the support
        assert model.fused_args() is not None
        rec = run_stage(model, dev, args.repeats, args.base_scale) if name == "stage" else run_bridge(model, dev, args.repeats,
                                                                                                       args.base_scale, args.seed)
        print(json.dumps(rec), flush=True)
        out["configs"][name] = rec
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
