#!/usr/bin/env python3
"""Throughput and accuracy of bg_hyper_rom_run_wide (the hyper-reduced POD PROM for 41 to 96 modes on NNLS-sampled mesh rows)
against the full POD PROM of the same basis: bg_rom_run_long_wide up to N = 1024, the library path beyond (pod_prom_run's
default there), with --host against the weighted-row library iteration that redoes the samples the loop hands back, and
with --pivot device against itself with the repair kernel in the place of that redo (BG_OPT_PIVOT_ON_DEVICE).
The routes are timed alternately in one process: one warm-up of each, then --reps repetitions between HIP events.  The basis
is built on the device (FOM runs of the 3 x 3 training grid, 200 steps, snapshot SVD truncated at --r); the row sampling is
pod.build_row_sampling on those nine runs at --tau, --stride and --min-rows (host work: about a minute per projection at
r = 96).  Prints one JSON line per projection: the rows sampled and the training residual, sample-Newton-steps/s of each
route (all repetitions; the hyper loop also with its on-demand decode U = Phi q included), the samples redone, whether the
hyper loop's slowest repetition beats the full route's fastest, whether the iteration counts are identical, and the worst
per-sample rel-L2 of the hyper-reduced run against the full PROM and of both against the FOM.  --pivot device adds the rates
of that route, whether its slowest repetition beats the default route's fastest, and the same comparisons for its result.
usage: python tools/time_hyper_wide_rom.py [--batch 1024] [--steps 40] [--n 4096] [--r 96] [--dt 0.00625] [--tau 1e-4]
       [--stride 10] [--min-rows M] [--reps 3] [--host] [--no-full] [--pivot device]"""
import argparse, json, time
import numpy as np, torch
from _timing import draw, time_alternately, training_list, training_snapshots
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--n", type=int, default=4096); ap.add_argument("--r", type=int, default=96)
ap.add_argument("--dt", type=float, default=0.00625); ap.add_argument("--tau", type=float, default=1e-4)
ap.add_argument("--stride", type=int, default=10); ap.add_argument("--min-rows", type=int, default=None)
ap.add_argument("--reps", type=int, default=3); ap.add_argument("--host", action="store_true")
ap.add_argument("--no-full", action="store_true"); ap.add_argument("--pivot", choices=["host", "device"], default="host")
a = ap.parse_args()
from burgers_hip import fom, pod, rom
N = a.n
X, S = training_snapshots(N, a.dt)
Phi = pod.pod_basis(S, n_modes=a.r)[0].contiguous()
train = training_list(S, host=True)
mu1, mu2 = draw(a.batch)
worst = lambda x, y: float(((x.flatten(1) - y.flatten(1)).norm(dim=1) / y.flatten(1).norm(dim=1)).max())
sig = lambda v: float(f"{v:.4g}")
truth = fom.fom_run(X, np.ones(N), mu1, mu2, a.dt, a.steps).hist
for proj in ("Galerkin", "LSPG"):
    p = rom.PROJ[proj.lower()]
    t0 = time.time()
    s = pod.build_row_sampling(X, Phi, train, a.dt, proj, tau=a.tau, stride=a.stride, min_rows=a.min_rows)
    print(f"# {proj}: {s.m} rows sampled in {time.time() - t0:.0f} s on the host", flush=True)
    plan = rom.HyperWidePodPlan(Phi, s, X, Phi.device)
    runs = {"hyper": lambda: rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, a.dt, a.steps, None, plan, p)}
    def decoded():                                              # the same with U = Phi q formed, as the full loops write it
        res = runs["hyper"]()
        res.hist
        return res
    runs["decoded"] = decoded
    if not a.no_full:
        runs["full"] = lambda: rom.pod_prom_run(X, np.ones(N), mu1, mu2, a.dt, a.steps, Phi, projection=proj, long_wide=True)
    if a.pivot == "device":
        runs["device"] = lambda: rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, a.dt, a.steps, None, plan, p, pivot="device")
    if a.host:
        runs["host"] = lambda: rom._pod_prom_run_hyper_library(plan, np.ones(N), mu1, mu2, a.dt, a.steps, p, 0.0, 1e-6, 20)
    rates, last = time_alternately(runs, a.reps)
    hy = last["hyper"]
    out = {"projection": proj, "N": N, "r": a.r, "batch": a.batch, "steps": a.steps, "dt": a.dt, "tau": a.tau, "stride": a.stride,
           "rows": s.m, "training_residual": sig(s.residual), "path": hy.path, "redone": hy.redone,
           "newton_steps": int(hy.iters.sum().item()), "flagged_samples": int(hy.flags.ne(0).sum().item()),
           "info_nonzero": int(hy.info.ne(0).sum().item()), "hyper_rates": [sig(v) for v in rates["hyper"]],
           "hyper_rates_with_decode": [sig(v) for v in rates["decoded"]], "hyper_vs_fom": sig(worst(hy.hist, truth))}
    if not a.no_full:
        full = last["full"]
        out.update({"full_path": full.path, "full_rates": [sig(v) for v in rates["full"]],
                    "slowest_hyper_beats_fastest_full": bool(min(rates["hyper"]) > max(rates["full"])),
                    "ratio_of_medians": sig(np.median(rates["hyper"]) / np.median(rates["full"])),
                    "same_iters": bool(torch.equal(hy.iters, full.iters)), "hyper_vs_full": sig(worst(hy.hist, full.hist)),
                    "full_vs_fom": sig(worst(full.hist, truth))})
    if a.pivot == "device":
        dv = last["device"]
        out.update({"device_rates": [sig(v) for v in rates["device"]], "device_redone": dv.redone,
                    "device_info_nonzero": int(dv.info.ne(0).sum().item()), "device_flagged_samples": int(dv.flags.ne(0).sum().item()),
                    "slowest_device_beats_fastest_hyper": bool(min(rates["device"]) > max(rates["hyper"])),
                    "device_over_hyper_medians": sig(np.median(rates["device"]) / np.median(rates["hyper"])),
                    "device_same_iters_as_hyper": bool(torch.equal(dv.iters, hy.iters)), "device_vs_hyper_q": sig(worst(dv.q, hy.q)),
                    "device_vs_fom": sig(worst(dv.hist, truth))})
        if not a.no_full:
            out.update({"device_same_iters_as_full": bool(torch.equal(dv.iters, last["full"].iters)),
                        "device_vs_full": sig(worst(dv.hist, last["full"].hist))})
    if a.host:
        host = last["host"]
        out.update({"host_rates": [sig(v) for v in rates["host"]],
                    "slowest_hyper_beats_fastest_host": bool(min(rates["hyper"]) > max(rates["host"])),
                    "same_iters_as_host": bool(torch.equal(hy.iters, host.iters)),
                    "hyper_vs_host_q": sig(worst(hy.q, host.q))})
    print(json.dumps(out), flush=True)
