#!/usr/bin/env python3
"""Throughput and accuracy of bg_hyper_rom_run (the hyper-reduced POD PROM on NNLS-sampled mesh rows) against the full POD
PROM of the same basis: bg_rom_run_long up to N = 1024, the library path beyond.  The two routes are timed alternately in
one process: one warm-up of each, then --reps repetitions between HIP events.  The basis is built on the device (FOM runs
of the 3 x 3 training grid, 200 steps, snapshot SVD truncated at --r); the row sampling is pod.build_row_sampling on those
nine runs at --tau.  Prints one JSON line per projection: the rows sampled and the training residual, sample-Newton-steps/s
of each route (all repetitions; the hyper loop also with its on-demand decode U = Phi q included), whether the hyper loop's slowest repetition beats the full loop's fastest, whether the
iteration counts are identical, and the worst per-sample rel-L2 of the hyper-reduced run against the full PROM and of both
against the FOM.
usage: python tools/time_hyper_rom.py [--batch 1024] [--steps 40] [--n 1024] [--r 40] [--dt 0.025] [--tau 1e-4] [--reps 3] [--no-full]"""
import argparse, json
import numpy as np, torch
from _timing import draw, time_alternately, training_list, training_snapshots
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--n", type=int, default=1024); ap.add_argument("--r", type=int, default=40)
ap.add_argument("--dt", type=float, default=0.025); ap.add_argument("--tau", type=float, default=1e-4)
ap.add_argument("--reps", type=int, default=3); ap.add_argument("--no-full", action="store_true")
a = ap.parse_args()
from burgers_hip import fom, pod, rom
N = a.n
X, S = training_snapshots(N, a.dt)
Phi = pod.pod_basis(S, n_modes=a.r)[0].contiguous()
train = training_list(S, host=True)
mu1, mu2 = draw(a.batch)
worst = lambda x, y: float(((x.flatten(1) - y.flatten(1)).norm(dim=1) / y.flatten(1).norm(dim=1)).max())
truth = fom.fom_run(X, np.ones(N), mu1, mu2, a.dt, a.steps).hist
for proj in ("Galerkin", "LSPG"):
    s = pod.build_row_sampling(X, Phi, train, a.dt, proj, tau=a.tau)
    plan = rom.HyperPodPlan(Phi, s, X, Phi.device)
    runs = {"hyper": lambda: rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, a.dt, a.steps, None, plan, rom.PROJ[proj.lower()])}
    def decoded():                                              # the same with U = Phi q formed, as the full loops write it
        res = runs["hyper"]()
        res.hist
        return res
    runs["decoded"] = decoded
    if not a.no_full:
        runs["full"] = lambda: rom.pod_prom_run(X, np.ones(N), mu1, mu2, a.dt, a.steps, Phi, projection=proj, long_mesh=True)
    rates, last = time_alternately(runs, a.reps)
    hy = last["hyper"]
    out = {"projection": proj, "N": N, "r": a.r, "batch": a.batch, "steps": a.steps, "dt": a.dt, "tau": a.tau, "rows": s.m,
           "training_residual": float(f"{s.residual:.3g}"), "path": hy.path, "newton_steps": int(hy.iters.sum().item()),
           "flagged_samples": int(hy.flags.ne(0).sum().item()), "info_nonzero": int(hy.info.ne(0).sum().item()),
           "hyper_rates": [float(f"{v:.4g}") for v in rates["hyper"]],
           "hyper_rates_with_decode": [float(f"{v:.4g}") for v in rates["decoded"]], "hyper_vs_fom": float(f"{worst(hy.hist, truth):.3g}")}
    if not a.no_full:
        full = last["full"]
        out.update({"full_path": full.path, "full_rates": [float(f"{v:.4g}") for v in rates["full"]],
                    "slowest_hyper_beats_fastest_full": bool(min(rates["hyper"]) > max(rates["full"])),
                    "ratio_of_medians": float(f"{np.median(rates['hyper']) / np.median(rates['full']):.3g}"),
                    "same_iters": bool(torch.equal(hy.iters, full.iters)), "hyper_vs_full": float(f"{worst(hy.hist, full.hist):.3g}"),
                    "full_vs_fom": float(f"{worst(full.hist, truth):.3g}")})
    print(json.dumps(out), flush=True)
