#!/usr/bin/env python3
"""Throughput and accuracy of bg_hyper_quad_rom_run (the hyper-reduced quadratic-manifold PROM on NNLS-sampled mesh rows)
against the full quadratic-manifold PROM of the same manifold: bg_quad_rom_run up to N = 512, bg_quad_rom_run_long up to
N = 1024 (the host-driven iteration with --host), the host-driven iteration beyond.  The two routes are timed alternately in
one process: one warm-up of each, then --reps repetitions between HIP events.  The manifold is pod.build_quadratic_manifold
(n = --r, alpha = 1e-2) on the FOM runs of the 3 x 3 training grid, 200 steps, run on the device and factored on the host
(LAPACK: Phi^T H stays at rounding, which the loop requires).  The row sampling is pod.build_quad_row_sampling on those nine
runs with the builder's defaults unless --tau / --min-rows say otherwise.
Prints one JSON line per projection: rows and table nodes, the training residual, sample-Newton-steps/s of each route (all
repetitions; the hyper loop also with its on-demand decode included), whether the hyper loop's slowest repetition beats the
full route's fastest, and the worst per-sample rel-L2 of the hyper-reduced run against the full PROM.
usage: python tools/time_hyper_quad_rom.py [--host] [--n 1024] [--r 40] [--batch 1024] [--steps 40] [--dt DT] [--tau 1e-5] [--min-rows M] [--reps 3]"""
import argparse, json
import numpy as np
from _timing import draw, time_alternately, training_list, training_snapshots
ap = argparse.ArgumentParser()
ap.add_argument("--host", action="store_true"); ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--r", type=int, default=40); ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--steps", type=int, default=40); ap.add_argument("--dt", type=float, default=None)
ap.add_argument("--tau", type=float, default=1e-5); ap.add_argument("--min-rows", type=int, default=None)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
from burgers_hip import pod, rom
N = a.n
dt = a.dt if a.dt is not None else 25.6 / N
X, S = training_snapshots(N, dt)
S = S.cpu()
Phi, H, _ = pod.build_quadratic_manifold(S, a.r, alpha=1e-2)
Phi, H = Phi.contiguous(), H.contiguous()
train = training_list(S)
mu1, mu2 = draw(a.batch)
long_mesh = not a.host and 512 < N <= 1024
full_plan = rom.QuadLongPlan(Phi, H, "cuda") if long_mesh else None           # built once per (Phi, H), outside the timing
worst = lambda x, y: float(((x.flatten(1) - y.flatten(1)).norm(dim=1) / y.flatten(1).norm(dim=1)).max())
for proj in ("Galerkin", "LSPG"):
    s = pod.build_quad_row_sampling(X, Phi, H, train, dt, proj, tau=a.tau, min_rows=a.min_rows)
    plan = rom.HyperQuadPlan(Phi, H, s, X, "cuda")
    runs = {"hyper": lambda: rom.quadratic_run_hyper(X, np.ones(N), mu1, mu2, dt, a.steps, None, None, plan, rom.PROJ[proj.lower()])}
    def decoded():                                              # the same with U = Phi q + H Q(q) formed, as the full loops write it
        res = runs["hyper"]()
        res.hist
        return res
    runs["decoded"] = decoded
    runs["full"] = lambda: rom.quadratic_run(X, np.ones(N), mu1, mu2, dt, a.steps, Phi, H, projection=proj,
                                             fused=not a.host, long_mesh=long_mesh, plan=full_plan)
    rates, last = time_alternately(runs, a.reps)
    hy, full = last["hyper"], last["full"]
    fmt = lambda vs: [float(f"{v:.4g}") for v in vs]
    print(json.dumps({
        "projection": proj, "N": N, "n": a.r, "batch": a.batch, "steps": a.steps, "dt": dt, "tau": a.tau, "rows": s.m,
        "nodes": plan.n_nodes, "training_residual": float(f"{s.residual:.3g}"), "path": hy.path,
        "newton_steps": int(hy.iters.sum().item()), "flagged_samples": int(hy.flags.ne(0).sum().item()),
        "info_nonzero": int(hy.info.ne(0).sum().item()), "hyper_rates": fmt(rates["hyper"]),
        "hyper_rates_with_decode": fmt(rates["decoded"]), "full_path": full.path, "full_rates": fmt(rates["full"]),
        "full_newton_steps": int(full.iters.sum().item()), "full_flagged_samples": int(full.flags.ne(0).sum().item()),
        "slowest_hyper_beats_fastest_full": bool(min(rates["hyper"]) > max(rates["full"])),
        "ratio_of_medians": float(f"{np.median(rates['hyper']) / np.median(rates['full']):.3g}"),
        "hyper_vs_full": float(f"{worst(hy.hist, full.hist):.3g}")}), flush=True)
