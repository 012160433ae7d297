#!/usr/bin/env python3
"""Throughput of bg_quad_rom_run_long (quadratic-manifold PROM on meshes of 513 .. 1024 nodes, n <= 40) or, with --host,
of the host-driven batched iteration that is the default route there.  The manifold is built on the device: FOM runs of
the 3 x 3 training grid (200 steps), pod.build_quadratic_manifold with alpha = 1e-2.
usage: python tools/time_quad_long_rom.py [--batch 1024] [--steps 40] [--n 1024] [--r 40] [--dt 0.025] [--reps 3] [--host]"""
import argparse
import numpy as np
from _timing import draw, peak_text, rates_of, rates_text, time_runs, training_snapshots
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--n", type=int, default=1024); ap.add_argument("--r", type=int, default=40)
ap.add_argument("--dt", type=float, default=0.025); ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--host", action="store_true")
a = ap.parse_args()
from burgers_hip import pod, rom
N, r = a.n, a.r
X, S = training_snapshots(N, a.dt)
Phi, H, _ = pod.build_quadratic_manifold(S, r, alpha=1e-2)
Phi, H = Phi.contiguous(), H.contiguous()
mu1, mu2 = draw(a.batch)
k = r * (r + 1) // 2
flop = 2 * N * (r + k) + 4 * N * k + 2 * N * r ** 2 + 11 * N * r + 2 * r ** 3 / 3      # per sample-Newton-step (bench.py's quadratic config)
plan = None if a.host else rom.QuadLongPlan(Phi, H, Phi.device)                           # built once per (Phi, H), outside the timing
for proj in ("Galerkin", "LSPG"):
    run = lambda: rom.quadratic_run(X, np.ones(N), mu1, mu2, a.dt, a.steps, Phi, H, projection=proj, long_mesh=not a.host, plan=plan)
    ms, res = time_runs(run, a.reps)
    rates = rates_of(ms, res)
    print(f"{res.path} {proj} N={N} n={r} B={a.batch} steps={a.steps} dt={a.dt}: {rates_text(rates)} "
          f"(spread {max(rates) - min(rates):.2g}), iterations {int(res.iters.sum().item())}, "
          f"capped samples {int((res.flags != 0).sum().item())}, {peak_text(rates, flop)}", flush=True)
