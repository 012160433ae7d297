#!/usr/bin/env python3
"""Throughput of bg_rom_run_long_wide (POD PROM on meshes of 513 .. 1024 nodes, 41 .. 96 modes) or, with --library, of the
library path that is the default route there.  The basis is built on the device: FOM runs of the 3 x 3 training grid
(200 steps), snapshot SVD truncated at r.  Both projections at every r of --r (default: 96 and 64).
usage: python tools/time_long_wide_rom.py [--batch 1024] [--steps 40] [--n 1024] [--r 96 64] [--dt 0.025] [--reps 3] [--library]"""
import argparse
import numpy as np
from _timing import draw, peak_text, rates_of, rates_text, time_runs, training_snapshots
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--n", type=int, default=1024); ap.add_argument("--r", type=int, nargs="+", default=[96, 64])
ap.add_argument("--dt", type=float, default=0.025); ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--library", action="store_true")
a = ap.parse_args()
from burgers_hip import pod, rom
N = a.n
X, S = training_snapshots(N, a.dt)
modes = pod.pod_basis(S, n_modes=max(a.r))[0].contiguous()
mu1, mu2 = draw(a.batch)
for r in a.r:
    Phi = modes[:, :r].contiguous()
    flop = 2 * N * r ** 2 + 11 * N * r + 2 * r ** 3 / 3             # per sample-Newton-step (BASELINE section 4)
    for proj in ("Galerkin", "LSPG"):
        run = lambda: rom.pod_prom_run(X, np.ones(N), mu1, mu2, a.dt, a.steps, Phi, projection=proj, long_wide=not a.library)
        ms, res = time_runs(run, a.reps)
        rates = rates_of(ms, res)
        print(f"{res.path} {proj} N={N} r={r} B={a.batch} steps={a.steps} dt={a.dt} redone={getattr(res, 'redone', 0)}: "
              f"{rates_text(rates)}, {peak_text(rates, flop)}", flush=True)
