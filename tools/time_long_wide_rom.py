#!/usr/bin/env python3
"""Throughput of bg_rom_run_long_wide (POD PROM on meshes of 513 .. 1024 nodes, 41 .. 96 modes) or, with --library, of the
library path that is the default route there.  The basis is built on the device: FOM runs of the 3 x 3 training grid
(200 steps), snapshot SVD truncated at r.  Both projections at every r of --r (default: 96 and 64).
usage: python tools/time_long_wide_rom.py [--batch 1024] [--steps 40] [--n 1024] [--r 96 64] [--dt 0.025] [--reps 3] [--library]"""
import argparse, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "1d-burgers-equation-roms_amd")]
import numpy as np, torch
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--n", type=int, default=1024); ap.add_argument("--r", type=int, nargs="+", default=[96, 64])
ap.add_argument("--dt", type=float, default=0.025); ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--library", action="store_true")
a = ap.parse_args()
from burgers_hip import fom, pod, rom
N = a.n
X = np.linspace(0, 100, N)
mu1t = np.repeat(np.linspace(4.25, 5.5, 3), 3); mu2t = np.tile(np.linspace(0.015, 0.03, 3), 3)
S = pod.snapshot_matrix(fom.fom_run(X, np.ones(N), mu1t, mu2t, a.dt, 200).hist).contiguous()
modes = pod.pod_basis(S, n_modes=max(a.r))[0].contiguous()
rng = np.random.default_rng(20251121)
mu1, mu2 = rng.uniform(4.25, 5.5, a.batch), rng.uniform(0.015, 0.03, a.batch)
for r in a.r:
    Phi = modes[:, :r].contiguous()
    flop = 2 * N * r ** 2 + 11 * N * r + 2 * r ** 3 / 3             # per sample-Newton-step (BASELINE section 4)
    for proj in ("Galerkin", "LSPG"):
        run = lambda: rom.pod_prom_run(X, np.ones(N), mu1, mu2, a.dt, a.steps, Phi, projection=proj, long_wide=not a.library)
        run(); torch.cuda.synchronize()                             # warm-up
        rates = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); res = run(); e1.record(); torch.cuda.synchronize()
            rates.append(int(res.iters.sum().item()) / e0.elapsed_time(e1) * 1e3)
        med = float(np.median(rates))
        redone = getattr(res, "redone", 0)
        print(f"{res.path} {proj} N={N} r={r} B={a.batch} steps={a.steps} dt={a.dt} redone={redone}: " +
              ", ".join(f"{v:.3g}" for v in rates) +
              f" -> median {med:.3g} sample-Newton-steps/s, {med * flop / 78.6e12:.3f} of the 78.6 TFLOP/s fp64 matrix peak", flush=True)
