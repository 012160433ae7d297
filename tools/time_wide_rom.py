#!/usr/bin/env python3
"""Throughput of bg_rom_run_wide (POD PROM, 41 .. 96 modes) against the library path, committed r = 96 basis.
usage: python tools/time_wide_rom.py [--batch 1024] [--steps 40] [--r 96] [--library]"""
import argparse, os
import numpy as np
from _timing import GOLDEN, draw, phase_report, time_runs
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--r", type=int, default=96); ap.add_argument("--library", action="store_true")
ap.add_argument("--phases", action="store_true", help="-DBG_PHASE_CLOCK build of rom_wide.hip (BG_LIB_PATH): kilo-clocks per phase and pass")
a = ap.parse_args()
from burgers_hip import rom
g = np.load(os.path.join(GOLDEN, "committed_pod_r96.npz"))
Phi = np.ascontiguousarray(g["Phi"][:, :a.r])
X = np.linspace(0, 100, 512)
mu1, mu2 = draw(a.batch)
for proj in ("Galerkin", "LSPG"):
    run = lambda: rom.pod_prom_run(X, np.ones(512), mu1, mu2, 0.05, a.steps, Phi, projection=proj, fused=not a.library)
    (ms,), res = time_runs(run)
    its = int(res.iters.sum().item())
    if a.phases:
        names = ["wait slab + barrier", "lift + assembly", "projection (+ coefficient barrier)", "park", "solve", "update / per-step / pass start"]
        rep = phase_report(res, names)
        print(f"{proj}: {ms:.1f} ms, passes per sample (median) {rep.passes:.0f}; kilo-clocks per pass: " +
              ", ".join(f"{nm} {v:.1f}" for nm, v in zip(names, rep.per_pass)) + f"; total {rep.total:.1f} k at {rep.mhz:.0f} MHz")
        continue
    print(f"{'library path' if a.library else 'bg_rom_run_wide'} {proj} r={a.r} B={a.batch} steps={a.steps}: {ms:.1f} ms, {its} sample-iterations, "
          f"{its / ms * 1e3:.3g} sample-Newton-steps/s" + (f", handed back {res.redone}" if res.path == "bg_rom_run_wide" else ""))
