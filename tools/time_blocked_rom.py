#!/usr/bin/env python3
"""Throughput of bg_rom_run_blocked (POD PROM, up to 256 modes) against the library path on the thesis' r = 160 and
r = 227 bases, rebuilt from the 9 training runs (eps^2 = 1e-5, 1e-6).
usage: python tools/time_blocked_rom.py [--batch 1024] [--steps 20] [--r 160 227] [--no-library] [--phases]"""
import argparse
import numpy as np
from _timing import draw, phase_report, time_runs, training_snapshots
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--r", type=int, nargs="+", default=[160, 227]); ap.add_argument("--no-library", action="store_true")
ap.add_argument("--phases", action="store_true", help="-DBG_PHASE_CLOCK build of rom_blocked.hip (BG_LIB_PATH): kilo-clocks per phase and pass")
a = ap.parse_args()
from burgers_hip import pod, rom
X, S = training_snapshots(512, 0.05, steps=500)
U, _, s_all = pod.pod_basis(S, 1e-6)
K = {160: pod.n_modes_for_tolerance(s_all, 1e-5), 227: U.shape[1]}
mu1, mu2 = draw(a.batch)
for r in a.r:
    k = K.get(r, r)
    Phi = U[:, :k].contiguous()
    plan = rom.BlockedPodPlan(Phi, U.device)
    for proj in ("Galerkin", "LSPG"):
        p = rom.PROJ[proj.lower()]
        (ms,), res = time_runs(lambda: rom.pod_prom_run_blocked(X, np.ones(512), mu1, mu2, 0.05, a.steps, plan, p))
        if a.phases:
            names = ["lift + assembly", "projection", "solve", "other (q update, final lift, per step)"]
            rep = phase_report(res, names)
            print(f"r={k} {proj}: {ms:.1f} ms, passes per sample (median) {rep.passes:.0f}; kilo-clocks per pass: " +
                  ", ".join(f"{nm} {v:.1f}" for nm, v in zip(names, rep.per_pass)) + f"; total {rep.total:.1f} k at {rep.mhz:.0f} MHz", flush=True)
            continue
        its = int(res.iters.sum().item())
        line = (f"bg_rom_run_blocked {proj} r={k} B={a.batch} steps={a.steps}: {ms:.1f} ms, {its} sample-iterations, "
                f"{its / ms * 1e3:.3g} sample-Newton-steps/s, handed back {res.redone}")
        if not a.no_library:
            (lms,), lres = time_runs(lambda: rom.pod_prom_run(X, np.ones(512), mu1, mu2, 0.05, a.steps, Phi, projection=proj, fused=False))
            lits = int(lres.iters.sum().item())
            line += f"; library path {lms:.1f} ms, {lits / lms * 1e3:.3g} sample-Newton-steps/s, speed-up {(its / ms) / (lits / lms):.2f}x"
        print(line, flush=True)
