#!/usr/bin/env python3
"""Per-phase shader clocks of the fused quadratic-manifold kernel (bg_quad_rom_run) from a phase-clock build:
  tools/build_variant.sh qt quad_fused.hip -DBG_PHASE_CLOCK [-DBG_QUAD_CHUNK=..]
  BG_LIB_PATH=1d-burgers-equation-roms_amd/build/libvar_qt.so python tools/time_quad_fused.py [--batch 1024] [--steps 40]
Bases: this framework's own training sweep, n = 40 (as bench.py --config quadratic)."""
import argparse
import numpy as np, torch
from _timing import draw, phase_report, time_runs, training_snapshots
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--proj", default="LSPG")
a = ap.parse_args()
from burgers_hip import pod, rom
N = 512
X, S = training_snapshots(N, 0.05, steps=500)
Phi, H, _ = pod.build_quadratic_manifold(S, 40, alpha=1e-2)
dev = torch.device("cuda", torch.cuda.current_device())
plan = rom.QuadFusedPlan(Phi, H, dev)
mu1, mu2 = draw(a.batch)
run = lambda: rom.quadratic_run(X, np.ones(N), mu1, mu2, 0.05, a.steps, Phi, H, projection=a.proj, plan=plan)
(ms,), r = time_runs(run)
names = ["pass start (Phi q)", "tangent tiles", "wait: tangent done", "decode", "assembly + projection", "wait: slab done", "reduce + solve + update", "step start / end"]
rep = phase_report(r, names)
print(f"{a.proj} B={a.batch} steps={a.steps}: {ms:.2f} ms; passes per workgroup (median) {rep.passes:.0f}; kilo-clocks per pass (median over samples):")
for nm, v in zip(names, rep.per_pass):
    print(f"  {nm:28s} {v:7.2f} k")
print(f"  {'total':28s} {rep.total:7.2f} k   = {ms * 1e3 / rep.passes:.1f} us per pass; in-kernel clock {rep.mhz:.0f} MHz")
