#!/usr/bin/env python3
"""Throughput of bg_local_rom_run_long (local POD PROM on meshes of 513 .. 1024 nodes) and, with --host, of the host-driven
iteration that is the default route there, timed alternately in one process.  Everything is built on the device: FOM runs
of the 3 x 3 training grid (200 steps), snapshot SVD truncated at 40 (Phi = U_global), m = 12, 11 centres at U_g^T u of the
LSPG r = 40 POD run at mu = (4.9, 0.022), steps 0, 4, ..., 40, bases Phi[:, :w] for w in 8, 40, 17, 24, 12, 33, 25, 9, 40, 30, 20.
Prints one JSON line per projection: sample-Picard-steps/s of each route (median of --reps), their ratio, the switches.
usage: python tools/time_local_long_rom.py [--batch 1024] [--steps 40] [--n 1024] [--dt 0.025] [--reps 3] [--host]"""
import argparse, json
from _timing import draw, time_alternately, training_snapshots
import numpy as np, torch
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--n", type=int, default=1024); ap.add_argument("--dt", type=float, default=0.025)
ap.add_argument("--reps", type=int, default=3); ap.add_argument("--host", action="store_true")
a = ap.parse_args()
from burgers_hip import pod, rom
N = a.n
X, S = training_snapshots(N, a.dt)
Phi = pod.pod_basis(S, n_modes=40)[0].contiguous()
traj = rom.pod_prom_run(X, np.ones(N), [4.9], [0.022], a.dt, 40, Phi, projection="LSPG", long_mesh=True).hist[0]    # (41, N)
centres = (traj[::4] @ Phi[:, :12]).contiguous()
bases = {c: Phi[:, :w].contiguous() for c, w in enumerate([8, 40, 17, 24, 12, 33, 25, 9, 40, 30, 20])}
mu1, mu2 = draw(a.batch)
plan = rom.LocalPodPlan(centres, bases, Phi, 12, N, Phi.device, long_mesh=True)
assert plan.ok, plan.reason
for proj in ("Galerkin", "LSPG"):
    runs = {"device": lambda: rom.local_prom_run_long(X, np.ones(N), mu1, mu2, a.dt, a.steps, None, None, None, 12,
                                                      projection=proj, plan=plan)}
    if a.host:
        runs["host"] = lambda: rom.local_prom_run(X, np.ones(N), mu1, mu2, a.dt, a.steps, centres, bases, Phi, 12, projection=proj)
    rates, last = time_alternately(runs, a.reps)
    cl = last["device"].clusters
    out = {"projection": proj, "N": N, "batch": a.batch, "steps": a.steps, "dt": a.dt, "path": last["device"].path,
           "switches": int((cl[:, 1:] != cl[:, :-1]).sum().item()), "capped_samples": int((last["device"].flags & 1).ne(0).sum().item()),
           "device_rates": [float(f"{v:.4g}") for v in rates["device"]], "device_rate": float(np.median(rates["device"]))}
    if a.host:
        ok = (last["host"].flags & 1) == 0
        d, h = last["device"].hist[ok].flatten(1), last["host"].hist[ok].flatten(1)
        out.update({"host_path": last["host"].path, "host_rates": [float(f"{v:.4g}") for v in rates["host"]],
                    "host_rate": float(np.median(rates["host"])),
                    "ratio": float(np.median(rates["device"]) / np.median(rates["host"])),
                    "worst_rel_l2_uncapped": float(((d - h).norm(dim=1) / h.norm(dim=1)).max()),
                    "same_clusters_uncapped": bool(torch.equal(last["device"].clusters[ok], last["host"].clusters[ok]))})
    print(json.dumps(out), flush=True)
