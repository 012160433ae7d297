#!/usr/bin/env python3
"""Throughput of bg_rbf_rom_run_long (POD-RBF PROM on meshes of 513 .. 1024 nodes) and, with --host, of the host-driven
iteration that is the default route there, timed alternately in one process.  The closure is the reference's 300-centre one
(tests/golden/rbf_n17.npz) with its bases carried to the N-node mesh and orthonormalised (tests/rbf_long_cases.py); the
parameters are the bench's draw.  One warm-up of each route, then --reps repetitions between HIP events.
Prints one JSON line per projection: sample-Newton-steps/s of each route (all repetitions and the median), the iteration
total, the capped samples, and with --host the ratio, whether counts and flags are identical and the worst per-sample rel-L2.
usage: python tools/time_rbf_long_rom.py [--batch 1024] [--steps 12] [--n 1024] [--dt 0.025] [--reps 3] [--kernel gaussian] [--host]"""
import argparse, json, os, sys
from _timing import REPO, time_alternately
import numpy as np, torch
sys.path.insert(0, os.path.join(REPO, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--n", type=int, default=1024); ap.add_argument("--dt", type=float, default=0.025)
ap.add_argument("--reps", type=int, default=3); ap.add_argument("--kernel", default="gaussian", choices=("gaussian", "imq"))
ap.add_argument("--host", action="store_true")
a = ap.parse_args()
import bench
import rbf_long_cases as rc
from burgers_hip import rom
N = a.n
X, cl = rc.long_mesh(N), rc.closure(N, a.kernel)
mu1, mu2 = bench.mu_shard(a.batch, 1, 0)
plan = rom.RbfFusedPlan(*cl, a.kernel, torch.device("cuda", 0), long_mesh=True)
assert plan.ok
for proj in ("Galerkin", "LSPG"):
    runs = {"device": lambda: rom.pod_rbf_run_long(X, np.ones(N), mu1, mu2, a.dt, a.steps, *cl, projection=proj,
                                                   kernel=a.kernel, plan=plan)}
    if a.host:
        runs["host"] = lambda: rom.pod_rbf_run(X, np.ones(N), mu1, mu2, a.dt, a.steps, *cl, projection=proj, kernel=a.kernel)
    rates, last = time_alternately(runs, a.reps)
    dev = last["device"]
    out = {"projection": proj, "kernel": a.kernel, "N": N, "batch": a.batch, "steps": a.steps, "dt": a.dt, "path": dev.path,
           "newton_steps": int(dev.iters.sum().item()), "capped_samples": int((dev.flags & 1).ne(0).sum().item()),
           "info_nonzero": int(dev.info.ne(0).sum().item()),
           "device_rates": [float(f"{v:.4g}") for v in rates["device"]], "device_rate": float(np.median(rates["device"]))}
    if a.host:
        host = last["host"]
        d, h = dev.hist.flatten(1), host.hist.flatten(1)
        spread = max(max(v) - min(v) for v in rates.values())
        out.update({"host_path": host.path, "host_rates": [float(f"{v:.4g}") for v in rates["host"]],
                    "host_rate": float(np.median(rates["host"])), "host_newton_steps": int(host.iters.sum().item()),
                    "ratio": float(np.median(rates["device"]) / np.median(rates["host"])),
                    "larger_spread": float(f"{spread:.4g}"),
                    "faster_by_more_than_spread": bool(np.median(rates["device"]) - np.median(rates["host"]) > spread),
                    "same_iters": bool(torch.equal(dev.iters, host.iters)), "same_flags": bool(torch.equal(dev.flags, host.flags)),
                    "worst_rel_l2": float(((d - h).norm(dim=1) / h.norm(dim=1)).max())})
    print(json.dumps(out), flush=True)
