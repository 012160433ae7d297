#!/usr/bin/env python3
"""Throughput of the device-side POD-RBF time loop (bg_rbf_rom_run) against the host-driven batched iteration, on the
reference's 300-centre closure (tests/golden/rbf_n17.npz) and the bench's (mu1, mu2) draw.  The two are timed alternately
after a warm-up, each run synchronised before the clock stops; prints sample-Newton-steps/s of both and the worst
per-sample rel-L2 between them.
usage: python tools/time_rbf_rom.py [--batch 2048] [--steps 12] [--reps 3] [--projection LSPG] [--kernel gaussian]"""
import argparse, json, os, time
import numpy as np, torch
from _timing import GOLDEN
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=2048); ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--reps", type=int, default=3); ap.add_argument("--projection", default="LSPG")
ap.add_argument("--kernel", default="gaussian", choices=("gaussian", "imq"))
a = ap.parse_args()
import bench
from burgers_hip import rom
g = np.load(os.path.join(GOLDEN, "rbf_n17.npz"))
cl = (g["U_p"], g["U_s"], g["X_train"], g["W_" + a.kernel], float(g["eps_" + a.kernel]), g["x_min"], g["x_max"],
      g["y_min"], g["y_max"])
X = np.linspace(0.0, 100.0, 512)
mu1, mu2 = bench.mu_shard(a.batch, 1, 0)
plan = rom.RbfFusedPlan(*cl, a.kernel, torch.device("cuda", 0))
runs = {
    "device": lambda: rom.pod_rbf_run_fused(X, np.ones(512), mu1, mu2, 0.05, a.steps, *cl, projection=a.projection,
                                            kernel=a.kernel, plan=plan),
    "host": lambda: rom.pod_rbf_run(X, np.ones(512), mu1, mu2, 0.05, a.steps, *cl, projection=a.projection,
                                    kernel=a.kernel, fused=False),
}
last, best = {}, {k: float("inf") for k in runs}
for k, f in runs.items():                                  # warm-up: library load, code objects, allocator
    f(); torch.cuda.synchronize()
for _ in range(a.reps):
    for k, f in runs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = f()
        torch.cuda.synchronize()
        best[k] = min(best[k], time.perf_counter() - t0)
        last[k] = res
assert last["device"].path == "bg_rbf_rom_run" and last["host"].path == "host"
its = {k: int(r.iters.sum().item()) for k, r in last.items()}
d, h = last["device"].hist.flatten(1), last["host"].hist.flatten(1)
worst = float(((d - h).norm(dim=1) / h.norm(dim=1)).max())
same_iters = bool(torch.equal(last["device"].iters, last["host"].iters))
same_flags = bool(torch.equal(last["device"].flags, last["host"].flags))
out = {"batch": a.batch, "steps": a.steps, "projection": a.projection, "kernel": a.kernel,
       "newton_steps": its["device"], "capped_samples": int((last["device"].flags & 1).ne(0).sum().item()),
       "device_s": best["device"], "host_s": best["host"],
       "device_rate": its["device"] / best["device"], "host_rate": its["host"] / best["host"],
       "speedup": best["host"] / best["device"], "worst_rel_l2": worst, "same_iters": same_iters, "same_flags": same_flags}
print(json.dumps(out))
