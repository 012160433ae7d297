#!/usr/bin/env python3
"""Throughput of the device-side POD-ANN time loop for up to 20 primary modes (bg_ann_rom_run_wide) against the host-driven
batched iteration, on the reference's second model size (17 -> 32 -> 64 -> 128 -> 256 -> 256 -> 79, ELU; case A of
tests/ann_wide_cases.py at scale 3.0), the committed 17 + 79 basis (tests/golden/rbf_n17.npz) and the bench's (mu1, mu2)
draw.  The two are timed alternately after a warm-up, each run synchronised before the clock stops; prints one JSON line:
sample-Newton-steps/s of both (best and every repetition), the speed-up, the worst per-sample rel-L2 between them and
whether the iteration counts and flags agree.
usage: python tools/time_ann_wide_rom.py [--batch 2048] [--steps 12] [--reps 3] [--projection LSPG]"""
import argparse, json, os, sys, time
import numpy as np, torch
from _timing import REPO
sys.path.insert(0, os.path.join(REPO, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=2048); ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--reps", type=int, default=3); ap.add_argument("--projection", default="LSPG")
a = ap.parse_args()
import bench
import ann_wide_cases as aw
from burgers_hip import rom
X, Up, Us = aw.case_bases(aw.CASE_A)
model = aw.case_model(aw.CASE_A)
mu1, mu2 = bench.mu_shard(a.batch, 1, 0)
proj = rom.PROJ[a.projection.lower()]
dev = torch.device("cuda", 0)
plan = rom._ann_fused_plan(model.to(device=dev, dtype=torch.float32).eval(), 17, 79, 512, torch.float32, dev,
                           "bg_ann_rom_run_wide_limits")
runs = {
    "device": lambda: rom.pod_ann_run_wide(X, np.ones(512), mu1, mu2, 0.05, a.steps, Up, Us, model, proj, plan=plan),
    "host": lambda: rom.pod_ann_run(X, np.ones(512), mu1, mu2, 0.05, a.steps, Up, Us, model, projection=a.projection,
                                    fused=False),
}
last, times = {}, {k: [] for k in runs}
for k, f in runs.items():                                  # warm-up: library load, code objects, allocator
    f(); torch.cuda.synchronize()
for _ in range(a.reps):
    for k, f in runs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = f()
        torch.cuda.synchronize()
        times[k].append(time.perf_counter() - t0)
        last[k] = res
assert last["device"].path == "bg_ann_rom_run_wide" and last["host"].path == "host"
its = {k: int(r.iters.sum().item()) for k, r in last.items()}
d, h = last["device"].hist.flatten(1), last["host"].hist.flatten(1)
worst = float(((d - h).norm(dim=1) / h.norm(dim=1)).max())
di = (last["device"].iters - last["host"].iters).abs()
best = {k: min(v) for k, v in times.items()}
out = {"batch": a.batch, "steps": a.steps, "projection": a.projection, "newton_steps": its["device"],
       "capped_samples": int((last["device"].flags & 1).ne(0).sum().item()),
       "device_s": times["device"], "host_s": times["host"],
       "device_rate": its["device"] / best["device"], "host_rate": its["host"] / best["host"],
       "device_rates": [its["device"] / t for t in times["device"]], "host_rates": [its["host"] / t for t in times["host"]],
       "speedup": best["host"] / best["device"], "slowest_device_over_fastest_host": max(times["device"]) / best["host"],
       "worst_rel_l2": worst, "max_count_difference": int(di.max().item()),
       "steps_with_another_count": float((di > 0).float().mean().item()),
       "same_flags": bool(torch.equal(last["device"].flags, last["host"].flags))}
print(json.dumps(out))
