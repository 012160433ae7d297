#!/usr/bin/env python3
"""Throughput of the device-side local POD time loop (bg_local_rom_run) against the host-driven batched iteration, on the
bench's (mu1, mu2) draw.  Clusterings: "fixture" (tests/golden/local_pod.npz: 4 centres, widths 14 / 22 / 30 / 18) and
"dense" (11 centres on the fixture's LSPG trajectory, widths 8 .. 40 of the committed 40-mode basis: a switch every ~15
steps).  The runs are timed alternately after a warm-up, each synchronised before the clock stops.  Prints
sample-Picard-steps/s of both, the speedup, the worst per-sample rel-L2 between them, whether iterations, flags and
cluster sequences are identical (also over the samples that never hit the iteration cap), and the number of cluster
switches.  Two references isolate the cost of the new work:
the fused POD loop (bg_rom_run) on the widest fixture basis at the same B ("pod_rate"), and the local loop with that
basis as the ONLY cluster ("local1"), whose iterations equal bg_rom_run's: their difference per time step is the
nearest-centre pick (the q_g product and the argmin), with no reload after the first step.
usage: python tools/time_local_rom.py [--batch 2048] [--steps 150] [--reps 3] [--projection LSPG] [--clusters fixture]"""
import argparse, json, os, time
import numpy as np, torch
from _timing import GOLDEN
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=2048); ap.add_argument("--steps", type=int, default=150)
ap.add_argument("--reps", type=int, default=3); ap.add_argument("--projection", default="LSPG")
ap.add_argument("--clusters", default="fixture", choices=("fixture", "dense"))
a = ap.parse_args()
import bench
from burgers_hip import rom
g = np.load(os.path.join(GOLDEN, "local_pod.npz"))
X = np.linspace(0.0, 100.0, 512)
Ug = g["U_global"]
if a.clusters == "fixture":
    centres, bases = g["centers"], {c: g[f"basis{c}"] for c in range(4)}
else:
    Phi = np.load(os.path.join(GOLDEN, "committed_pod_r40.npz"))["Phi"]
    centres = (Ug[:, :12].T @ g["U_LSPG"][:, ::3]).T.copy()
    bases = {c: np.ascontiguousarray(Phi[:, :w]) for c, w in enumerate([8, 40, 17, 24, 12, 33, 25, 9, 40, 30, 20])}
mu1, mu2 = bench.mu_shard(a.batch, 1, 0)
dev0 = torch.device("cuda", 0)
plan = rom.LocalPodPlan(centres, bases, Ug, 12, 512, dev0)
assert plan.ok, plan.reason
wide = max(bases, key=lambda c: bases[c].shape[1])
plan1 = rom.LocalPodPlan(centres[wide:wide + 1], {0: bases[wide]}, Ug, 12, 512, dev0)
proj = rom.PROJ[a.projection.lower()]
u0 = np.ones(512)
runs = {
    "device": lambda: rom.local_prom_run_fused(X, u0, mu1, mu2, 0.05, a.steps, None, None, None, 12,
                                               projection=a.projection, plan=plan),
    "host": lambda: rom.local_prom_run(X, u0, mu1, mu2, 0.05, a.steps, centres, bases, Ug, 12, projection=a.projection),
    "local1": lambda: rom.local_prom_run_fused(X, u0, mu1, mu2, 0.05, a.steps, None, None, None, 12,
                                               projection=a.projection, plan=plan1),
    "pod": lambda: rom.pod_prom_run_fused(X, u0, mu1, mu2, 0.05, a.steps, bases[wide], proj),
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
assert last["device"].path == "bg_local_rom_run" and last["host"].path == "host"
its = {k: int(r.iters.sum().item()) for k, r in last.items()}
ok = (last["host"].flags & 1) == 0                      # samples that never hit the iteration cap (see below)
d, h = last["device"].hist.flatten(1), last["host"].hist.flatten(1)
rel = (d - h).norm(dim=1) / h.norm(dim=1)
worst, worst_ok = float(rel.max()), float(rel[ok].max())
cl = last["device"].clusters
same_pod_iters = bool(torch.equal(last["local1"].iters, last["pod"].iters))
out = {"batch": a.batch, "steps": a.steps, "projection": a.projection, "clusters": a.clusters,
       "picard_steps": its["device"], "switches": int((cl[:, 1:] != cl[:, :-1]).sum().item()),
       "device_s": best["device"], "host_s": best["host"],
       "device_rate": its["device"] / best["device"], "host_rate": its["host"] / best["host"],
       "speedup": best["host"] / best["device"], "worst_rel_l2": worst,
       "same_iters": bool(torch.equal(last["device"].iters, last["host"].iters)),
       "same_flags": bool(torch.equal(last["device"].flags, last["host"].flags)),
       "same_clusters": bool(torch.equal(last["device"].clusters, last["host"].clusters)),
       # a sample that hits the cap in some step does not contract there: rounding decides its later steps on either path
       "capped_samples": int((~ok).sum().item()), "worst_rel_l2_uncapped": worst_ok,
       "same_iters_uncapped": bool(torch.equal(last["device"].iters[ok], last["host"].iters[ok])),
       "same_clusters_uncapped": bool(torch.equal(last["device"].clusters[ok], last["host"].clusters[ok])),
       "pod_width": int(bases[wide].shape[1]), "pod_rate": its["pod"] / best["pod"],
       "local1_rate": its["local1"] / best["local1"], "local1_iters_equal_pod": same_pod_iters,
       "pick_us_per_step": (best["local1"] - best["pod"]) / (a.batch * a.steps) * 1e6 * 2 * torch.cuda.get_device_properties(0).multi_processor_count}
print(json.dumps(out))
