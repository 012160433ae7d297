#!/usr/bin/env python3
"""Throughput and accuracy of bg_hyper_ann_rom_run_wide (the hyper-reduced POD-ANN PROM for up to 20 primary modes on
NNLS-sampled mesh rows) against the full POD-ANN PROM of the same bases and closure: bg_ann_rom_run_wide up to N = 512 (the
host-driven iteration with --host), the host-driven iteration pod_ann_run(fused=False) beyond, where it is the only other
route.  The routes are timed alternately in one process: one warm-up of each, then --reps repetitions between HIP events.
The model has the shape of the reference's second POD-ANN model, n = 17, nbar = 79, closure 17 -> 32 -> 64 -> 128 -> 256 ->
256 -> 79 (ELU): a random one (seed 529, weights x 0.5, last layer x 3) on the POD basis built on the device from the FOM
runs of the 3 x 3 training grid, 200 steps.  The row sampling is pod.build_ann_row_sampling on those nine runs at --tau
(--min-rows: default 120); with --every K it is rows 0, K, 2 K, ... with weight K (row 0: 1) instead, which reaches the
larger tables (--n 2049 --every 8: 256 rows, 767 table nodes).  Meshes of the recorded table: --n 512, 1024, 2049, 4096.
Prints one JSON line per projection: rows and table nodes, the training residual, sample-Newton-steps/s of each route (all
repetitions; the hyper loop also with its on-demand decode included), whether the hyper loop's slowest repetition beats the
full route's fastest, and the worst per-sample rel-L2 of the hyper-reduced run against the full PROM.
usage: python tools/time_hyper_ann_wide_rom.py [--host] [--n 1024] [--batch 2048] [--steps 12] [--dt DT] [--tau 1e-4] [--min-rows M] [--every K] [--reps 3]"""
import argparse, json
import numpy as np, torch
from _timing import draw, time_alternately, training_list, training_snapshots
ap = argparse.ArgumentParser()
ap.add_argument("--host", action="store_true"); ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--batch", type=int, default=2048); ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--dt", type=float, default=None); ap.add_argument("--tau", type=float, default=1e-4)
ap.add_argument("--min-rows", type=int, default=120); ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--every", type=int, default=0)
a = ap.parse_args()
import torch.nn as nn
from burgers_hip import pod, rom
N = a.n
dt = a.dt if a.dt is not None else 25.6 / N
dims = [17, 32, 64, 128, 256, 256, 79]
X, S = training_snapshots(N, dt)
U = pod.pod_basis(S, n_modes=dims[0] + dims[-1])[0].cpu()
Up, Us = U[:, :dims[0]].contiguous(), U[:, dims[0]:].contiguous()
torch.manual_seed(529)
layers = []
for i in range(6):
    lin = nn.Linear(dims[i], dims[i + 1])
    with torch.no_grad():
        lin.weight.mul_(0.5)
        if i == 5:
            lin.weight.mul_(3.0); lin.bias.mul_(3.0)
    layers += [lin] + ([nn.ELU()] if i < 5 else [])
model = nn.Sequential(*layers).eval()
train = training_list(S, host=True)
mu1, mu2 = draw(a.batch)
worst = lambda x, y: float(((x.flatten(1) - y.flatten(1)).norm(dim=1) / y.flatten(1).norm(dim=1)).max())
for proj in ("Galerkin", "LSPG"):
    if a.every:
        rows = np.arange(0, N - 1, a.every, dtype=np.int32)
        s = pod.RowSampling(rows, np.where(rows == 0, 1.0, float(a.every)), proj.lower(), 0.0, 0, 0.0)
    else:
        s = pod.build_ann_row_sampling(X, Up, Us, model, train, dt, proj, tau=a.tau, min_rows=a.min_rows)
    plan = rom.HyperAnnWidePlan(Up, Us, model, s, X, "cuda")
    runs = {"hyper": lambda: rom.pod_ann_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, a.steps, None, None, None, plan,
                                                        rom.PROJ[proj.lower()])}
    def decoded():                                              # the same with U = U_p q + U_s q_s formed, as the full loops write it
        res = runs["hyper"]()
        res.hist
        return res
    runs["decoded"] = decoded
    wide = not a.host and N <= 512
    runs["full"] = lambda: rom.pod_ann_run(X, np.ones(N), mu1, mu2, dt, a.steps, Up, Us, model, projection=proj, fused=wide, wide=wide)
    rates, last = time_alternately(runs, a.reps)
    hy, full = last["hyper"], last["full"]
    fmt = lambda vs: [float(f"{v:.4g}") for v in vs]
    print(json.dumps({
        "projection": proj, "N": N, "batch": a.batch, "steps": a.steps, "dt": dt, "tau": a.tau, "rows": s.m, "nodes": plan.n_nodes,
        "workgroups_per_cu": plan.wg_per_cu, "training_residual": float(f"{s.residual:.3g}"), "path": hy.path,
        "newton_steps": int(hy.iters.sum().item()), "flagged_samples": int(hy.flags.ne(0).sum().item()),
        "info_nonzero": int(hy.info.ne(0).sum().item()), "hyper_rates": fmt(rates["hyper"]),
        "hyper_rates_with_decode": fmt(rates["decoded"]), "full_path": getattr(full, "path", None), "full_rates": fmt(rates["full"]),
        "full_newton_steps": int(full.iters.sum().item()), "full_flagged_samples": int(full.flags.ne(0).sum().item()),
        "slowest_hyper_beats_fastest_full": bool(min(rates["hyper"]) > max(rates["full"])),
        "ratio_of_medians": float(f"{np.median(rates['hyper']) / np.median(rates['full']):.3g}"),
        "hyper_vs_full": float(f"{worst(hy.hist, full.hist):.3g}")}), flush=True)
