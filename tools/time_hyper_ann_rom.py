#!/usr/bin/env python3
"""Throughput and accuracy of bg_hyper_ann_rom_run (the hyper-reduced POD-ANN PROM on NNLS-sampled mesh rows) against the
full POD-ANN PROM of the same bases and closure: bg_ann_rom_run up to N = 512 (the host-driven iteration with --host), the
host-driven iteration pod_ann_run(fused=False) beyond.  The two routes are timed alternately in one process: one warm-up of
each, then --reps repetitions between HIP events.  The closure has the BASELINE shape 5 -> 32 -> 64 -> 128 -> 256 -> 256 -> 91
(ELU): at N = 512 the committed one with its bases (tests/golden/ann_n5.npz), elsewhere a random one (seed 505, weights
x 0.5, last layer x 3) on the POD basis built on the device from the FOM runs of the 3 x 3 training grid, 200 steps.  The
row sampling is pod.build_ann_row_sampling on those nine runs at --tau (--min-rows: default 3 n at N = 512, 120 elsewhere).
Prints one JSON line per projection: rows and table nodes, the training residual, sample-Newton-steps/s of each route (all
repetitions; the hyper loop also with its on-demand decode included), whether the hyper loop's slowest repetition beats the
full route's fastest, and the worst per-sample rel-L2 of the hyper-reduced run against the full PROM.
usage: python tools/time_hyper_ann_rom.py [--host] [--n 1024] [--batch 2048] [--steps 12] [--dt DT] [--tau 1e-4] [--min-rows M] [--reps 3]"""
import argparse, json, os
import numpy as np, torch
from _timing import GOLDEN, draw, time_alternately, training_list, training_snapshots
ap = argparse.ArgumentParser()
ap.add_argument("--host", action="store_true"); ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--batch", type=int, default=2048); ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--dt", type=float, default=None); ap.add_argument("--tau", type=float, default=1e-4)
ap.add_argument("--min-rows", type=int, default=None); ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
import torch.nn as nn
from burgers_hip import pod, rom
N = a.n
dt = a.dt if a.dt is not None else 25.6 / N
dims = [5, 32, 64, 128, 256, 256, 91]
X, S = training_snapshots(N, dt)
layers = []
if N == 512:
    g = np.load(os.path.join(GOLDEN, "ann_n5.npz"))
    Up, Us = torch.as_tensor(g["U_p"]), torch.as_tensor(g["U_s"])
else:
    U = pod.pod_basis(S, n_modes=dims[0] + dims[-1])[0].cpu()
    Up, Us = U[:, :dims[0]].contiguous(), U[:, dims[0]:].contiguous()
torch.manual_seed(505)
for i in range(6):
    lin = nn.Linear(dims[i], dims[i + 1])
    with torch.no_grad():
        if N == 512:
            lin.weight.copy_(torch.from_numpy(g[f"W{i}"])); lin.bias.copy_(torch.from_numpy(g[f"b{i}"]))
        else:
            lin.weight.mul_(0.5)
            if i == 5:
                lin.weight.mul_(3.0); lin.bias.mul_(3.0)
    layers += [lin] + ([nn.ELU()] if i < 5 else [])
model = nn.Sequential(*layers).eval()
train = training_list(S, host=True)
mu1, mu2 = draw(a.batch)
min_rows = a.min_rows if a.min_rows is not None else (None if N == 512 else 120)
worst = lambda x, y: float(((x.flatten(1) - y.flatten(1)).norm(dim=1) / y.flatten(1).norm(dim=1)).max())
for proj in ("Galerkin", "LSPG"):
    s = pod.build_ann_row_sampling(X, Up, Us, model, train, dt, proj, tau=a.tau, min_rows=min_rows)
    plan = rom.HyperAnnPlan(Up, Us, model, s, X, "cuda")
    runs = {"hyper": lambda: rom.pod_ann_run_hyper(X, np.ones(N), mu1, mu2, dt, a.steps, None, None, None, plan, rom.PROJ[proj.lower()])}
    def decoded():                                              # the same with U = U_p q + U_s q_s formed, as the full loops write it
        res = runs["hyper"]()
        res.hist
        return res
    runs["decoded"] = decoded
    runs["full"] = lambda: rom.pod_ann_run(X, np.ones(N), mu1, mu2, dt, a.steps, Up, Us, model, projection=proj,
                                           fused=not a.host and N <= 512)
    rates, last = time_alternately(runs, a.reps)
    hy, full = last["hyper"], last["full"]
    fmt = lambda vs: [float(f"{v:.4g}") for v in vs]
    print(json.dumps({
        "projection": proj, "N": N, "batch": a.batch, "steps": a.steps, "dt": dt, "tau": a.tau, "rows": s.m, "nodes": plan.n_nodes,
        "workgroups_per_cu": plan.wg_per_cu, "training_residual": float(f"{s.residual:.3g}"), "path": hy.path,
        "newton_steps": int(hy.iters.sum().item()), "flagged_samples": int(hy.flags.ne(0).sum().item()),
        "info_nonzero": int(hy.info.ne(0).sum().item()), "hyper_rates": fmt(rates["hyper"]),
        "hyper_rates_with_decode": fmt(rates["decoded"]), "full_path": full.path, "full_rates": fmt(rates["full"]),
        "full_newton_steps": int(full.iters.sum().item()), "full_flagged_samples": int(full.flags.ne(0).sum().item()),
        "slowest_hyper_beats_fastest_full": bool(min(rates["hyper"]) > max(rates["full"])),
        "ratio_of_medians": float(f"{np.median(rates['hyper']) / np.median(rates['full']):.3g}"),
        "hyper_vs_full": float(f"{worst(hy.hist, full.hist):.3g}")}), flush=True)
