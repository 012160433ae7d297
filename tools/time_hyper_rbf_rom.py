#!/usr/bin/env python3
"""Throughput and accuracy of bg_hyper_rbf_rom_run (the hyper-reduced POD-RBF PROM on NNLS-sampled mesh rows) against the full
POD-RBF PROM of the same bases and closure: bg_rbf_rom_run_long at 513 <= N <= 1024 (the host-driven iteration with --host),
bg_rbf_rom_run up to 512, the host-driven iteration pod_rbf_run beyond 1024, the only other route there.  The routes are
timed alternately in one process: one warm-up of each, then --reps repetitions between HIP events.  The closure has the
thesis' shape (n = 17, nbar = 79, ~300 centres) and is fitted to the mesh: the POD basis built on the device from the FOM runs
of the 3 x 3 training grid (200 steps), the centres every 6th snapshot in reduced coordinates scaled to [-1, 1] with the
data's min / max, imq kernel, eps = 1, W = solve(K + 1e-8 I, Ys).  The row sampling is pod.build_rbf_row_sampling on those
nine runs with its defaults (--tau, --min-rows).
Prints one JSON line per projection: rows and table nodes, the training residual, sample-Newton-steps/s of each route (all
repetitions and the median; the hyper loop also with its on-demand decode included), the ratio of the medians, the larger
spread of the repetitions and whether the medians differ by more than it, and the worst per-sample rel-L2 of the
hyper-reduced run against the full PROM.
usage: python tools/time_hyper_rbf_rom.py [--host] [--n 1024] [--batch 1024] [--steps 12] [--dt DT] [--tau 1e-4] [--min-rows M] [--reps 3]"""
import argparse, json
import numpy as np, torch
from _timing import draw, time_alternately, training_list, training_snapshots
ap = argparse.ArgumentParser()
ap.add_argument("--host", action="store_true"); ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=12)
ap.add_argument("--dt", type=float, default=None); ap.add_argument("--tau", type=float, default=1e-4)
ap.add_argument("--min-rows", type=int, default=None); ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
from burgers_hip import pod, rom
N, n, nbar, kernel, eps = a.n, 17, 79, "imq", 1.0
dt = a.dt if a.dt is not None else 25.6 / N
X, S = training_snapshots(N, dt)
U = pod.pod_basis(S, n_modes=n + nbar)[0].cpu().numpy()
Up, Us = np.ascontiguousarray(U[:, :n]), np.ascontiguousarray(U[:, n:])
Sh = S.cpu().numpy()
Qp, Qs = (Up.T @ Sh[:, ::6]).T, (Us.T @ Sh[:, ::6]).T
x_min, x_max, y_min, y_max = Qp.min(0), Qp.max(0), Qs.min(0), Qs.max(0)
scale = lambda A, lo, hi: 2.0 * ((A - lo) / np.where(hi - lo < 1e-15, 1.0, hi - lo)) - 1.0
Xt, Ys = scale(Qp, x_min, x_max), scale(Qs, y_min, y_max)
K = 1.0 / np.sqrt(1.0 + eps ** 2 * ((Xt[:, None, :] - Xt[None]) ** 2).sum(-1))
W = np.linalg.solve(K + 1e-8 * np.eye(len(K)), Ys)
cl = (Up, Us, Xt, W, eps, x_min, x_max, y_min, y_max)
train = training_list(Sh)
mu1, mu2 = draw(a.batch)
dev = torch.device("cuda", 0)
full_plan = rom.RbfFusedPlan(*cl, kernel, dev, long_mesh=N > 512) if N <= 1024 and not a.host else None
worst = lambda x, y: float(((x.flatten(1) - y.flatten(1)).norm(dim=1) / y.flatten(1).norm(dim=1)).max())
for proj in ("Galerkin", "LSPG"):
    s = pod.build_rbf_row_sampling(X, *cl, train, dt, proj, kernel=kernel, tau=a.tau, min_rows=a.min_rows)
    plan = rom.HyperRbfPlan(*cl, kernel, s, X, dev)
    runs = {"hyper": lambda: rom.pod_rbf_run_hyper(X, np.ones(N), mu1, mu2, dt, a.steps, *([None] * 9), plan, rom.PROJ[proj.lower()])}
    def decoded():                                              # the same with U = U_p q + U_s q_s formed, as the full loops write it
        res = runs["hyper"]()
        res.hist
        return res
    runs["decoded"] = decoded
    if full_plan is None:
        runs["full"] = lambda: rom.pod_rbf_run(X, np.ones(N), mu1, mu2, dt, a.steps, *cl, projection=proj, kernel=kernel)
    else:
        fused = rom.pod_rbf_run_long if N > 512 else rom.pod_rbf_run_fused
        runs["full"] = lambda: fused(X, np.ones(N), mu1, mu2, dt, a.steps, *cl, projection=proj, kernel=kernel, plan=full_plan)
    rates, last = time_alternately(runs, a.reps)
    hy, full = last["hyper"], last["full"]
    fmt = lambda vs: [float(f"{v:.4g}") for v in vs]
    med = {k: float(np.median(v)) for k, v in rates.items()}
    spread = max(max(rates[k]) - min(rates[k]) for k in ("hyper", "full"))
    print(json.dumps({
        "projection": proj, "N": N, "batch": a.batch, "steps": a.steps, "dt": dt, "tau": a.tau, "rows": s.m, "nodes": plan.n_nodes,
        "workgroups_per_cu": plan.wg_per_cu, "training_residual": float(f"{s.residual:.3g}"), "path": hy.path,
        "newton_steps": int(hy.iters.sum().item()), "flagged_samples": int(hy.flags.ne(0).sum().item()),
        "info_nonzero": int(hy.info.ne(0).sum().item()), "hyper_rates": fmt(rates["hyper"]), "hyper_rate": float(f"{med['hyper']:.4g}"),
        "hyper_rates_with_decode": fmt(rates["decoded"]), "full_path": full.path, "full_rates": fmt(rates["full"]),
        "full_rate": float(f"{med['full']:.4g}"), "full_newton_steps": int(full.iters.sum().item()),
        "full_flagged_samples": int(full.flags.ne(0).sum().item()), "ratio_of_medians": float(f"{med['hyper'] / med['full']:.3g}"),
        "larger_spread": float(f"{spread:.4g}"), "faster_by_more_than_spread": bool(med["hyper"] - med["full"] > spread),
        "hyper_vs_full": float(f"{worst(hy.hist, full.hist):.3g}")}), flush=True)
