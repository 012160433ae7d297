#!/usr/bin/env python3
"""Throughput and accuracy of bg_hyper_local_rom_run (the hyper-reduced local POD PROM on NNLS-sampled mesh rows) against the
full local PROM of the same clustering: bg_local_rom_run_long up to N = 1024 and, with --host, the host-driven iteration
(the only other route beyond).  The routes are timed alternately in one process: one warm-up of each, then --reps
repetitions between HIP events, every repetition printed.  Everything is built on the device: FOM runs of the 3 x 3 training
grid (200 steps), U_global = the 40 leading left singular vectors, m = 12, 11 centres at U_g^T u of the LSPG r = 40 POD run
at mu = (4.9, 0.022), steps 0, 4, ..., 40; the members of cluster c are the snapshots whose squared distance to centre c is
at most 1.5^2 times their smallest, its basis their leading w left singular vectors, w in 8, 40, 17, 24, 12, 33, 25, 9, 40,
30, 20.  The row sampling is pod.build_local_row_sampling on the nine runs at --tau.  Prints one JSON line per projection:
the rows sampled and the training residual, sample-Picard-steps/s of each route (the hyper loop also with its on-demand
decode), the rate of bg_hyper_rom_run at r = 40 on the same sampling, whether the hyper loop's slowest repetition beats the
full loop's fastest, the worst per-sample rel-L2 against the full local PROM over the samples neither run caps, and the share
of samples whose cluster path differs.
usage: python tools/time_hyper_local_rom.py [--batch 1024] [--steps 40] [--n 1024] [--dt 0.025] [--tau 1e-4] [--reps 3] [--host]"""
import argparse, json
import numpy as np
from _timing import draw, time_alternately, training_list, training_snapshots
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024); ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--n", type=int, default=1024); ap.add_argument("--dt", type=float, default=0.025)
ap.add_argument("--tau", type=float, default=1e-4); ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--host", action="store_true")
a = ap.parse_args()
from burgers_hip import pod, rom
N, MG, WIDTHS = a.n, 12, [8, 40, 17, 24, 12, 33, 25, 9, 40, 30, 20]
X, S = training_snapshots(N, a.dt)
Ug = pod.pod_basis(S, n_modes=40)[0].contiguous()
long_ok = N <= rom._limit(rom._ROUTES["bg_rom_run_long"].max_n)
traj = rom.pod_prom_run(X, np.ones(N), [4.9], [0.022], a.dt, 40, Ug, projection="LSPG", long_mesh=True).hist[0]     # (41, N)
centres = (traj[::4] @ Ug[:, :MG]).contiguous()
d2 = ((S.t() @ Ug[:, :MG])[None, :, :] - centres[:, None, :]).square().sum(-1)                 # (C, snapshots)
bases = {}
for c, w in enumerate(WIDTHS):
    members = S[:, d2[c] <= 1.5 ** 2 * d2.min(0).values].contiguous()
    bases[c] = pod.thin_svd(members)[0][:, :w].contiguous()
train = training_list(S, host=True)
mu1, mu2 = draw(a.batch)
full_plan = rom.LocalPodPlan(centres, bases, Ug, MG, N, Ug.device, long_mesh=True) if long_ok else None
assert full_plan is None or full_plan.ok, full_plan.reason
for proj in ("Galerkin", "LSPG"):
    p = rom.PROJ[proj.lower()]
    s = pod.build_local_row_sampling(X, centres, bases, Ug, MG, train, a.dt, proj, tau=a.tau)
    plan = rom.HyperLocalPlan(centres, bases, Ug, MG, s, X, Ug.device)
    pod_plan = rom.HyperPodPlan(Ug, s, X, Ug.device)
    runs = {"hyper": lambda: rom.local_prom_run_hyper(X, np.ones(N), mu1, mu2, a.dt, a.steps, None, None, None, MG, plan, p)}
    def decoded():                                              # the same with the history decoded, as the full loops write it
        res = runs["hyper"]()
        res.hist
        return res
    runs["decoded"] = decoded
    runs["pod"] = lambda: rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, a.dt, a.steps, None, pod_plan, p)
    if long_ok:
        runs["long"] = lambda: rom.local_prom_run_long(X, np.ones(N), mu1, mu2, a.dt, a.steps, None, None, None, MG, projection=proj,
                                                       plan=full_plan)
    if a.host:
        runs["host"] = lambda: rom.local_prom_run(X, np.ones(N), mu1, mu2, a.dt, a.steps, centres, bases, Ug, MG, projection=proj)
    rates, last = time_alternately(runs, a.reps)
    hy = last["hyper"]
    fmt = lambda v: [float(f"{x:.4g}") for x in v]
    out = {"projection": proj, "N": N, "batch": a.batch, "steps": a.steps, "dt": a.dt, "tau": a.tau, "rows": s.m,
           "training_residual": float(f"{s.residual:.3g}"), "path": hy.path, "picard_steps": int(hy.iters.sum().item()),
           "switches": int((hy.clusters[:, 1:] != hy.clusters[:, :-1]).sum().item()),
           "capped_samples": int((hy.flags & 1).ne(0).sum().item()), "info_nonzero": int(hy.info.ne(0).sum().item()),
           "hyper_rates": fmt(rates["hyper"]), "hyper_rates_with_decode": fmt(rates["decoded"]),
           "pod_hyper_r40_rates": fmt(rates["pod"])}
    for k in ("long", "host"):
        if k not in runs:
            continue
        full = last[k]
        ok = ((full.flags | hy.flags) & 1) == 0
        d, h = hy.hist[ok].flatten(1), full.hist[ok].flatten(1)
        out.update({f"{k}_path": full.path, f"{k}_rates": fmt(rates[k]),
                    f"slowest_hyper_beats_fastest_{k}": bool(min(rates["hyper"]) > max(rates[k])),
                    f"ratio_of_medians_{k}": float(f"{np.median(rates['hyper']) / np.median(rates[k]):.3g}"),
                    f"uncapped_samples_{k}": int(ok.sum().item()),
                    f"worst_rel_l2_uncapped_vs_{k}": float(f"{float(((d - h).norm(dim=1) / h.norm(dim=1)).max()):.3g}"),
                    f"share_other_cluster_path_vs_{k}": float(f"{float((hy.clusters != full.clusters).any(dim=1).double().mean()):.3g}"),
                    f"same_iters_share_vs_{k}": float(f"{float((hy.iters == full.iters).all(dim=1).double().mean()):.3g}")})
    print(json.dumps(out), flush=True)
