#!/usr/bin/env python3
"""Throughput and accuracy of bg_hyper_rom_run_blocked (the hyper-reduced POD PROM for 97 to 256 modes on NNLS-sampled mesh
rows) against the routes the same basis has without it: with --host the weighted-row library iteration on the same rows
(_pod_prom_run_hyper_library, which also redoes the samples the loop hands back) and the full PROM's library path
(_pod_prom_run_library, pod_prom_run's default for these bases), and at N <= 512 also the full device-side loop
bg_rom_run_blocked.  The routes are timed alternately in one process: one warm-up of each, then --reps repetitions between HIP
events, so that the run-to-run spread of every route is in the report.  The basis is built on the device (FOM runs of the 3 x 3
training grid, 200 steps, snapshot SVD truncated at --r).  The row sampling is pod.build_row_sampling on --runs of those nine
runs at --tau, --stride, --min-rows and --solver; the NNLS is host work that grows with the pairs and with r, so the defaults
keep the training set small (three runs, every 20th step).  If the fill to --min-rows (default 3 r) finds no column left to add
-- and only then: every other refusal of the builder ends the run -- the fit is repeated without a fill, which costs the NNLS a
second time, and the report says so ("filled": false); --min-rows 1 asks for the unfilled fit at once.  --max-rows defaults to
the builder's (the loop's limit) for the host solver and to 513 for --solver device, whose NNLS holds 512 active columns.
--all-rows takes every mesh row with unit weight instead (N <= the loop's row limit): the loop is then the exact full PROM.
Prints one JSON line per projection: the rows and the seconds the sampling took, sample-Newton-steps/s of every repetition of
every route, the samples redone, whether the new loop's slowest repetition beats each other route's fastest, the ratio of the
medians, and on the first --check samples the worst rel-L2 of the decoded history and the iteration totals against the full PROM.
usage: python tools/time_hyper_blocked_rom.py [--n 4096] [--dt 0.00625] [--r 160] [--batch 1024] [--steps 12] [--proj both]
       [--host] [--runs 3] [--stride 20] [--min-rows M] [--max-rows M] [--tau 1e-4] [--solver host] [--all-rows] [--reps 2]
       [--check 4]"""
import argparse, json, time
import numpy as np, torch
from _timing import draw, time_alternately, training_list, training_snapshots
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096); ap.add_argument("--dt", type=float, default=0.00625)
ap.add_argument("--r", type=int, default=160); ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--steps", type=int, default=12); ap.add_argument("--proj", choices=["Galerkin", "LSPG", "both"], default="both")
ap.add_argument("--host", action="store_true"); ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--stride", type=int, default=20); ap.add_argument("--min-rows", type=int, default=None)
ap.add_argument("--tau", type=float, default=1e-4); ap.add_argument("--solver", choices=["host", "device"], default="host")
ap.add_argument("--all-rows", action="store_true"); ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--check", type=int, default=4); ap.add_argument("--max-rows", type=int, default=None)
a = ap.parse_args()
from burgers_hip import pod, rom
N = a.n
X, S = training_snapshots(N, a.dt)
Phi = pod.pod_basis(S, n_modes=a.r)[0].contiguous()
keep = sorted(set(int(v) for v in np.linspace(0, 8, max(1, min(a.runs, 9))).round()))
train = [t for k, t in enumerate(training_list(S, host=True)) if k in keep]
mu1, mu2 = draw(a.batch)
max_rows = a.max_rows if a.max_rows is not None else (513 if a.solver == "device" else None)
fit = lambda proj, min_rows: pod.build_row_sampling(X, Phi, train, a.dt, proj, tau=a.tau, stride=a.stride, min_rows=min_rows,
                                                    max_rows=max_rows, solver=a.solver)
worst = lambda x, y: float(((x.flatten(1) - y.flatten(1)).norm(dim=1) / y.flatten(1).norm(dim=1)).max())
sig = lambda v: float(f"{v:.4g}")
C = max(1, min(a.check, a.batch))
for proj in (("Galerkin", "LSPG") if a.proj == "both" else (a.proj,)):
    p = rom.PROJ[proj.lower()]
    t0, filled = time.time(), True
    if a.all_rows:
        s = pod.RowSampling(np.arange(N, dtype=np.int32), np.ones(N), proj.lower(), 0.0, 0, 0.0)
    else:
        filled = a.min_rows is None or a.min_rows > 1
        try:
            s = fit(proj, a.min_rows)
        except ValueError as e:
            if "no column left to add" not in str(e) or not filled:
                raise
            print(f"# {proj}: {e}; fitting again without a fill", flush=True)
            s, filled = fit(proj, 1), False
    build_s = time.time() - t0
    print(f"# {proj}: {s.m} rows in {build_s:.0f} s ({'all rows' if a.all_rows else a.solver})", flush=True)
    plan = rom.HyperBlockedPodPlan(Phi, s, X, Phi.device)
    runs = {"hyper": lambda: rom.pod_prom_run_hyper_blocked(X, np.ones(N), mu1, mu2, a.dt, a.steps, None, plan, p)}
    if a.host:
        runs["host"] = lambda: rom._pod_prom_run_hyper_library(plan, np.ones(N), mu1, mu2, a.dt, a.steps, p, 0.0, 1e-6, 20)
        runs["full"] = lambda: rom._pod_prom_run_library(X, np.ones(N), mu1, mu2, a.dt, a.steps, Phi, p, 0.0, 1e-6, 20, Phi.device)
    if N <= 512:
        bplan = rom.BlockedPodPlan(Phi, Phi.device)
        runs["blocked"] = lambda: rom.pod_prom_run_blocked(X, np.ones(N), mu1, mu2, a.dt, a.steps, bplan, p)
    rates, last = time_alternately(runs, a.reps)
    hy = last["hyper"]
    ref = rom._pod_prom_run_library(X, np.ones(N), mu1[:C], mu2[:C], a.dt, a.steps, Phi, p, 0.0, 1e-6, 20, Phi.device)
    out = {"projection": proj, "N": N, "r": a.r, "batch": a.batch, "steps": a.steps, "dt": a.dt, "rows": s.m, "all_rows": a.all_rows,
           "training_runs": len(train), "stride": a.stride, "tau": a.tau, "solver": a.solver, "filled": filled,
           "sampling_seconds": sig(build_s), "training_residual": sig(s.residual), "path": hy.path, "redone": hy.redone,
           "newton_steps": int(hy.iters.sum().item()), "flagged_samples": int(hy.flags.ne(0).sum().item()),
           "info_nonzero": int(hy.info.ne(0).sum().item()), "hyper_rates": [sig(v) for v in rates["hyper"]],
           "checked_samples": C, "hyper_vs_full_prom": sig(worst(hy.hist[:C], ref.hist)),
           "iters_hyper_vs_full_prom": [int(hy.iters[:C].sum().item()), int(ref.iters.sum().item())]}
    for k in ("host", "full", "blocked"):
        if k in runs:
            out.update({f"{k}_rates": [sig(v) for v in rates[k]],
                        f"slowest_hyper_beats_fastest_{k}": bool(min(rates["hyper"]) > max(rates[k])),
                        f"hyper_over_{k}_medians": sig(np.median(rates["hyper"]) / np.median(rates[k])),
                        f"same_iters_as_{k}": bool(torch.equal(hy.iters, last[k].iters))})
    print(json.dumps(out), flush=True)
