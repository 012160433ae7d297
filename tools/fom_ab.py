#!/usr/bin/env python3
"""A/B of two library builds on one FOM workload: one process per build (BG_LIB_PATH picks the library), results compared
through a file.  The default workload is bench.py's flagship (B = 1024, N = 1024, 500 steps, dt = 0.025, the bench's seed):

  BG_LIB_PATH=1d-burgers-equation-roms_amd/build/libvar_noexit.so python tools/fom_ab.py --save /tmp/fom_a.npz
  python tools/fom_ab.py --against /tmp/fom_a.npz

--n, --b, --nsteps choose another shape (N > 1536 reaches the workgroup-per-sample kernels), --graded a non-uniform mesh,
--fd the finite-difference Newton stepper instead of the FEM one; give both calls the same options.

The second call prints one JSON line: whether iteration counts and flags are identical, and the largest |hist_b - hist_a|
relative to max |hist_a|.  The saved file holds the full history (4.2 GB uncompressed at the default shape); --against deletes
it unless --keep."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "1d-burgers-equation-roms_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--save")
ap.add_argument("--against")
ap.add_argument("--keep", action="store_true")
ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--b", type=int, default=1024)
ap.add_argument("--nsteps", type=int, default=500)
ap.add_argument("--graded", action="store_true")
ap.add_argument("--fd", action="store_true")
a = ap.parse_args()
if a.fd and a.graded:
    ap.error("--fd runs on a uniform mesh only")

import torch
from burgers_hip import fom, lib

rng = np.random.default_rng(20251121)
N, B, nsteps, dt = a.n, a.b, a.nsteps, 0.025 * min(1.0, 1024 / a.n)     # the flagship's dt / h beyond its N
mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
if a.fd:
    res = fom.fd_run(0.0, 100.0, N, np.ones(N), mu1, mu2, dt, nsteps)
else:
    X = np.linspace(0.0, 100.0, N)
    if a.graded:
        w = rng.uniform(0.7, 1.3, N - 1)
        X = np.concatenate([[0.0], np.cumsum(w)]) * (100.0 / w.sum())
    res = fom.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps)
torch.cuda.synchronize()
hist, iters, flags = lib.to_host(res.hist), res.iters.cpu().numpy(), res.flags.cpu().numpy()
name = os.path.basename(os.environ.get("BG_LIB_PATH", "product"))
shape = {"N": N, "B": B, "nsteps": nsteps, "graded": a.graded, "fd": a.fd}
if a.save:
    np.savez(a.save, hist=hist, iters=iters, flags=flags)
    print(json.dumps({"library": name, **shape, "saved": a.save, "iterations": int(iters.sum())}))
if a.against:
    with np.load(a.against) as g:
        ha, ia, fa = g["hist"], g["iters"], g["flags"]
    if ha.shape != hist.shape:
        sys.exit(f"{a.against} holds a history of shape {ha.shape}, this run one of {hist.shape}: not the same options")
    d, same = 0.0, True
    for b0 in range(0, B, 64):                               # blockwise: no third 4 GB array
        d = max(d, float(np.abs(hist[b0:b0 + 64] - ha[b0:b0 + 64]).max()))
        same = same and np.array_equal(hist[b0:b0 + 64].view(np.int64), ha[b0:b0 + 64].view(np.int64))   # NaN-proof
    print(json.dumps({"library": name, **shape, "against": a.against, "iterations": int(iters.sum()),
                      "iters_identical": bool(np.array_equal(iters, ia)), "flags_identical": bool(np.array_equal(flags, fa)),
                      "max_abs_dhist": d, "max_abs_hist": float(np.abs(ha).max()),
                      "max_abs_dhist_over_max_abs_hist": d / float(np.abs(ha).max()),
                      "bitwise_identical": bool(same)}))
    if not a.keep:
        os.remove(a.against)
