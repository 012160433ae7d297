#!/usr/bin/env python3
"""A/B of two library builds on bench.py's flagship FOM workload (B = 1024, N = 1024, 500 steps, dt = 0.025, the bench's seed):
one process per build (BG_LIB_PATH picks the library), results compared through a file.

  BG_LIB_PATH=1d-burgers-equation-roms_amd/build/libvar_noexit.so python tools/fom_ab.py --save /tmp/fom_a.npz
  python tools/fom_ab.py --against /tmp/fom_a.npz

The second call prints one JSON line: whether iteration counts and flags are identical, and the largest |hist_b - hist_a|
relative to max |hist_a|.  The saved file holds the full history (4.2 GB uncompressed); --against deletes it unless --keep."""
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
a = ap.parse_args()

import torch
from burgers_hip import fom, lib

rng = np.random.default_rng(20251121)
N, B, nsteps, dt = 1024, 1024, 500, 0.025
mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
res = fom.fom_run(np.linspace(0.0, 100.0, N), np.ones(N), mu1, mu2, dt, nsteps)
torch.cuda.synchronize()
hist, iters, flags = lib.to_host(res.hist), res.iters.cpu().numpy(), res.flags.cpu().numpy()
name = os.path.basename(os.environ.get("BG_LIB_PATH", "product"))
if a.save:
    np.savez(a.save, hist=hist, iters=iters, flags=flags)
    print(json.dumps({"library": name, "saved": a.save, "iterations": int(iters.sum())}))
if a.against:
    with np.load(a.against) as g:
        ha, ia, fa = g["hist"], g["iters"], g["flags"]
    d = 0.0
    for b0 in range(0, B, 64):                               # blockwise: no third 4 GB array
        d = max(d, float(np.abs(hist[b0:b0 + 64] - ha[b0:b0 + 64]).max()))
    print(json.dumps({"library": name, "against": a.against, "iterations": int(iters.sum()),
                      "iters_identical": bool(np.array_equal(iters, ia)), "flags_identical": bool(np.array_equal(flags, fa)),
                      "max_abs_dhist": d, "max_abs_hist": float(np.abs(ha).max()),
                      "max_abs_dhist_over_max_abs_hist": d / float(np.abs(ha).max()),
                      "bitwise_identical": bool(d == 0.0)}))
    if not a.keep:
        os.remove(a.against)
