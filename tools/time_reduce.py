#!/usr/bin/env python3
"""Time bg_rom_reduce / bg_rom_reduce_lifted / bg_lu_solve_update alone (HIP events), B samples on an N-node mesh with r modes.

  python tools/time_reduce.py --n 512 --r 40 --b 4096 [--force16] [--persample] [--reps 5]

Prints one JSON line per (projection, mode): the microseconds per launch of each repetition (a repetition is 10 launches
between two events) and their median; then one line for the solve.  BG_LIB_PATH picks the library, so two builds are
compared from two processes."""
import argparse
import json
import os

import _timing
from _timing import np, torch

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--r", type=int, default=40)
ap.add_argument("--b", type=int, default=4096)
ap.add_argument("--force16", action="store_true", help="BG_OPT_MFMA_16X16: the 16x16x4 shape for every r")
ap.add_argument("--persample", action="store_true", help="also time a per-sample basis (B, N, r)")
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()

from burgers_hip import lib, rom

LAUNCHES = 10
N, r, B = a.n, a.r, a.b
opts = lib.BG_OPT_MFMA_16X16 if a.force16 else 0
rng = np.random.default_rng(0)
X = np.linspace(0, 100, N)
mu1, mu2 = rng.uniform(4.25, 5.5, B), rng.uniform(0.015, 0.03, B)
U = 1 + 4 * rng.random((B, N))
Phi = np.linalg.qr(rng.standard_normal((N, r)))[0]
c = rom._setup(X, U, mu1, mu2, 0.05, 0.0, None)
dev = c.device
Ud = torch.as_tensor(U, device=dev); G = torch.empty_like(Ud); rom._mass_rhs(c, Ud, G)
Phid = torch.as_tensor(Phi, device=dev)
W = torch.as_tensor(rng.standard_normal((B, N, r)), device=dev) if a.persample else None
f64 = dict(dtype=torch.float64, device=dev)
Ar, br, wtu = torch.zeros((B, r, r), **f64), torch.zeros((B, r), **f64), torch.zeros((B, r), **f64)
q = torch.as_tensor(U @ Phi, device=dev)
head = {"library": os.path.basename(os.environ.get("BG_LIB_PATH", "product")), "N": N, "r": r, "B": B, "force16": a.force16}

calls = {"U": lambda proj: rom.rom_reduce(c, Phid, Ud, G, proj, True, None, Ar, br, wtu, extra_opts=opts),
         "lifted": lambda proj: rom.rom_reduce_lifted(c, Phid, q, Ud, G, proj, True, None, Ar, br, wtu, extra_opts=opts)}
if a.persample:
    calls["persample"] = lambda proj: rom.rom_reduce(c, W, Ud, G, proj, True, None, Ar, br, None, extra_opts=opts)
for proj, name in ((0, "galerkin"), (1, "lspg")):
    for mode, call in calls.items():
        def run():
            for _ in range(LAUNCHES):
                call(proj)
        ms, _ = _timing.time_runs(run, a.reps)
        us = [t * 1e3 / LAUNCHES for t in ms]
        print(json.dumps({**head, "what": "reduce", "projection": name, "mode": mode, "us_per_launch": [round(v, 2) for v in us],
                          "median_us": round(float(np.median(us)), 2)}), flush=True)

st = rom._IterState(c, r)
ms = []
for rep in range(3 + a.reps):                    # three warm-ups; the reset of the iteration state stays outside the events
    st.active.fill_(1); st.k.zero_(); st.launched = 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); st.solve_update(1, Ar, br, wtu, q, 1e-6, 20); e1.record(); torch.cuda.synchronize()
    if rep >= 3:
        ms.append(e0.elapsed_time(e1))
print(json.dumps({**head, "what": "lu_solve_update", "us_per_launch": [round(t * 1e3, 2) for t in ms],
                  "median_us": round(float(np.median(ms)) * 1e3, 2)}))
