#!/usr/bin/env python3
"""Time of the row-sampling fit on the host (pod.nnls_rows) and on the device (pod.nnls_rows_device, csrc/nnls.hip) on the
training matrix of pod.build_row_sampling, and the time to assemble that matrix (pod.row_sampling_system, host work).
The basis is built on the device (FOM runs of the 3 x 3 training grid, 200 steps, snapshot SVD truncated at --r); G comes
from the first --runs of the nine runs at every --stride-th step.  Prints one JSON line per projection: the shape of G, the
seconds to assemble it, of the host fit, of the upload of G and of the device fit with the upload included (wall clock
around a synchronised device; the device fit is run twice and the second run counts), whether the two row sets are equal
and how far the weights are apart, the counts of the device fit (adds, drops, dependent columns, solves, the smallest
|v| / |G[:, j]| appended), and the bytes the kernels read per outer step by the model of DESIGN K28 -- the gradient pass
over the columns that are not active, four passes over Q and one over the active columns for the residual, at the mean
number of active columns -- with the rate that model and the measured time per outer step imply.
usage: python tools/time_nnls_rows.py [--n 4096] [--r 96] [--dt 0.00625] [--projection both] [--runs 9] [--stride 10]
       [--tau 1e-4] [--min-rows M] [--no-host]"""
import argparse, json, time
import numpy as np, torch
from _timing import training_list, training_snapshots
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096); ap.add_argument("--r", type=int, default=96)
ap.add_argument("--dt", type=float, default=0.00625); ap.add_argument("--projection", default="both", choices=["both", "Galerkin", "LSPG"])
ap.add_argument("--runs", type=int, default=9); ap.add_argument("--stride", type=int, default=10)
ap.add_argument("--tau", type=float, default=1e-4); ap.add_argument("--min-rows", type=int, default=None)
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()
from burgers_hip import pod
N = a.n
X, S = training_snapshots(N, a.dt)
dev = S.device
Phi = pod.pod_basis(S, n_modes=a.r)[0].contiguous().cpu().numpy()
train = training_list(S, host=True)[:a.runs]
min_rows = min(3 * a.r, N) if a.min_rows is None else a.min_rows
max_rows = pod.hyper_rom_limits()[1] if a.r <= pod.hyper_rom_limits()[0] else pod.hyper_wide_rom_limits()[1]
sig = lambda v: float(f"{v:.4g}")


def clock(f):
    torch.cuda.synchronize(); t0 = time.perf_counter(); out = f(); torch.cuda.synchronize()
    return time.perf_counter() - t0, out


for proj in (("Galerkin", "LSPG") if a.projection == "both" else (a.projection,)):
    t_g, (G, pairs) = clock(lambda: pod.row_sampling_system(X, Phi, train, a.dt, proj.lower(), 0.0, True, a.stride))
    d = G.sum(axis=1)
    args = (d - G[:, 0], a.tau * float(np.linalg.norm(d)) / float(np.linalg.norm(d - G[:, 0])), max(min_rows - 1, 0), max_rows - 1)
    out = {"projection": proj, "N": N, "r": a.r, "runs": len(train), "stride": a.stride, "tau": a.tau, "G": list(G.shape),
           "G_MB": sig(G.nbytes / 1e6), "min_rows": min_rows, "max_rows": max_rows, "assemble_s": sig(t_g)}
    refused = None
    for rep in range(2):                                                        # the first run loads the code objects
        info = {}
        t_up, Gd = clock(lambda: torch.as_tensor(G[:, 1:]).to(dev))
        try:
            t_fit, (x, rel) = clock(lambda: pod.nnls_rows_device(Gd, *args, info=info))
        except ValueError as e:                                                 # e.g. min_rows beyond the numerical rank of G
            refused = str(e)
        del Gd
    if refused is not None:
        out.update({"device_refused": refused, **{k: (sig(v) if isinstance(v, float) else v) for k, v in info.items()}})
        if not a.no_host:
            t_host, (xh, relh) = clock(lambda: pod.nnls_rows(G[:, 1:], *args))
            out.update({"host_s": sig(t_host), "host_rows": int((xh > 0.0).sum()) + 1})
        print(json.dumps(out), flush=True)
        continue
    rows_dev = np.flatnonzero(x > 0.0)
    K = len(rows_dev)
    steps = info["adds"] + info["dependent"]
    model = 8.0 * G.shape[0] * ((G.shape[1] - 1 - K / 2.0) + 5.0 * K / 2.0)       # bytes per outer step at the mean K / 2 active columns
    out.update({"upload_s": sig(t_up), "device_s": sig(t_up + t_fit), "device_rows": K + 1, "device_residual": sig(rel),
                "outer_steps": steps, **{k: (sig(v) if isinstance(v, float) else v) for k, v in info.items()},
                "ms_per_outer_step": sig(1e3 * t_fit / max(steps, 1)), "model_MB_per_outer_step": sig(model / 1e6),
                "model_GB_per_s": sig(model * steps / t_fit / 1e9)})
    if not a.no_host:
        t_host, (xh, relh) = clock(lambda: pod.nnls_rows(G[:, 1:], *args))
        rows_host = np.flatnonzero(xh > 0.0)
        same = bool(np.array_equal(rows_host, rows_dev))
        out.update({"host_s": sig(t_host), "host_rows": len(rows_host) + 1, "rows_equal": same, "host_over_device": sig(t_host / (t_up + t_fit)),
                    "weights_apart": sig(float(np.abs(x - xh).max() / xh.max())) if same else None})
    print(json.dumps(out), flush=True)
