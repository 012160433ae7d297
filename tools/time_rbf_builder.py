#!/usr/bin/env python3
"""Time and accuracy of the POD-RBF closure fit (pod.fit_rbf_weights) on a FOM sweep built on the device: the 3 x 3 training
grid at N = 512 over 500 steps (4509 snapshots), n = 17, nbar = 79 -- the shape of the golden fixture -- at 300, 1024 and
4509 centres.  Stages: the kernel matrix (bg_rbf_gram), the factorisation (bg_chol_factor), the solve (bg_chol_solve), the
whole fit; beside them the two library routes on the same matrix, solver="library" (LU) and torch.linalg.cholesky_ex +
cholesky_solve.  For every solver: the backward error of the ridge system and the relative difference of its closure from
the snapshots' own secondary coordinates on the snapshots that are no centres (none at 4509).  One JSON line per size;
milliseconds are medians of --reps after a warm-up, between HIP events.  The rate is (Ns^3/3 + 2 Ns^2 nbar) flop over
factorisation + solve.  BG_LIB_PATH selects a variant build (tools/build_variant.sh ... -DBG_CHOL_TILE_VALU).
usage: python tools/time_rbf_builder.py [--sizes 300 1024 4509] [--kernel gaussian] [--eps 2.0] [--ridge 1e-8] [--reps 3]"""
import argparse, json
from _timing import training_snapshots
import numpy as np, torch
ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[300, 1024, 4509]); ap.add_argument("--kernel", default="gaussian")
ap.add_argument("--eps", type=float, default=2.0); ap.add_argument("--ridge", type=float, default=1e-8)
ap.add_argument("--n", type=int, default=17); ap.add_argument("--nbar", type=int, default=79)
ap.add_argument("--reps", type=int, default=3); ap.add_argument("--no-library", action="store_true")
a = ap.parse_args()
from burgers_hip import lib, pod, rom
L = lib.load()
X, S = training_snapshots(512, 0.05, steps=500)                                 # (512, 4509)
dev = S.device
U = pod.thin_svd(S)[0]
U_p, U_s = U[:, :a.n].contiguous(), U[:, a.n:a.n + a.nbar].contiguous()
Q, Qb = (U_p.t() @ S).t().contiguous(), (U_s.t() @ S).t().contiguous()
x_min, x_max, y_min, y_max = Q.min(0).values, Q.max(0).values, Qb.min(0).values, Qb.max(0).values
host = lambda t: t.cpu().numpy()


def timed(run, reps, setup=None):
    """Median milliseconds of ``run`` between HIP events, ``setup`` before each call outside the events; the last result."""
    ms = []
    for rep in range(reps + 1):                                                 # the first is the warm-up
        if setup:
            setup()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); res = run(); e1.record(); torch.cuda.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1))
    return float(f"{np.median(ms):.4g}"), res


def attempt(run, reps, setup=None):
    try:
        return timed(run, reps, setup)
    except Exception as e:                                                      # a library route that cannot allocate its workspace
        return None, f"{type(e).__name__}: {e}"[:160]


for Ns in a.sizes:
    idx = np.linspace(0, S.shape[1] - 1, Ns).astype(int)
    rows = torch.as_tensor(idx, device=dev)
    Xs = (2.0 * ((Q[rows] - x_min) / (x_max - x_min)) - 1.0).contiguous()
    Ys = (2.0 * ((Qb[rows] - y_min) / (y_max - y_min)) - 1.0).contiguous()
    rest = torch.as_tensor(np.setdiff1d(np.arange(S.shape[1]), idx), device=dev)
    ms_gram, A = timed(lambda: pod.rbf_kernel_matrix(Xs, a.eps, a.kernel, a.ridge), a.reps)
    Lm, B = torch.empty_like(A), torch.empty_like(Ys)
    flag = torch.zeros((1,), dtype=torch.int32, device=dev)
    factor = lambda: lib.check(L.bg_chol_factor(Ns, lib.ptr(Lm), Ns, lib.ptr(flag), lib.stream_ptr(dev)), "bg_chol_factor")
    solve = lambda: lib.check(L.bg_chol_solve(Ns, a.nbar, lib.ptr(Lm), Ns, lib.ptr(B), a.nbar, lib.stream_ptr(dev)), "bg_chol_solve")
    ms_factor, _ = timed(factor, a.reps, setup=lambda: Lm.copy_(A))
    ms_solve, _ = timed(solve, a.reps, setup=lambda: B.copy_(Ys))
    W = {"cholesky": B.clone()}
    ms_fit, _ = timed(lambda: pod.fit_rbf_weights(Xs, Ys, a.eps, a.kernel, a.ridge), a.reps)
    ms_lu = ms_tc = None
    if not a.no_library:
        ms_lu, W["library_lu"] = attempt(lambda: torch.linalg.solve(A, Ys), a.reps)

        def torch_cholesky():
            Lt, bad = torch.linalg.cholesky_ex(A)
            return torch.cholesky_solve(Ys, Lt)
        ms_tc, W["library_cholesky"] = attempt(torch_cholesky, a.reps)
    out = {"Ns": Ns, "n": a.n, "nbar": a.nbar, "kernel": a.kernel, "ridge": a.ridge, "info": int(flag.item()),
           "gram_ms": ms_gram, "factor_ms": ms_factor, "solve_ms": ms_solve, "fit_ms": ms_fit, "library_lu_ms": ms_lu,
           "library_cholesky_ms": ms_tc}
    flop = Ns ** 3 / 3.0 + 2.0 * Ns ** 2 * a.nbar
    out["tflops_factor_and_solve"] = float(f"{flop / ((ms_factor + ms_solve) * 1e-3) / 1e12:.4g}")
    for name, w in W.items():
        if not isinstance(w, torch.Tensor):
            out[name + "_error"] = w
            continue
        out[name + "_backward_error"] = float(f"{pod.backward_error(A, w, Ys):.3e}")
        if name != "cholesky":
            out[name + "_vs_cholesky"] = float(f"{float(torch.linalg.matrix_norm(w - W['cholesky']) / torch.linalg.matrix_norm(W['cholesky'])):.3e}")
        if len(rest):
            closure = rom.RbfClosure(host(Xs), host(w), a.eps, a.kernel, host(x_min), host(x_max), host(y_min), host(y_max), dev)
            val = closure.value(Q[rest].contiguous())
            out[name + "_held_out"] = float(f"{float(torch.linalg.matrix_norm(val - Qb[rest]) / torch.linalg.matrix_norm(Qb[rest])):.6e}")
            if name == "cholesky":
                val_chol = val.clone()                                          # (value() returns a view of the closure's buffer)
            else:
                out[name + "_held_out_vs_cholesky"] = float(f"{float(torch.linalg.matrix_norm(val - val_chol) / torch.linalg.matrix_norm(val_chol)):.3e}")
    print(json.dumps(out), flush=True)
