"""What the tests of the hyper-reduced POD-ANN loop (bg_hyper_ann_rom_run) share: the numpy restatement of the weighted-row
POD-ANN iteration, built from oracle.burgers_ref's own assembly, mlp_forward and mlp_jacobian; the cases; the committed
closure with its training runs.  With all rows and unit weights the restatement is oracle.burgers_ref.pod_ann_prom
(tests/test_ann_row_sampling.py holds it to that).  Closures and bases come from tests/ann_wide_cases.py (mlp, weights) and
loop_cases.training_snapshots.  numpy only at import."""
import functools

import numpy as np

import ann_wide_cases as aw
from conftest import load_golden, mesh
from hyper_ref import training_runs
from loop_cases import training_snapshots

ENTRY = "bg_hyper_ann_rom_run"
NT = 6
# name: N, dt, n, nbar, hidden widths, seed of the closure, scale, E, seed of the mesh (None: uniform)
CASES = {
    "full-256": (256, 0.05, 5, 91, (32, 64, 128, 256, 256), 505, 3.0, 0.0, None),
    "perturbed-96": (96, 0.05, 8, 40, (7,), 520, 3.0, 0.01, 7),
}
# the full-256 closure shape on the POD basis of a mesh beyond every other POD-ANN loop
LONG = (2049, 0.0125, 5, 91, (32, 64, 128, 256, 256), 505, 3.0, 0.0, None)


@functools.lru_cache(maxsize=None)
def case_data(case):
    """(X, U_p, U_s, model): ``case`` is a name of CASES or a tuple of that form."""
    N, dt, n, nbar, hidden, seed, scale, E, mseed = CASES[case] if isinstance(case, str) else case
    X, _, U = training_snapshots(N, dt, E, mseed)
    Up, Us = np.ascontiguousarray(U[:, :n]), np.ascontiguousarray(U[:, n:n + nbar])
    return X, Up, Us, aw.mlp([n, *hidden, nbar], "ELU", True, seed, scale)


def committed():
    """(X, U_p, U_s, model, Ws, bs, dt): the committed closure of tests/golden/ann_n5.npz (N = 512, n = 5, nbar = 91)."""
    import torch
    import torch.nn as nn
    g = load_golden("ann_n5.npz")
    Ws, bs = [g[f"W{i}"] for i in range(6)], [g[f"b{i}"] for i in range(6)]
    layers = []
    for i, (W, b) in enumerate(zip(Ws, bs)):
        lin = nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(W)); lin.bias.copy_(torch.from_numpy(b))
        layers += [lin] + ([nn.ELU()] if i < 5 else [])
    X, _ = mesh(512)
    return X, g["U_p"], g["U_s"], nn.Sequential(*layers).eval(), Ws, bs, float(g["At"])


@functools.lru_cache(maxsize=None)
def committed_sampling(proj):
    """build_ann_row_sampling on the committed closure: the nine training runs, every 10th step, tau = 1e-4, the defaults."""
    from burgers_hip import pod
    X, Up, Us, model, _, _, dt = committed()
    return pod.build_ann_row_sampling(X, Up, Us, model, training_runs(512, dt), dt, proj, tau=1e-4)


def decode(Up, Us, Q, Qs, u0):
    """(N, nT+1): U = U_p q + U_s q_s with u0 itself in column 0."""
    U = Up @ Q + Us @ Qs
    U[:, 0] = u0
    return U


def hyper_ann_prom(X, dt, nT, u0, mu1, E, mu2, U_p, U_s, Ws, bs, projection, rows, xi, tol=1e-6, max_it=50, backwards=False):
    """(Q (n, nT+1), Qs (nbar, nT+1), iters): pod_ann_prom (oracle/burgers_ref.py:423-460) with the two projections as sums
    over the mesh rows ``rows`` weighted by ``xi``, and without the re-projection at the start of a step: column 0 of Q is
    U_p^T u0, afterwards q_p carries over (q_p <- q_p + dq).  The state is the decode U_p q_p + U_s N(q_p) except in the first
    iteration of the run, which assembles at u0 itself and takes u^n = u0.  Qs holds the closure value of every step's
    decode (column 0: zeros, no closure value belongs to u0).  ``backwards``: sum the rows in descending order."""
    from oracle import burgers_ref as br
    assert projection in ("Galerkin", "LSPG")
    X = np.asarray(X, dtype=np.float64)
    rows, xi = np.asarray(rows, dtype=np.int64), np.asarray(xi, dtype=np.float64)
    if backwards:
        rows, xi = rows[::-1], xi[::-1]
    n, nbar = U_p.shape[1], U_s.shape[1]
    Q, Qs = np.zeros((n, nT + 1)), np.zeros((nbar, nT + 1))
    U0 = np.asarray(u0, dtype=np.float64)
    q_p = U_p.T @ U0
    Q[:, 0] = q_p
    M3, K3, F = br.mass_tridiag(X), br.diffusion_tridiag(X), br.forcing_vector(X, mu2)
    iters = np.zeros(nT, dtype=np.int32)
    for nt in range(nT):
        Mun = br.tridiag_matvec(*M3, U0)
        err, k, q_s = 1.0, 0, Qs[:, nt]
        while err > tol and k < max_it:
            C3 = br.convection_tridiag(X, U0)
            S = br.supg_term(X, U0, mu2)
            lo, di, up = br.system_tridiag(M3, K3, C3, dt, E)
            b = Mun + dt * F - dt * S
            b[0] = mu1
            R = br.tridiag_matvec(lo, di, up, U0) - b
            dN = br.mlp_jacobian(Ws, bs, q_p.astype(np.float32)).astype(np.float64)
            W = U_p + U_s @ dN
            Y = br.tridiag_matmat(lo, di, up, W)
            Wt = W if projection == "Galerkin" else Y
            Ar, br_ = np.zeros((n, n)), np.zeros(n)
            for i, w in zip(rows, xi):                      # one row at a time: the order of the sum is the order of ``rows``
                Ar += w * np.outer(Wt[i], Y[i])
                br_ += w * Wt[i] * R[i]
            dq = np.linalg.solve(Ar, -br_)
            q_p = q_p + dq
            q_s = br.mlp_forward(Ws, bs, q_p.astype(np.float32)).astype(np.float64)
            U0 = U_p @ q_p + U_s @ q_s
            err = np.linalg.norm(dq) / (np.linalg.norm(q_p) + 1e-14)
            k += 1
        iters[nt] = k
        Q[:, nt + 1], Qs[:, nt + 1] = q_p, q_s
    return Q, Qs, iters
