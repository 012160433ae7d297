"""What the hyper-reduction tests share: the numpy restatement of the weighted-row POD-PROM iteration (bg_hyper_rom_run's
semantics), built from oracle.burgers_ref's own assembly functions, and the training runs of the 3 x 3 grid.  With all rows and
unit weights the restatement is oracle.burgers_ref.pod_prom_burgers (tests/test_row_sampling.py holds it to that)."""
import numpy as np

from loop_cases import training_snapshots

TRAIN_MU1 = np.repeat([4.25, 4.875, 5.5], 3)
TRAIN_MU2 = np.tile([0.015, 0.0225, 0.03], 3)


def training_runs(N, dt, E=0.0, seed=None, keep=None):
    """The ``runs`` of build_row_sampling from loop_cases.training_snapshots: (hist (N, 201), mu1, mu2) per training point
    (``keep``: indices of the points to use, default all nine)."""
    _, S, _ = training_snapshots(N, dt, E, seed)
    nT1 = S.shape[1] // 9
    return [(S[:, k * nT1:(k + 1) * nT1], TRAIN_MU1[k], TRAIN_MU2[k]) for k in (range(9) if keep is None else keep)]


def hyper_prom(X, dt, nT, u0, mu1, E, mu2, Phi, projection, rows, xi, tol=1e-6, max_it=20, backwards=False):
    """(Q (r, nT+1), iters): pod_prom_burgers (oracle/burgers_ref.py:285-320) with the two projections as sums over the mesh
    rows ``rows`` weighted by ``xi``.  Column 0 of Q is Phi^T u0; the update is q + dq; the state is Phi q except in the first
    iteration of the run, which assembles at u0 itself and takes u^n = u0.  ``backwards``: sum the rows in descending order."""
    from oracle import burgers_ref as br
    assert projection in ("Galerkin", "LSPG")
    X = np.asarray(X, dtype=np.float64)
    rows, xi = np.asarray(rows, dtype=np.int64), np.asarray(xi, dtype=np.float64)
    if backwards:
        rows, xi = rows[::-1], xi[::-1]
    r = Phi.shape[1]
    Q = np.zeros((r, nT + 1))
    q = Phi.T @ u0
    Q[:, 0] = q
    M3, K3, F = br.mass_tridiag(X), br.diffusion_tridiag(X), br.forcing_vector(X, mu2)
    iters = np.zeros(nT, dtype=np.int32)
    U0 = np.asarray(u0, dtype=np.float64)
    for n in range(nT):
        Un = U0
        err, k = 1.0, 0
        Mun = br.tridiag_matvec(*M3, Un)
        while err > tol and k < max_it:
            C3 = br.convection_tridiag(X, U0)
            S = br.supg_term(X, U0, mu2)
            lo, di, up = br.system_tridiag(M3, K3, C3, dt, E)
            b = Mun + dt * F - dt * S
            b[0] = mu1
            R = br.tridiag_matvec(lo, di, up, U0) - b
            Y = br.tridiag_matmat(lo, di, up, Phi)
            W = Phi if projection == "Galerkin" else Y
            Ar, br_ = np.zeros((r, r)), np.zeros(r)
            for i, w in zip(rows, xi):                      # one row at a time: the order of the sum is the order of ``rows``
                Ar += w * np.outer(W[i], Y[i])
                br_ += w * W[i] * R[i]
            dq = np.linalg.solve(Ar, -br_)
            q = q + dq
            U0 = Phi @ q
            err = np.linalg.norm(dq) / np.linalg.norm(q)
            k += 1
        iters[n] = k
        Q[:, n + 1] = q
    return Q, iters
