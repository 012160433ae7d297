"""What the tests of the hyper-reduced quadratic-manifold loop (bg_hyper_quad_rom_run) share: the numpy restatement of the
weighted-row, carried-q iteration, built from oracle.burgers_ref's own assembly, get_sym and get_dQ_dq, with its decode; the
cases; the manifolds (oracle.burgers_ref.compute_H on loop_cases.training_snapshots, alpha = 1e-2) and the builder's
samplings.  With all rows and unit weights the restatement is oracle.burgers_ref.pod_quadratic_manifold
(tests/test_quad_row_sampling.py holds it to that).  numpy only at import."""
import functools

import numpy as np

from hyper_ref import training_runs
from loop_cases import training_snapshots

ENTRY = "bg_hyper_quad_rom_run"
NT = 6
ALPHA = 1e-2
CAP = 25
# name: N, dt, n, E, seed of the mesh (None: uniform)
CASES = {
    "full-256": (256, 0.05, 40, 0.0, None),           # the row limit: four full slabs of table nodes
    "perturbed-96": (96, 0.05, 17, 0.01, 21),         # a partial slab, n not a multiple of 4, a non-uniform mesh
}
LONG = (2049, 0.0125, 40, 0.0, None)                  # a mesh beyond every other quadratic-manifold loop
MID = (1024, 0.0125, 40, 0.0, None)


def _case(case):
    return CASES[case] if isinstance(case, str) else case


@functools.lru_cache(maxsize=None)
def case_data(case):
    """(X, Phi, H): ``case`` is a name of CASES or a tuple of that form.  One copy per process: leave it as it is."""
    from oracle import burgers_ref as br
    N, dt, n, E, mseed = _case(case)
    X, S, U = training_snapshots(N, dt, E, mseed)
    Phi = np.ascontiguousarray(U[:, :n])
    q = Phi.T @ S
    return X, Phi, np.ascontiguousarray(br.compute_H(br.build_Q(q), S - Phi @ q, ALPHA))


@functools.lru_cache(maxsize=None)
def builder_sampling(case, proj, min_rows=None):
    """pod.build_quad_row_sampling on the case's manifold: the nine training runs, every 10th step, the defaults (tau = 1e-5)."""
    from burgers_hip import pod
    N, dt, _, E, mseed = _case(case)
    X, Phi, H = case_data(case)
    return pod.build_quad_row_sampling(X, Phi, H, training_runs(N, dt, E, mseed), dt, proj, E=E, min_rows=min_rows)


def decode(Phi, H, Q, u0):
    """(N, nT+1): U = Phi q + H sym(q) with u0 itself in column 0."""
    I, J = np.triu_indices(Q.shape[0])
    U = Phi @ Q + H @ (Q[I] * Q[J])
    U[:, 0] = u0
    return U


def hyper_quad_prom(X, dt, nT, u0, uxa, E, mu2, Phi, H, projection, rows, xi, tol=1e-6, max_it=CAP, backwards=False):
    """(Q (n, nT+1), iters): pod_quadratic_manifold (oracle/burgers_ref.py:347-382) with the two projections as sums over the
    mesh rows ``rows`` weighted by ``xi``, and without the re-projection at the start of a step: column 0 of Q is Phi^T u0,
    afterwards q carries over (q <- q + dq).  Every pass assembles at the decode Phi q + H sym(q); the mass row of the first
    step takes u^n = u0 itself, later steps the decode.  ``backwards``: sum the rows in descending order."""
    from oracle import burgers_ref as br
    assert projection in ("Galerkin", "LSPG")
    X = np.asarray(X, dtype=np.float64)
    rows, xi = np.asarray(rows, dtype=np.int64), np.asarray(xi, dtype=np.float64)
    if backwards:
        rows, xi = rows[::-1], xi[::-1]
    n = Phi.shape[1]
    Q = np.zeros((n, nT + 1))
    Un = np.asarray(u0, dtype=np.float64)
    q = Phi.T @ Un
    Q[:, 0] = q
    M3, K3, F = br.mass_tridiag(X), br.diffusion_tridiag(X), br.forcing_vector(X, mu2)
    iters = np.zeros(nT, dtype=np.int32)
    for m in range(nT):
        u = Phi @ q + H @ br.get_sym(q)
        Mun = br.tridiag_matvec(*M3, Un)
        k = 0
        for _ in range(max_it):
            C3 = br.convection_tridiag(X, u)
            lo, di, up = br.system_tridiag(M3, K3, C3, dt, E)
            b = Mun + dt * F
            b[0] = uxa
            R = br.tridiag_matvec(lo, di, up, u) - b
            T = Phi + H @ br.get_dQ_dq(q)
            Y = br.tridiag_matmat(lo, di, up, T)
            Wt = T if projection == "Galerkin" else Y
            Ar, br_ = np.zeros((n, n)), np.zeros(n)
            for i, w in zip(rows, xi):                      # one row at a time: the order of the sum is the order of ``rows``
                Ar += w * np.outer(Wt[i], Y[i])
                br_ += w * Wt[i] * R[i]
            dq = np.linalg.solve(Ar, -br_)
            q = q + dq
            u = Phi @ q + H @ br.get_sym(q)
            k += 1
            if np.linalg.norm(dq) / max(1e-14, np.linalg.norm(q)) < tol:
                break
        iters[m] = k
        Q[:, m + 1] = q
        Un = u
    return Q, iters
