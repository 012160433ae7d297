"""What the tests of the hyper-reduced local POD loop share: the numpy restatement of bg_hyper_local_rom_run's semantics,
built from oracle.burgers_ref's own assembly functions, and the dense clustering with NON-NESTED orthonormal bases.  With all
rows and unit weights the restatement is oracle.burgers_ref.local_prom_burgers (tests/test_local_row_sampling.py holds it to
that)."""
import functools

import numpy as np

from loop_cases import DENSE_WIDTHS, training_snapshots

MG = 12
NT = 40
MUS = [(4.6, 0.02), (5.3, 0.028)]


@functools.lru_cache(maxsize=None)
def dense_clustering(N, dt, E=0.0, seed=None):
    """(X, centres (11, 12), bases {c: (N, DENSE_WIDTHS[c])}, U_g (N, 40)): U_g the 40 leading left singular vectors of
    loop_cases.training_snapshots; the centres U_g[:, :12]^T u at steps 0, 4, ..., 40 of the oracle's LSPG r = 40 POD run at
    mu = (4.9, 0.022); the members of cluster c the snapshots whose squared distance to centre c is at most 1.5^2 times their
    smallest; basis c the leading DENSE_WIDTHS[c] left singular vectors of the members.  One copy per process: callers leave
    it as it is."""
    from oracle import burgers_ref as br
    X, S, U = training_snapshots(N, dt, E, seed)
    Ug = np.ascontiguousarray(U[:, :40])
    traj = br.pod_prom_burgers(X, dt, 40, np.ones(N), 4.9, E, 0.022, Ug, "LSPG")
    centres = (Ug[:, :MG].T @ traj[:, ::4]).T.copy()
    assert centres.shape == (11, MG)
    Q = Ug[:, :MG].T @ S
    d2 = ((Q[None, :, :] - centres[:, :, None]) ** 2).sum(1)                     # (C, snapshots)
    bases = {}
    for c, w in enumerate(DENSE_WIDTHS):
        members = S[:, d2[c] <= 1.5 ** 2 * d2.min(0)]
        assert members.shape[1] >= w, (c, members.shape)
        bases[c] = np.ascontiguousarray(np.linalg.svd(members, full_matrices=False)[0][:, :w])
    return X, centres, bases, Ug


def all_rows(N, proj):
    from burgers_hip import pod
    return pod.RowSampling(np.arange(N, dtype=np.int32), np.ones(N), proj.lower(), 0.0, 0, 0.0)


def hyper_local_prom(X, dt, nT, u0, mu1, E, mu2, centres, bases, Ug, mg, projection, rows, xi, tol=1e-6, max_it=20,
                     backwards=False):
    """(U (N, nT+1), Q (rmax, nT+1), iters, clusters, margin): local_prom_burgers (oracle/burgers_ref.py:674-716) with the
    two projections as sums over the mesh rows ``rows`` weighted by ``xi``, on the state (p, q) = the cluster held and the
    coordinates in its basis.  Step 0 picks from U_g^T u0, starts from Phi_c^T u0 and assembles at u0 itself.  Step n >= 1
    picks from (U_g^T Phi_p) q; at a switch the first iteration assembles at u^n = Phi_p q (the old basis) and the base of the
    update is (Phi_c^T Phi_p) q; otherwise the state is Phi_c q and the update q + dq.  Column n + 1 of Q holds the
    coordinates in the basis of clusters[n], column 0 Phi_{c0}^T u0; U is the decoded history with u0 in column 0.
    ``margin``: the smallest relative gap between the best and the second-best squared centre distance over the picks.
    ``backwards``: sum the rows in descending order."""
    from oracle import burgers_ref as br
    assert projection in ("Galerkin", "LSPG")
    X = np.asarray(X, dtype=np.float64)
    rows, xi = np.asarray(rows, dtype=np.int64), np.asarray(xi, dtype=np.float64)
    if backwards:
        rows, xi = rows[::-1], xi[::-1]
    N, rmax = len(X), max(b.shape[1] for b in bases.values())
    Ugm = Ug[:, :mg]
    U, Q = np.zeros((N, nT + 1)), np.zeros((rmax, nT + 1))
    U[:, 0] = u0
    M3, K3, F = br.mass_tridiag(X), br.diffusion_tridiag(X), br.forcing_vector(X, mu2)
    iters, clusters = np.zeros(nT, dtype=np.int32), np.zeros(nT, dtype=np.int32)
    margin = np.inf
    p, q = -1, None
    for n in range(nT):
        qg = Ugm.T @ np.asarray(u0, dtype=np.float64) if n == 0 else (Ugm.T @ bases[p]) @ q
        d2 = ((centres - qg[None, :]) ** 2).sum(1)
        c = int(np.argmin(d2))
        two = np.sort(d2)[:2]
        margin = min(margin, (two[1] - two[0]) / max(two[1], 1e-300))
        Phi = bases[c]
        if n == 0:
            U0 = np.asarray(u0, dtype=np.float64)
            q = Phi.T @ U0
            Q[:len(q), 0] = q
        else:
            U0 = bases[p] @ q                                     # u^n: in the OLD basis when the cluster changes
            if c != p:
                q = (Phi.T @ bases[p]) @ q
        p = c
        clusters[n] = c
        r = Phi.shape[1]
        err, k = 1.0, 0
        Mun = br.tridiag_matvec(*M3, U0)
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
            for i, w in zip(rows, xi):                            # one row at a time: the order of the sum is the order of ``rows``
                Ar += w * np.outer(W[i], Y[i])
                br_ += w * W[i] * R[i]
            dq = np.linalg.solve(Ar, -br_)
            q = q + dq
            U0 = Phi @ q
            err = np.linalg.norm(dq) / np.linalg.norm(q)
            k += 1
        iters[n] = k
        Q[:r, n + 1] = q
        U[:, n + 1] = U0
    return U, Q, iters, clusters, float(margin)
