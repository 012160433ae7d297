"""What the tests of the hyper-reduced POD-RBF loop (bg_hyper_rbf_rom_run) share: the numpy restatement of the weighted-row
POD-RBF iteration, built from oracle.burgers_ref's own assembly, rbf_value and rbf_jacobian; the cases; the committed closure
with its sampling.  With all rows and unit weights the restatement is oracle.burgers_ref.pod_rbf_prom
(tests/test_rbf_row_sampling.py holds it to that).  Closures and bases come from tests/rbf_long_cases.py (the fixture closure
carried to an N-node mesh) and loop_cases.training_snapshots (a closure fitted to the 2049-node mesh).  numpy only at import."""
import functools

import numpy as np

import rbf_long_cases as lc
from conftest import mesh
from hyper_ref import training_runs
from loop_cases import training_snapshots

ENTRY = "bg_hyper_rbf_rom_run"
TOL = lc.TOL
# name: N, dt, E, seed of the mesh (None: uniform); bases rbf_long_cases.long_bases(N), closure rbf_long_cases.closure(N, kernel)
CASES = {
    "full-256": (256, 0.05, 0.0, None),
    "perturbed-96": (96, 0.05, 0.01, 7),
}
LONG_N, LONG_DT, LONG_KERNEL = 2049, 0.0125, "imq"


def case_data(case, kernel):
    """(X, dt, E, the nine closure arguments) of a case of CASES."""
    N, dt, E, seed = CASES[case]
    return lc.long_mesh(N, seed), dt, E, lc.closure(N, kernel)


@functools.lru_cache(maxsize=None)
def long_data():
    """(X, dt, E, the nine closure arguments) of LONG: N = 2049, a closure fitted to that mesh in numpy.  U_p, U_s: singular
    vectors 0 .. 16 and 17 .. 95 of the training snapshots; the centres are every 6th snapshot (302) in reduced coordinates,
    scaled to [-1, 1] with the data's min / max; imq kernel, eps = 1; W = solve(K + 1e-8 I, Ys).  (The fixture closure
    interpolated to 2049 nodes hits the iteration cap in every step.)"""
    X, S, U = training_snapshots(LONG_N, LONG_DT, 0.0, None)
    Up, Us = np.ascontiguousarray(U[:, :17]), np.ascontiguousarray(U[:, 17:96])
    Sc = S[:, ::6]
    Qp, Qs = (Up.T @ Sc).T, (Us.T @ Sc).T
    x_min, x_max, y_min, y_max = Qp.min(0), Qp.max(0), Qs.min(0), Qs.max(0)
    scale = lambda A, lo, hi: 2.0 * ((A - lo) / np.where(hi - lo < 1e-15, 1.0, hi - lo)) - 1.0
    Xt, Ys = scale(Qp, x_min, x_max), scale(Qs, y_min, y_max)
    eps = 1.0
    r2 = ((Xt[:, None, :] - Xt[None]) ** 2).sum(-1)
    K = 1.0 / np.sqrt(1.0 + eps ** 2 * r2)
    W = np.linalg.solve(K + 1e-8 * np.eye(len(K)), Ys)
    for A in (Up, Us, Xt, W):
        A.setflags(write=False)
    return X, LONG_DT, 0.0, (Up, Us, Xt, W, eps, x_min, x_max, y_min, y_max)


def committed(kernel):
    """(X, dt, the nine closure arguments): the committed closure of tests/golden/rbf_n17.npz on mesh(512)."""
    g = lc.golden()
    X, _ = mesh(512)
    return X, float(g["At"]), (g["U_p"], g["U_s"], g["X_train"], g["W_" + kernel], float(g["eps_" + kernel]), g["x_min"],
                                g["x_max"], g["y_min"], g["y_max"])


@functools.lru_cache(maxsize=None)
def committed_sampling(kernel, proj):
    """build_rbf_row_sampling on the committed closure: the nine training runs, every 10th step, tau = 1e-4, the defaults."""
    from burgers_hip import pod
    X, dt, cl = committed(kernel)
    return pod.build_rbf_row_sampling(X, *cl, training_runs(512, dt), dt, proj, kernel=kernel, tau=1e-4)


def sampling(rows, xi, proj):
    from burgers_hip import pod
    return pod.RowSampling(np.asarray(rows, dtype=np.int32), np.asarray(xi, dtype=np.float64), proj.lower(), 0.0, 0, 0.0)


@functools.lru_cache(maxsize=None)
def long_sampling(kind, proj):
    """"built": build_rbf_row_sampling's rows (training runs 0, 4, 8, every 10th step, the default min_rows) plus rows added
    by hand with weight 0.05, so that 0, 1, N - 2, N - 1, an adjacent pair (700, 701) and an isolated row (1500) are present.
    "limits": rows 0, 8, ..., 2040 with weight 8 (row 0: 1): m = 256 and 767 table nodes, both limits at once."""
    from burgers_hip import pod
    N = LONG_N
    if kind == "limits":
        rows = np.arange(0, N - 1, 8)
        xi = np.full(len(rows), 8.0); xi[0] = 1.0
        assert len(rows) == 256
        return sampling(rows, xi, proj)
    X, dt, _, cl = long_data()
    s = pod.build_rbf_row_sampling(X, *cl, training_runs(N, dt, keep=[0, 4, 8]), dt, proj, kernel=LONG_KERNEL, stride=10)
    w = dict(zip(s.rows.tolist(), s.xi.tolist()))
    for extra in (0, 1, N - 2, N - 1, 700, 701, 1500):
        w.setdefault(extra, 0.05)
    rows = np.array(sorted(w), dtype=np.int32)
    assert len(rows) <= pod.hyper_rbf_rom_limits()[3]
    return sampling(rows, [w[int(i)] for i in rows], proj)


# ---- the runs in which tests/test_rom_hyper_rbf_gpu.py demands the restatement's iteration counts of the kernel ------------
NT_ALL, NT_LONG, NT_LEFT = 4, 6, 6
ALL_ROWS = (("full-256", "gaussian"), ("perturbed-96", "imq"))          # three samples draw(3), both projections
LEFT_OUT = (10, 50, 51, 70)                                             # rows of perturbed-96 left out, unit weights elsewhere
# projection: kernel and two samples of draw(10) at which the restatement converges in every step (at most 17 / 16 iterations)
LEFT_OUT_RUNS = {"Galerkin": ("gaussian", (6, 7)), "LSPG": ("imq", (4, 5))}


def left_out_rows():
    return np.setdiff1d(np.arange(CASES["perturbed-96"][0]), LEFT_OUT)


def restatement_cases():
    """(name, X, dt, E, closure, proj, kernel, rows, xi, (mu1, mu2), steps) of every such run."""
    from loop_cases import draw
    for proj in ("Galerkin", "LSPG"):
        for case, kernel in ALL_ROWS:
            X, dt, E, cl = case_data(case, kernel)
            yield case, X, dt, E, cl, proj, kernel, np.arange(len(X)), np.ones(len(X)), draw(3), NT_ALL
        X, dt, E, cl = long_data()
        for kind in ("built", "limits"):
            s = long_sampling(kind, proj)
            yield "long-" + kind, X, dt, E, cl, proj, LONG_KERNEL, s.rows.numpy(), s.xi.numpy(), draw(2, seed=11), NT_LONG
        kernel, pick = LEFT_OUT_RUNS[proj]
        X, dt, E, cl = case_data("perturbed-96", kernel)
        rows = left_out_rows()
        yield "left-out", X, dt, E, cl, proj, kernel, rows, np.ones(len(rows)), tuple(v[list(pick)] for v in draw(10)), NT_LEFT


def decode(Up, Us, Q, Qs, u0):
    """(N, nT+1): U = U_p q + U_s q_s with u0 itself in column 0."""
    U = Up @ Q + Us @ Qs
    U[:, 0] = u0
    return U


def perturbed(cl, seed=20251121):
    """The closure with U_p, U_s and W multiplied entrywise by 1 + 4e-16 N(0, 1): operand noise of two units in the last place."""
    cl = list(cl)
    rng = np.random.default_rng(seed)
    for k in (0, 1, 3):
        cl[k] = cl[k] * (1.0 + 4e-16 * rng.standard_normal(cl[k].shape))
    return tuple(cl)


def hyper_rbf_prom(X, dt, nT, u0, mu1, E, mu2, U_p, U_s, X_train, W, epsilon, x_min, x_max, y_min, y_max, projection, kernel,
                   rows, xi, tol=1e-6, max_it=30, backwards=False):
    """(Q (n, nT+1), Qs (nbar, nT+1), iters): pod_rbf_prom (oracle/burgers_ref.py) with the two projections as sums over the
    mesh rows ``rows`` weighted by ``xi``, and without the re-projection q_p = U_p^T U0: column 0 of Q is U_p^T u0, afterwards
    q_p carries over (q_p <- q_p + dq).  The state is the decode U_p q_p + U_s f(q_p) except in the first iteration of the
    run, which assembles at u0 itself and takes u^n = u0.  err = |dq| / |q_p| (|dq| when |q_p| = 0).  Qs holds the closure
    value of every step's decode (column 0: zeros).  ``backwards``: sum the rows in descending order."""
    from oracle import burgers_ref as br
    assert projection in ("Galerkin", "LSPG") and kernel in ("gaussian", "imq")
    X = np.asarray(X, dtype=np.float64)
    rows, xi = np.asarray(rows, dtype=np.int64), np.asarray(xi, dtype=np.float64)
    if backwards:
        rows, xi = rows[::-1], xi[::-1]
    rb = (X_train, W, epsilon, kernel, x_min, x_max, y_min, y_max)
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
            lo, di, up = [m + dt * (c + E * kk) for m, c, kk in zip(M3, C3, K3)]
            lo[0] = 0.0; di[0] = 1.0; up[0] = 0.0
            b = Mun + dt * (F - S)
            b[0] = mu1
            R = br.tridiag_matvec(lo, di, up, U0) - b
            Wt = U_p + U_s @ br.rbf_jacobian(q_p, *rb)
            Y = br.tridiag_matmat(lo, di, up, Wt)
            T = Wt if projection == "Galerkin" else Y
            Ar, br_ = np.zeros((n, n)), np.zeros(n)
            for i, w in zip(rows, xi):                      # one row at a time: the order of the sum is the order of ``rows``
                Ar += w * np.outer(T[i], Y[i])
                br_ += w * T[i] * R[i]
            dq = np.linalg.solve(Ar, -br_)
            q_p = q_p + dq
            q_s = br.rbf_value(q_p, *rb)
            U0 = U_p @ q_p + U_s @ q_s
            denom = np.linalg.norm(q_p)
            err = (np.linalg.norm(dq) / denom) if denom > 0 else np.linalg.norm(dq)
            k += 1
        iters[nt] = k
        Q[:, nt + 1], Qs[:, nt + 1] = q_p, q_s
    return Q, Qs, iters
