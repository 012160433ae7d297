"""What the tests (and the timer) of the POD-RBF loop for meshes of 513 .. 1024 nodes share: the bases for an N-node mesh made
from the reference's live fixture (tests/golden/rbf_n17.npz, a 512-node mesh), the cases the loop is tested at with the
iteration counts the oracle gives for them, and one cached oracle run per case.  numpy only at import; the oracle is
imported where it is used."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rbf_n17.npz")
TOL = 1e-9            # the project's own gate for this closure (weights up to 3.6e2), tests/test_rom_rbf_fused_gpu.py


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def long_bases(N, extra=0):
    """(U_p, U_s): the fixture's 17 + 79 basis columns carried to an N-node mesh.  The 96 columns are interpolated linearly
    from the 512-node uniform mesh by node index (so a graded mesh gets the same columns), ``extra`` columns
    sin(pi k i / (N - 1)), k = 200 .. 199 + extra, are appended, and the thin QR with diag R > 0 makes them orthonormal:
    without that step U_p^T (U_p q + U_s f) != q and every run ends at the iteration cap."""
    g = golden()
    src = np.arange(N) * (511.0 / (N - 1))
    cols = np.concatenate([g["U_p"], g["U_s"]], axis=1)
    A = np.stack([np.interp(src, np.arange(512.0), cols[:, j]) for j in range(cols.shape[1])], axis=1)
    if extra:
        xi = np.arange(N) / (N - 1.0)
        A = np.concatenate([A] + [np.sin(np.pi * xi * k)[:, None] for k in range(200, 200 + extra)], axis=1)
    Q, R = np.linalg.qr(A)
    Q = Q * np.sign(np.diag(R))[None, :]
    Q.setflags(write=False)
    return Q[:, :17], Q[:, 17:]


def long_mesh(N, jitter_seed=None):
    X = np.linspace(0.0, 100.0, N)
    if jitter_seed is not None:
        X[1:-1] += np.random.default_rng(jitter_seed).uniform(-0.2, 0.2, N - 2) * (X[1] - X[0])
    return X


def closure(N, kernel, shape="plain"):
    """The nine closure arguments (U_p, U_s, X_train, W, eps, x_min, x_max, y_min, y_max) of pod_rbf_prom on an N-node mesh.
    ``shape``: "plain" (n = 17, nbar = 79, 300 centres); "n20" (n = 20, nbar = 76: the first three secondary columns move
    to the primary side with zero centre coordinates and x_min = x_max = 0); "nbar128" (nbar = 128 with 49 extra columns
    of zero weight and range, and 2400 centres: eight jittered copies of X_train, the weights divided by 8)."""
    g = golden()
    Xt, W, eps = g["X_train"], g["W_" + kernel], float(g["eps_" + kernel])
    x_min, x_max, y_min, y_max = g["x_min"], g["x_max"], g["y_min"], g["y_max"]
    if shape == "plain":
        Up, Us = long_bases(N)
    elif shape == "n20":
        Up, Us = long_bases(N)
        Up, Us = np.concatenate([Up, Us[:, :3]], axis=1), Us[:, 3:]
        Xt = np.concatenate([Xt, np.zeros((Xt.shape[0], 3))], axis=1)
        x_min, x_max = np.concatenate([x_min, np.zeros(3)]), np.concatenate([x_max, np.zeros(3)])
        W, y_min, y_max = W[:, 3:], y_min[3:], y_max[3:]
    elif shape == "nbar128":
        Up, Us = long_bases(N, extra=49)
        rng = np.random.default_rng(7)
        Xt = np.concatenate([Xt + (0 if c == 0 else 1e-3) * rng.standard_normal(Xt.shape) for c in range(8)])
        W = np.concatenate([np.concatenate([W / 8.0] * 8), np.zeros((8 * W.shape[0], 49))], axis=1)
        y_min, y_max = np.concatenate([y_min, np.zeros(49)]), np.concatenate([y_max, np.zeros(49)])
    else:
        raise KeyError(shape)
    return (np.ascontiguousarray(Up), np.ascontiguousarray(Us), Xt, np.ascontiguousarray(W), eps, x_min, x_max, y_min, y_max)


# name: N, kernel, projection, (mu1, mu2) of the two samples, dt, steps, max_newton, E, jitter seed, closure shape, and the
# oracle's iteration counts of the first sample.  u0 = 1 everywhere.
CASES = {
    "n1024-imq-lspg":       (1024, "imq", "LSPG", ((4.3, 0.016), (4.75, 0.02)), 0.025, 4, 30, 0.0, None, "plain", [30, 9, 8, 5]),
    "n1024-imq-galerkin":   (1024, "imq", "Galerkin", ((4.75, 0.02), (4.3, 0.016)), 0.1, 4, 30, 0.0, None, "plain", [9, 30, 28, 10]),
    "n1024-gauss-galerkin": (1024, "gaussian", "Galerkin", ((4.3, 0.016), (4.75, 0.02)), 0.05, 4, 30, 0.0, None, "plain", [21, 22, 30, 30]),
    "n513-imq-galerkin":    (513, "imq", "Galerkin", ((4.75, 0.02), (4.3, 0.016)), 0.05, 4, 30, 0.0, None, "plain", [6, 18, 16, 13]),
    "n513-gauss-lspg":      (513, "gaussian", "LSPG", ((4.75, 0.02), (4.3, 0.016)), 0.05, 4, 30, 0.0, None, "plain", [7, 30, 10, 9]),
    "n600-gauss-lspg":      (600, "gaussian", "LSPG", ((4.75, 0.02), (4.3, 0.016)), 0.05, 4, 30, 0.0, None, "plain", [9, 30, 10, 7]),
    "n777-graded-imq-lspg": (777, "imq", "LSPG", ((4.6, 0.018), (5.3, 0.027)), 0.05, 4, 30, 0.02, 777, "plain", [30, 30, 6, 10]),
    "n1024-cap2":           (1024, "gaussian", "LSPG", ((4.75, 0.02), (4.3, 0.016)), 0.05, 3, 2, 0.0, None, "plain", [2, 2, 2]),
    "n1023-imq-lspg":       (1023, "imq", "LSPG", ((4.3, 0.016), (4.75, 0.02)), 0.025, 4, 30, 0.0, None, "plain", None),
    "n20-gauss-lspg":       (1024, "gaussian", "LSPG", ((4.3, 0.016), (4.75, 0.02)), 0.025, 3, 30, 0.0, None, "n20", [4, 4, 4]),
    "n20-gauss-galerkin":   (1024, "gaussian", "Galerkin", ((4.3, 0.016), (4.75, 0.02)), 0.025, 3, 3, 0.0, None, "n20", [3, 3, 3]),
    "nbar128-imq-galerkin": (1024, "imq", "Galerkin", ((4.3, 0.016), (4.75, 0.02)), 0.025, 3, 30, 0.0, None, "nbar128", [30, 30, 30]),
}


def case_inputs(name):
    """(X, mus, dt, steps, E, the nine closure arguments, the other keyword arguments of pod_rbf_prom / pod_rbf_run_long)."""
    N, kernel, proj, mus, dt, steps, max_newton, E, seed, shape, _ = CASES[name]
    return long_mesh(N, seed), mus, dt, steps, E, closure(N, kernel, shape), dict(projection=proj, kernel=kernel, max_newton=max_newton)


def _oracle(name, cl):
    from oracle import burgers_ref as br
    X, mus, dt, steps, E, _, kw = case_inputs(name)
    return [br.pod_rbf_prom(X, dt, steps, np.ones(len(X)), m1, E, m2, *cl, return_iters=True, **kw) for m1, m2 in mus]


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """[(U, iters)] of the case's two samples by the oracle: one run per process, shared by the tests; leave it as it is."""
    return _oracle(name, case_inputs(name)[5])


def oracle_run_perturbed(name, seed=20251121):
    """The same with U_p, U_s and W multiplied entrywise by 1 + 4e-16 N(0, 1): operand noise of two units in the last place."""
    cl = list(case_inputs(name)[5])
    rng = np.random.default_rng(seed)
    for k in (0, 1, 3):
        cl[k] = cl[k] * (1.0 + 4e-16 * rng.standard_normal(cl[k].shape))
    return _oracle(name, tuple(cl))
