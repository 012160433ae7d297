"""The device-side POD-RBF builder against the NumPy / SciPy references of rbf_builder_ref: bg_rbf_gram, bg_chol_factor,
bg_chol_solve, pod.spd_solve, pod.fit_rbf_weights and pod.build_rbf_closure, end to end into rom.pod_rbf_run and
FEMBurgers.pod_rbf_prom against the reference's recorded output.

Gates: the backward error <= 4 n 2^-53 (ref.gate); the spread s between SciPy's Cholesky and NumPy's LU solution of the same
system, and the difference between the NumPy block-64 factor and LAPACK's, both computed here from the references alone;
1e-9, 1e-10 and 1e-13 from the project's existing tests."""
import functools

import numpy as np
import pytest

import rbf_builder_ref as ref
from conftest import mesh, rel_l2
from loop_cases import TOL

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _gram(hip, Xs, eps, kernel, ridge, lda=None, fill=-7.0):
    """The raw entry point on scaled centres Xs (Ns, n): the (Ns, lda) array it wrote into one filled with ``fill``."""
    import torch
    Ns, n = Xs.shape
    lda = Ns if lda is None else lda
    XtT = _dev(Xs.T)
    A = torch.full((Ns, lda), fill, dtype=torch.float64, device="cuda")
    kind = hip.BG_RBF_GAUSSIAN if kernel == "gaussian" else hip.BG_RBF_IMQ
    hip.check(hip.load().bg_rbf_gram(Ns, n, kind, eps, ridge, hip.ptr(XtT), hip.ptr(A), lda, hip.stream_ptr(A.device)), "bg_rbf_gram")
    torch.cuda.synchronize()
    return A.cpu().numpy()


def _factor(hip, A):
    """bg_chol_factor on a copy of A: (the device matrix afterwards, info)."""
    import torch
    n = len(A)
    Ld = _dev(A)
    info = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    hip.check(hip.load().bg_chol_factor(n, hip.ptr(Ld), n, hip.ptr(info), hip.stream_ptr(Ld.device)), "bg_chol_factor")
    torch.cuda.synchronize()
    return Ld, int(info.item())


def _solve(hip, Ld, B):
    import torch
    n, nrhs = B.shape
    Bd = _dev(B)
    hip.check(hip.load().bg_chol_solve(n, nrhs, hip.ptr(Ld), n, hip.ptr(Bd), nrhs, hip.stream_ptr(Bd.device)), "bg_chol_solve")
    torch.cuda.synchronize()
    return Bd.cpu().numpy()


# ---- 1. the kernel matrix -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,eps", ref.KERNELS)
@pytest.mark.parametrize("n", [1, 17, 20])
@pytest.mark.parametrize("Ns", [1, 63, 64, 65, 300])
def test_gram_is_symmetric_exact_on_the_diagonal_and_the_numpy_matrix(hip, Ns, n, kernel, eps):
    Xs = np.random.default_rng([Ns, n]).uniform(-1.0, 1.0, (Ns, n))
    ridge = 1e-8
    lda = Ns + 5 if Ns == 65 else Ns
    out = _gram(hip, Xs, eps, kernel, ridge, lda)
    A = out[:, :Ns]
    assert np.array_equal(A, A.T)
    assert np.all(np.diag(A) == 1.0 + ridge)
    assert np.abs(A - ref.kernel_matrix(Xs, eps, kernel, ridge)).max() <= 1e-13
    assert np.all(out[:, Ns:] == -7.0)                                          # the padding columns are not touched


# ---- 2. factorisation and solve -----------------------------------------------------------------------------------------
ORDERS = [1, 5, 63, 64, 65, 128, 279, 300]     # no full tile, one tile, a tile and a row, whole tiles, ragged multi-tile
NRHS = [1, 20, 79, 130]


@functools.lru_cache(maxsize=None)
def _spd_case(n):
    """(A, LAPACK factor, the bound on the factor): left as they are by every test."""
    A = ref.spd_matrix(n)
    assert np.linalg.cond(A) < 10.0
    Lw = np.linalg.cholesky(A)
    return A, Lw, max(1e-14, 100.0 * ref.rel(ref.block_cholesky(A), Lw))


@pytest.mark.parametrize("n", ORDERS)
def test_factor_and_solve_against_lapack(hip, n):
    A, Lw, bound = _spd_case(n)
    Ld, info = _factor(hip, A)
    assert info == 0
    Lg = np.tril(Ld.cpu().numpy())
    err = ref.rel(Lg, Lw)
    print(f"n = {n}: |L - L_lapack| / |L_lapack| = {err:.2e} (bound {bound:.2e})")
    assert err <= bound
    for nrhs in NRHS:
        B = ref.rhs(n, nrhs)
        want = ref.lu_solve(A, B)
        tol = max(1e-14, 100.0 * ref.spread(A, B))
        X = _solve(hip, Ld, B)
        e, be = ref.rel(X, want), ref.backward_error(A, X, B)
        print(f"n = {n}, nrhs = {nrhs}: |X - X_lu| / |X_lu| = {e:.2e} (bound {tol:.2e}), backward error {be:.2e} (gate {ref.gate(n):.2e})")
        assert e <= tol
        assert be <= ref.gate(n)


# ---- 3. determinism and locality, bitwise -------------------------------------------------------------------------------
def test_factor_and_solve_are_reproducible_and_local(hip):
    import torch
    A, _, _ = _spd_case(279)
    L1, i1 = _factor(hip, A)
    L2, i2 = _factor(hip, A)
    assert i1 == 0 and i2 == 0
    low = lambda t: np.tril(t.cpu().numpy())
    assert np.array_equal(low(L1), low(L2))
    Ls, i3 = _factor(hip, np.ascontiguousarray(A[:128, :128]))
    assert i3 == 0 and np.array_equal(low(Ls), low(L1)[:128, :128])            # nothing below or right of an element enters it
    B = ref.rhs(279, 79)
    X = _solve(hip, L1, B)
    assert np.array_equal(_solve(hip, L1, B), X)
    for c in (0, 17, 78):
        assert np.array_equal(_solve(hip, L1, np.ascontiguousarray(B[:, c:c + 1]))[:, 0], X[:, c]), c
    assert np.array_equal(torch.triu(L1, 1).cpu().numpy(), np.triu(A, 1))      # the upper triangle is left alone


# ---- 4. info ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,value", [(0, -1.0), (63, -1.0), (64, -1.0), (129, -1.0), (64, float("nan"))])
def test_factor_reports_the_first_bad_pivot(hip, k, value):
    """An ordinary return-code path: every launch returns normally and info names the pivot, as LAPACK's dpotrf does."""
    A = np.eye(130)
    A[k, k] = value
    _, info = _factor(hip, A)
    assert info == k + 1


def test_spd_solve_raises_on_an_indefinite_matrix(hip):
    from burgers_hip import pod
    A = np.eye(130)
    A[64, 64] = -1.0
    info = {}
    with pytest.raises(np.linalg.LinAlgError, match="pivot 64"):
        pod.spd_solve(_dev(A), _dev(np.ones((130, 3))), info=info)
    assert info["info"] == 65


# ---- 5. the fit on the device -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden_fit(kernel):
    """The closure weights refitted on the device from the fixture's centres and Ys := (K + 1e-8 I) W_golden."""
    from burgers_hip import pod
    _, Xs, eps, A, Ys, _ = ref.golden_system(kernel)
    info = {}
    W = pod.fit_rbf_weights(_dev(Xs), _dev(Ys), eps, kernel, ridge=1e-8, info=info)
    return W, info


@pytest.mark.parametrize("kernel,eps", ref.KERNELS)
def test_fit_on_the_device_recovers_the_golden_weights(hip, kernel, eps):
    from burgers_hip import pod
    _, Xs, _, A, Ys, Wg = ref.golden_system(kernel)
    Wd, info = _golden_fit(kernel)
    assert Wd.is_cuda and info["info"] == 0
    W = Wd.cpu().numpy()
    err, be = ref.rel(W, Wg), ref.backward_error(A, W, Ys)
    print(f"{kernel}: |W - W_golden| / |W_golden| = {err:.2e}, backward error {be:.2e} (reported {info['backward_error']:.2e})")
    assert err <= TOL
    assert be <= ref.gate(len(A)) and info["backward_error"] <= ref.gate(len(A))
    Wl = pod.fit_rbf_weights(_dev(Xs), _dev(Ys), eps, kernel, ridge=1e-8, solver="library").cpu().numpy()
    tol = max(1e-13, 100.0 * ref.spread(A, Ys))
    print(f"{kernel}: library against cholesky {ref.rel(Wl, W):.2e} (bound {tol:.2e})")
    assert ref.rel(Wl, W) <= tol


# ---- 6. the pipeline on the device --------------------------------------------------------------------------------------
def _held_out(hip, fit, want, kernel, eps):
    """Relative differences of the closure on the non-centre snapshots: (the built closure against the helper's LU closure,
    the helper's Cholesky closure against its LU closure)."""
    import torch
    from burgers_hip import rom
    rest = np.setdiff1d(np.arange(len(want["Q"])), want["idx"])
    q = np.ascontiguousarray(want["Q"][rest])
    ranges = [want[k].copy() for k in ("x_min", "x_max", "y_min", "y_max")]
    lu = ref.closure_value(q, want["Xs"], want["W_lu"], eps, kernel, *ranges)
    ch = ref.closure_value(q, want["Xs"], want["W_chol"], eps, kernel, *ranges)
    args = fit.prom_args()
    got = rom.RbfClosure(args[2], args[3], args[4], kernel, *args[5:], torch.device("cuda", torch.cuda.current_device())).value(_dev(q))
    return ref.rel(got.cpu().numpy(), lu), ref.rel(ch, lu)


@pytest.mark.parametrize("centres", ref.CENTRES, ids=["all", "linspace93", "indices"])
@pytest.mark.parametrize("kernel,eps", ref.KERNELS)
def test_build_rbf_closure_on_the_device_is_the_reference_rule(hip, kernel, eps, centres):
    import torch
    from burgers_hip import pod
    S, U = ref.builder_snapshots()
    n, nbar = ref.BUILDER["n"], ref.BUILDER["nbar"]
    arg = None if centres is None else (centres if np.ndim(centres) == 0 else np.asarray(centres))
    Sd, Ud = _dev(S), _dev(U)
    for ridge in (1e-3, 1e-8):
        want = ref.builder_case(kernel, eps, ridge, centres)
        fit = pod.build_rbf_closure(Sd, n, nbar, eps, kernel=kernel, ridge=ridge, centres=arg, U=Ud)
        assert fit.W.is_cuda and fit.X_train.is_cuda and fit.centre_index.dtype == torch.int64
        assert np.array_equal(fit.centre_index.cpu().numpy(), want["idx"])
        assert np.abs(fit.X_train.cpu().numpy() - want["Xs"]).max() <= 1e-13
        for name in ("x_min", "x_max", "y_min", "y_max"):
            assert np.abs(getattr(fit, name).cpu().numpy() - want[name]).max() <= 1e-13 * np.abs(want[name]).max(), name
        W = fit.W.cpu().numpy()
        be = ref.backward_error(want["A"], W, want["Ys"])
        print(f"{kernel}, ridge {ridge:g}, {len(want['idx'])} centres: |W - W_lu| / |W_lu| = {ref.rel(W, want['W_lu']):.2e}, "
              f"backward error {be:.2e} (gate {ref.gate(len(W)):.2e}, reported {fit.backward_error:.2e})")
        if ridge == 1e-3:
            assert ref.rel(W, want["W_lu"]) <= TOL                              # at 1e-8 LU and Cholesky themselves differ by 1e-8
        assert be <= ref.gate(len(W)) and fit.backward_error <= ref.gate(len(W))
        if centres is not None:
            got, between = _held_out(hip, fit, want, kernel, eps)
            print(f"    held out: against the LU closure {got:.2e}; Cholesky against LU closure {between:.2e}")
            assert got <= max(1e-10, 100.0 * between)


def test_build_rbf_closure_with_its_own_basis(hip):
    import torch
    from burgers_hip import pod
    S, _ = ref.builder_snapshots()
    n, nbar = ref.BUILDER["n"], ref.BUILDER["nbar"]
    fit = pod.build_rbf_closure(_dev(S), n, nbar, 2.0, ridge=1e-3, centres=93)
    assert fit.U_p.shape == (96, n) and fit.U_s.shape == (96, nbar) and fit.X_train.shape == (93, n) and fit.W.shape == (93, nbar)
    eye = torch.eye(n, dtype=torch.float64, device="cuda")
    assert float((fit.U_p.t() @ fit.U_p - eye).abs().max()) <= 1e-12
    # the ridge system of the fit's own scaled data, rebuilt on the host
    Xs = fit.X_train.cpu().numpy()
    Qb = (fit.U_s.cpu().numpy().T @ S).T
    y_min, dy = fit.y_min.cpu().numpy(), (fit.y_max - fit.y_min).cpu().numpy()
    Ys = 2.0 * (Qb[fit.centre_index.cpu().numpy()] - y_min) / dy - 1.0
    be = ref.backward_error(ref.kernel_matrix(Xs, 2.0, "gaussian", 1e-3), fit.W.cpu().numpy(), Ys)
    assert be <= ref.gate(93) and fit.backward_error <= ref.gate(93)


# ---- 7. end to end against the reference's recorded output ---------------------------------------------------------------
@pytest.mark.parametrize("kernel,proj", [("gaussian", "LSPG"), ("imq", "Galerkin")])
def test_refitted_closure_runs_the_recorded_prom(hip, kernel, proj, tmp_path):
    """The gate of test_pod_rbf_prom_live_reference, with the weights refitted on the device instead of the golden ones."""
    import torch
    from burgers_hip import pod, rom
    from fem_burgers import FEMBurgers
    g, Xs, eps, _, _, _ = ref.golden_system(kernel)
    Wd, info = _golden_fit(kernel)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fit = pod.RbfFit(t(g["U_p"]), t(g["U_s"]), t(Xs), Wd, eps, kernel, t(g["x_min"]), t(g["x_max"]), t(g["y_min"]), t(g["y_max"]),
                     1e-8, torch.as_tensor(np.linspace(0, 4500, 300).astype(int)).cuda(), info["backward_error"])
    X, T = mesh(512)
    for fused in (False, True):
        res = rom.pod_rbf_run(X, np.ones(512), [float(g["mu1"])], [float(g["mu2"])], float(g["At"]), int(g["nT"]),
                              *fit.prom_args(), projection=proj, kernel=kernel, max_newton=20, fused=fused)
        torch.cuda.synchronize()
        err = rel_l2(res.hist[0].cpu().numpy().T, g["U_" + kernel])
        print(f"{kernel} {proj} fused={fused}: rel-L2 against the recorded output {err:.2e}")
        assert err < 1e-9
        assert np.array_equal(res.iters[0].cpu().numpy(), g["iters_" + kernel])
    back = pod.load_rbf_closure(pod.save_rbf_closure(str(tmp_path / "closure"), fit), device="cuda")
    assert torch.equal(back.W, fit.W) and back.kernel == kernel
    U = FEMBurgers(X, T).pod_rbf_prom(float(g["At"]), int(g["nT"]), np.ones(512), float(g["mu1"]), 0.0, float(g["mu2"]),
                                      *back.prom_args(), projection=proj, kernel=back.kernel, tol_newton=1e-6, max_newton=20,
                                      fused=True)
    assert np.asarray(U).shape == (512, 5) and rel_l2(np.asarray(U), g["U_" + kernel]) < 1e-9
