"""CPU-side checks of the POD-RBF builder: the new entry points (bg_rbf_gram, bg_chol_max_n, bg_chol_factor, bg_chol_solve)
are exported, declared and validate their arguments before anything is launched, and pod.fit_rbf_weights /
pod.build_rbf_closure / save_rbf_closure on CPU tensors reproduce the NumPy references of rbf_builder_ref.

Gates: the backward error |A W - Y|_F / (|A|_2 |W|_F + |Y|_F) <= 4 n 2^-53 (the Cholesky bound at order n); 1e-10 on weights
(the project's parity tolerance, loop_cases.TOL) only where the references themselves agree far inside it; 1e-13 on the
scaled data (test_local_builder_abi.py)."""
import os
import re

import numpy as np
import pytest

import rbf_builder_ref as ref
from conftest import REPO
from loop_cases import TOL, built_library

NEW = ("bg_rbf_gram", "bg_chol_max_n", "bg_chol_factor", "bg_chol_solve")


@pytest.fixture(scope="module")
def L():
    return built_library()


def test_new_symbols_are_exported_declared_and_bound(L):
    from burgers_hip import lib
    header = open(os.path.join(REPO, "include", "burgers_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in lib.declared_symbols(), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert L.bg_abi_version() == 1
    assert L.bg_chol_max_n() >= 8192


def test_argument_validation_before_launch(L):
    from burgers_hip import lib
    null = None
    big = L.bg_chol_max_n() + 1

    def gram(Ns=10, n=3, kind=lib.BG_RBF_GAUSSIAN, ridge=1e-8, lda=None):
        return L.bg_rbf_gram(Ns, n, kind, 2.0, ridge, null, null, Ns if lda is None else lda, null)

    assert gram(Ns=0) == lib.BG_OK
    assert gram(Ns=-1) == lib.BG_ERR_BAD_ARG
    assert gram(n=0) == lib.BG_ERR_BAD_ARG
    assert gram(lda=9) == lib.BG_ERR_BAD_ARG
    assert gram(kind=2) == lib.BG_ERR_BAD_ARG
    assert gram(ridge=-1e-8) == lib.BG_ERR_BAD_ARG
    assert gram(ridge=float("nan")) == lib.BG_ERR_BAD_ARG
    assert gram(ridge=float("inf")) == lib.BG_ERR_BAD_ARG
    assert gram(Ns=big) == lib.BG_ERR_UNSUPPORTED_R
    assert gram() == lib.BG_ERR_BAD_ARG                       # null pointers with centres to work on
    assert gram(kind=lib.BG_RBF_IMQ, ridge=0.0) == lib.BG_ERR_BAD_ARG

    def factor(n=10, lda=None):
        return L.bg_chol_factor(n, null, n if lda is None else lda, null, null)

    assert factor(n=0) == lib.BG_OK
    assert factor(n=-1) == lib.BG_ERR_BAD_ARG
    assert factor(lda=9) == lib.BG_ERR_BAD_ARG
    assert factor(n=big) == lib.BG_ERR_UNSUPPORTED_R
    assert factor() == lib.BG_ERR_BAD_ARG

    def solve(n=10, nrhs=4, lda=None, ldb=None):
        return L.bg_chol_solve(n, nrhs, null, n if lda is None else lda, null, nrhs if ldb is None else ldb, null)

    assert solve(n=0) == lib.BG_OK
    assert solve(nrhs=0) == lib.BG_OK
    assert solve(n=-1) == lib.BG_ERR_BAD_ARG
    assert solve(nrhs=-1) == lib.BG_ERR_BAD_ARG
    assert solve(lda=9) == lib.BG_ERR_BAD_ARG
    assert solve(ldb=3) == lib.BG_ERR_BAD_ARG
    assert solve(n=big) == lib.BG_ERR_UNSUPPORTED_R
    assert solve() == lib.BG_ERR_BAD_ARG


@pytest.mark.parametrize("kernel,eps", ref.KERNELS)
def test_fit_on_cpu_tensors_recovers_the_golden_weights(L, kernel, eps):
    """Ys := (K + 1e-8 I) W_golden, so the golden weights are the exact solution up to the rounding of one product."""
    import torch
    from burgers_hip import pod
    _, Xs, eps_g, A, Ys, Wg = ref.golden_system(kernel)
    assert eps_g == eps
    assert ref.rel(ref.chol_solve(A, Ys), Wg) <= TOL / 100.0                 # the reference alone stays far inside the gate
    info = {}
    W = pod.fit_rbf_weights(torch.from_numpy(Xs), torch.from_numpy(Ys), eps, kernel, ridge=1e-8, info=info).numpy()
    err = ref.rel(W, Wg)
    print(f"{kernel}: |W - W_golden| / |W_golden| = {err:.2e}, backward error {ref.backward_error(A, W, Ys):.2e}")
    assert err <= TOL
    assert ref.backward_error(A, W, Ys) <= ref.gate(len(A)) and info["backward_error"] <= ref.gate(len(A))
    Kt = pod.rbf_kernel_matrix(torch.from_numpy(Xs), eps, kernel, ridge=1e-8).numpy()
    assert np.abs(Kt - A).max() <= 1e-13 and np.array_equal(Kt, Kt.T) and np.all(np.diag(Kt) == 1.0 + 1e-8)
    lib_W = pod.fit_rbf_weights(torch.from_numpy(Xs), torch.from_numpy(Ys), eps, kernel, ridge=1e-8, solver="library").numpy()
    assert ref.rel(lib_W, Wg) <= TOL


@pytest.mark.parametrize("centres", ref.CENTRES, ids=["all", "linspace93", "indices"])
@pytest.mark.parametrize("kernel,eps", ref.KERNELS)
def test_build_rbf_closure_on_cpu_tensors_is_the_reference_rule(L, kernel, eps, centres):
    import torch
    from burgers_hip import pod
    S, U = ref.builder_snapshots()
    assert S.shape == (96, 302)
    n, nbar = ref.BUILDER["n"], ref.BUILDER["nbar"]
    arg = None if centres is None else (centres if np.ndim(centres) == 0 else np.asarray(centres))
    # ridge 1e-3: condition <= 1e6 (asserted by the helper), the weights against the LU solution
    want = ref.builder_case(kernel, eps, 1e-3, centres)
    assert ref.rel(want["W_chol"], want["W_lu"]) <= TOL / 10.0
    fit = pod.build_rbf_closure(torch.from_numpy(S), n, nbar, eps, kernel=kernel, ridge=1e-3, centres=arg, U=torch.from_numpy(U))
    assert np.array_equal(fit.centre_index.numpy(), want["idx"]) and fit.centre_index.dtype == torch.int64
    assert fit.X_train.shape == want["Xs"].shape and fit.W.shape == want["W_lu"].shape
    assert np.abs(fit.X_train.numpy() - want["Xs"]).max() <= 1e-13
    for name in ("x_min", "x_max", "y_min", "y_max"):
        assert np.abs(getattr(fit, name).numpy() - want[name]).max() <= 1e-13 * np.abs(want[name]).max(), name
    assert np.array_equal(fit.U_p.numpy(), want["U_p"]) and np.array_equal(fit.U_s.numpy(), want["U_s"])
    err = ref.rel(fit.W.numpy(), want["W_lu"])
    print(f"{kernel}, ridge 1e-3, {len(want['idx'])} centres: |W - W_lu| / |W_lu| = {err:.2e}")
    assert err <= TOL
    assert (fit.kernel, fit.epsilon, fit.ridge) == (kernel, eps, 1e-3)
    args = fit.prom_args()
    assert len(args) == 9 and args[0] is fit.U_p and args[4] == eps and np.array_equal(args[3], fit.W.numpy())
    # ridge 1e-8: LU and Cholesky themselves differ by 1e-8 on such data, so the backward error only
    want = ref.builder_case(kernel, eps, 1e-8, centres)
    fit = pod.build_rbf_closure(torch.from_numpy(S), n, nbar, eps, kernel=kernel, ridge=1e-8, centres=arg, U=torch.from_numpy(U))
    be = ref.backward_error(want["A"], fit.W.numpy(), want["Ys"])
    print(f"{kernel}, ridge 1e-8: backward error {be:.2e} (gate {ref.gate(len(want['A'])):.2e}), reported {fit.backward_error:.2e}")
    assert be <= ref.gate(len(want["A"])) and fit.backward_error <= ref.gate(len(want["A"]))


def test_save_load_round_trip_is_bitwise_and_pickle_free(L, tmp_path):
    import torch
    from burgers_hip import pod
    S, U = ref.builder_snapshots()
    fit = pod.build_rbf_closure(torch.from_numpy(S), 8, 20, 1.5, kernel="imq", ridge=1e-3, centres=93, U=torch.from_numpy(U))
    d = pod.save_rbf_closure(str(tmp_path / "closure"), fit)
    for f in sorted(os.listdir(d)):
        assert f.endswith((".npy", ".npz"))
        z = np.load(os.path.join(d, f), allow_pickle=False)                   # raises on an object array
        for k in (z.files if hasattr(z, "files") else ()):
            assert z[k].dtype != object
    back = pod.load_rbf_closure(d)
    for name in ("U_p", "U_s", "X_train", "W", "x_min", "x_max", "y_min", "y_max", "centre_index"):
        a, b = getattr(fit, name), getattr(back, name)
        assert a.dtype == b.dtype and torch.equal(a, b), name
    assert (back.epsilon, back.kernel, back.ridge, back.backward_error) == (fit.epsilon, fit.kernel, fit.ridge, fit.backward_error)
    for a, b in zip(fit.prom_args(), back.prom_args()):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_builder_and_solver_refusals(L):
    import torch
    from burgers_hip import pod
    S, U = ref.builder_snapshots()
    St, Ut = torch.from_numpy(S), torch.from_numpy(U)
    with pytest.raises(ValueError):
        pod.build_rbf_closure(St, 8, 20, 2.0, kernel="multiquadric", U=Ut)
    with pytest.raises(ValueError):
        pod.build_rbf_closure(St, 8, 89, 2.0, U=Ut)                            # 97 of 96 singular vectors
    with pytest.raises(ValueError):
        pod.build_rbf_closure(St, 8, 89, 2.0)
    with pytest.raises(ValueError):
        pod.build_rbf_closure(St, 8, 20, 2.0, centres=303, U=Ut)
    with pytest.raises(ValueError):
        pod.build_rbf_closure(St, 8, 20, 2.0, centres=np.array([4, 9, 4]), U=Ut)
    with pytest.raises(ValueError):
        pod.build_rbf_closure(St, 8, 20, 2.0, ridge=-1e-8, U=Ut)
    with pytest.raises(ValueError):
        pod.build_rbf_closure(St, 8, 20, 2.0, solver="qr", U=Ut)
    many = torch.zeros((3, L.bg_chol_max_n() + 1), dtype=torch.float64)        # refused before anything is computed
    with pytest.raises(ValueError):
        pod.build_rbf_closure(many, 1, 1, 2.0, U=torch.eye(3, dtype=torch.float64))
    with pytest.raises(ValueError):
        pod.fit_rbf_weights(torch.zeros((5, 2), dtype=torch.float64), torch.zeros((5, 1), dtype=torch.float64), 2.0, ridge=-1.0)
    eye = torch.eye(6, dtype=torch.float64)
    info = {}
    with pytest.raises(np.linalg.LinAlgError, match="ridge"):
        pod.spd_solve(-eye, torch.ones((6, 2), dtype=torch.float64), info=info)
    assert info["info"] == 1
    bad = torch.ones((6, 2), dtype=torch.float64)
    bad[3, 1] = float("nan")
    with pytest.raises(np.linalg.LinAlgError):
        pod.spd_solve(eye, bad)
    one = pod.spd_solve(4.0 * eye, torch.ones((6,), dtype=torch.float64))      # a vector right-hand side; sqrt(4) is exact
    assert one.shape == (6,) and torch.equal(one, torch.full((6,), 0.25, dtype=torch.float64))
