"""CPU-side checks of the device-side NNLS for the row samplings: bg_nnls_limits covers the 511 free rows of
bg_hyper_rom_run_wide, every bg_nnls_* entry point validates its arguments before anything is launched, and the ``solver``
argument of the build_*_row_sampling functions routes as documented: "host" calls _fit_row_sampling with the six arguments it
always had, "device" reaches pod.nnls_rows_device with the arguments pod.nnls_rows would get, anything else is refused."""
import numpy as np
import pytest

from loop_cases import built_library, host_pointers

NEW = ("bg_nnls_limits", "bg_nnls_work_elems", "bg_nnls_pick", "bg_nnls_append", "bg_nnls_solve", "bg_nnls_residual", "bg_nnls_mark")


@pytest.fixture(scope="module")
def L():
    return built_library()


def test_limits_cover_the_wide_loop_and_need_no_device(L):
    from burgers_hip import lib, pod
    max_active, max_cols = lib.limits("bg_nnls_limits", 2)
    assert (max_active, max_cols) == pod.nnls_limits()
    assert max_active >= lib.limits("bg_hyper_rom_wide_limits", 2)[1] - 1 >= 511
    assert max_cols >= L.bg_fom_max_n()
    assert L.bg_nnls_limits(None, None) == lib.BG_ERR_BAD_ARG
    for name in NEW:
        assert hasattr(L, name) and name in lib.declared_symbols(), name
    assert L.bg_nnls_work_elems(24) >= 24 + 2 * max_active and L.bg_nnls_work_elems(-1) == 0
    assert lib.NNLS_STATUS.itemsize == 64


def test_argument_validation_before_launch(L):
    from burgers_hip import lib
    null = None
    p, ip = host_pointers()
    max_active, max_cols = lib.limits("bg_nnls_limits", 2)
    BAD, OK, BIG = lib.BG_ERR_BAD_ARG, lib.BG_OK, lib.BG_ERR_UNSUPPORTED_R

    def pick(rows=10, n=5, ld=16, ops=p, masks=ip, status=p, dnorm=1.0, tau=1e-4, lo=3, hi=8):
        return L.bg_nnls_pick(rows, n, ld, ops, ops, masks, masks, dnorm, tau, lo, hi, ops, status, null)

    assert pick(rows=-1) == BAD and pick(n=-1) == BAD and pick(ld=9) == BAD and pick(lo=-1) == BAD and pick(hi=-1) == BAD
    assert pick(dnorm=-1.0) == BAD and pick(tau=float("nan")) == BAD
    assert pick(ld=11) == BAD                                           # an odd leading dimension: the loads are 16 bytes wide
    assert pick(n=0, ops=null, masks=null, status=null) == OK           # no column: nothing to do
    assert pick(n=max_cols + 1) == BIG and pick(hi=max_active + 1) == BIG
    assert pick(ops=null) == BAD and pick(masks=null) == BAD and pick(status=null) == BAD

    def append(rows=10, ld=16, k=2, rebuild=0, ops=p, masks=ip, status=p, ldr=8):
        return L.bg_nnls_append(rows, ld, k, rebuild, ops, ops, ops, ops, ldr, ops, ops, masks, masks, masks, ops, status, null)

    assert append(rows=-1) == BAD and append(k=-1) == BAD and append(ld=9) == BAD and append(ldr=-1) == BAD
    assert append(ldr=2) == BAD and append(ld=11) == BAD                 # no room for column k; an odd leading dimension
    assert append(rows=0, ld=0, ops=null, masks=null, status=null) == OK
    assert append(k=max_active, ldr=max_active + 1) == BIG
    assert append(ops=null) == BAD and append(masks=null) == BAD and append(status=null) == BAD
    assert append(rebuild=1, ops=null) == BAD

    def solve(k=3, ldr=8, ops=p, masks=ip, status=p):
        return L.bg_nnls_solve(k, ops, ldr, ops, ops, masks, masks, status, null)

    assert solve(k=-1) == BAD and solve(ldr=2) == BAD
    assert solve(k=0, ops=null, masks=null, status=null) == OK
    assert solve(k=max_active + 1, ldr=max_active + 1) == BIG
    assert solve(ops=null) == BAD and solve(masks=null) == BAD and solve(status=null) == BAD

    def residual(rows=10, ld=16, k=2, ops=p, order=ip):
        return L.bg_nnls_residual(rows, ld, k, ops, ops, ops, order, ops, null)

    assert residual(rows=-1) == BAD and residual(k=-1) == BAD and residual(ld=9) == BAD
    assert residual(rows=0, ld=0, ops=null, order=null) == OK
    assert residual(k=max_active + 1) == BIG
    assert residual(ops=null) == BAD and residual(order=null) == BAD

    def mark(n=5, tabu=ip, j=2, value=1):
        return L.bg_nnls_mark(n, tabu, j, value, null)

    assert mark(n=-1) == BAD and mark(j=5) == BAD and mark(tabu=null) == BAD
    assert mark(n=0, j=-1, tabu=null) == OK
    assert mark(n=max_cols + 1) == BIG


def small_case():
    from conftest import mesh
    N = 24
    X, _ = mesh(N)
    rng = np.random.default_rng(3)
    Phi = np.linalg.qr(rng.standard_normal((N, 3)))[0]
    hist = 1.0 + 0.1 * rng.random((N, 5))
    return X, Phi, [(hist, 4.5, 0.02)]


def test_an_unknown_solver_is_refused(L):
    from burgers_hip import pod
    X, Phi, runs = small_case()
    with pytest.raises(ValueError, match="solver"):
        pod.build_row_sampling(X, Phi, runs, 0.05, "Galerkin", stride=1, min_rows=4, solver="bogus")
    G, pairs = pod.row_sampling_system(X, Phi, runs, 0.05, "galerkin", stride=1)
    with pytest.raises(ValueError, match="solver"):
        pod._fit_row_sampling(G, pairs, "galerkin", 1e-4, 4, 24, "bogus")
    with pytest.raises(ValueError, match="max_cols"):                      # beyond bg_nnls_limits: refused before any launch
        pod.nnls_rows_device(G[:, 1:], G.sum(axis=1), 1e-4, 3, pod.nnls_limits()[0] + 1)


def test_the_host_solver_calls_the_fit_with_its_six_arguments(L, monkeypatch):
    from burgers_hip import pod
    X, Phi, runs = small_case()
    seen = []

    def six(G, pairs, projection, tau, min_rows, max_rows):
        seen.append((G.shape, pairs, projection, tau, min_rows, max_rows))
        return "fitted"
    monkeypatch.setattr(pod, "_fit_row_sampling", six)
    assert pod.build_row_sampling(X, Phi, runs, 0.05, "Galerkin", stride=2, min_rows=5, max_rows=20) == "fitted"
    assert pod.build_row_sampling(X, Phi, runs, 0.05, "LSPG", stride=2, min_rows=5, max_rows=20, solver="host") == "fitted"
    assert seen == [((6, 24), 2, "galerkin", 1e-4, 5, 20), ((6, 24), 2, "lspg", 1e-4, 5, 20)]


def test_the_device_solver_reaches_nnls_rows_device_with_the_hosts_arguments(L, monkeypatch):
    from burgers_hip import pod
    X, Phi, runs = small_case()
    calls = {}

    def recorder(name, real):
        def fit(G, d, tau, min_cols, max_cols):
            calls[name] = (G.copy(), d.copy(), tau, min_cols, max_cols)
            return real(G, d, tau, min_cols, max_cols)
        return fit
    monkeypatch.setattr(pod, "nnls_rows_device", recorder("device", pod.nnls_rows))      # no device here: the host's arithmetic
    monkeypatch.setattr(pod, "nnls_rows", recorder("host", pod.nnls_rows))
    dev = pod.build_row_sampling(X, Phi, runs, 0.05, "LSPG", stride=1, min_rows=6, max_rows=20, solver="device")
    assert set(calls) == {"device"}
    host = pod.build_row_sampling(X, Phi, runs, 0.05, "LSPG", stride=1, min_rows=6, max_rows=20)
    assert set(calls) == {"device", "host"}
    for a, b in zip(calls["device"], calls["host"]):
        assert np.array_equal(a, b)
    assert calls["device"][0].shape == (12, 23) and calls["device"][3:] == (5, 19)
    assert np.array_equal(dev.rows.numpy(), host.rows.numpy()) and np.array_equal(dev.xi.numpy(), host.xi.numpy())
    assert dev.residual == host.residual and dev.m >= 6
