"""The offline side of the hyper-reduced local POD PROM, without a GPU: the numpy restatement of bg_hyper_local_rom_run's
semantics (tests/hyper_local_ref.py: the state (p, q), the pick from reduced coordinates, Phi_c^T Phi_p q at a switch), which
with all rows and unit weights must be the oracle's local_prom_burgers, and pod.build_local_row_sampling (ONE NNLS sampling
for all clusters)."""
import functools

import numpy as np
import pytest
import torch

import hyper_local_ref as hl
from conftest import rel_l2
from hyper_ref import training_runs
from loop_cases import TOL, built_library

TAU = 1e-4                     # the builder's default
MIN_ROWS = 100
CASES = {"perturbed-96": (96, 0.07, 0.01, 3), "uniform-256": (256, 0.05, 0.0, None)}


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_with_all_rows_is_the_oracle(case, proj):
    """Also what lets the loop carry q and cross bases on reduced coordinates: for orthonormal bases Phi_c^T u^n is
    Phi_c^T Phi_p q, and U_g^T u^n is (U_g^T Phi_p) q."""
    from oracle import burgers_ref as br
    N, dt, E, seed = CASES[case]
    X, centres, bases, Ug = hl.dense_clustering(N, dt, E, seed)
    for c, b in bases.items():
        assert np.abs(b.T @ b - np.eye(b.shape[1])).max() < 1e-12
    for mu1, mu2 in hl.MUS:
        U, ito, clo = br.local_prom_burgers(X, dt, hl.NT, np.ones(N), mu1, E, mu2, centres, bases, Ug, hl.MG, projection=proj,
                                            return_iters=True)
        Uh, Q, it, cl, margin = hl.hyper_local_prom(X, dt, hl.NT, np.ones(N), mu1, E, mu2, centres, bases, Ug, hl.MG, proj,
                                                    np.arange(N), np.ones(N))
        sw = int((np.diff(clo) != 0).sum())
        err = rel_l2(Uh, U)
        print(f"{case} {proj} mu = ({mu1}, {mu2}): rel-L2 {err:.2e}, {sw} switches, iterations up to {int(ito.max())}, "
              f"tie margin {margin:.1e}")
        # conditions on the input, from the oracle's own output: the run switches, converges and has no near tie
        assert sw >= 4 and ito.max() < 20 and margin >= 1e-8
        assert clo[0] == 0 and bases[0].shape[1] == 8
        assert err < TOL
        assert np.array_equal(cl, clo) and np.array_equal(it, ito)
        assert np.array_equal(Q[:8, 0], bases[int(cl[0])].T @ np.ones(N)) and not Q[8:, 0].any()


@functools.lru_cache(maxsize=None)
def builder_case(proj):
    """Three training runs, every 10th step, ``min_rows`` = 100.  The default (3 x 40 = 120) cannot be reached on this mesh
    from three runs under LSPG: the fit is exact (residual 3e-11) at 116 rows, every further column gets a weight <= 0 and
    nnls_rows says so with its ValueError; all nine runs reach 120 but take 7 s on the host."""
    from burgers_hip import pod
    built_library()                                   # the builder asks the library for the kernel's row limit
    N, dt, E, seed = CASES["uniform-256"]
    X, centres, bases, Ug = hl.dense_clustering(N, dt, E, seed)
    runs = training_runs(N, dt, E, keep=[0, 4, 8])
    return X, centres, bases, Ug, runs, pod.build_local_row_sampling(X, centres, bases, Ug, hl.MG, runs, dt, proj, E=E, min_rows=MIN_ROWS)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_training_matrix_sums_to_the_reduced_right_hand_sides(proj):
    """d = G 1 is, block by block, the reduced right-hand side W^T R of the cluster the reference would hold there, formed
    here from the oracle's assembly functions."""
    from burgers_hip import pod
    from oracle import burgers_ref as br
    N, dt, E, seed = CASES["perturbed-96"]
    X, centres, bases, Ug = hl.dense_clustering(N, dt, E, seed)
    runs = training_runs(N, dt, E, seed, keep=[2, 6])
    G, pairs = pod.local_row_sampling_system(X, centres, bases, Ug, hl.MG, runs, dt, proj.lower(), E, True, 25)
    assert pairs == 2 * 8 and G.shape[1] == N
    M3, K3 = br.mass_tridiag(X), br.diffusion_tridiag(X)
    want, widths = [], []
    for S, mu1, mu2 in runs:
        F = br.forcing_vector(X, mu2)
        for n in range(0, S.shape[1] - 1, 25):
            qg = Ug[:, :hl.MG].T @ S[:, n]
            Phi = bases[int(np.argmin(((centres - qg[None, :]) ** 2).sum(1)))]
            Un, U0 = Phi @ (Phi.T @ S[:, n]), Phi @ (Phi.T @ S[:, n + 1])
            lo, di, up = br.system_tridiag(M3, K3, br.convection_tridiag(X, U0), dt, E)
            b = br.tridiag_matvec(*M3, Un) + dt * F - dt * br.supg_term(X, U0, mu2)
            b[0] = mu1
            R = br.tridiag_matvec(lo, di, up, U0) - b
            W = Phi if proj == "Galerkin" else br.tridiag_matmat(lo, di, up, Phi)
            want.append(W.T @ R)
            widths.append(Phi.shape[1])
    want = np.concatenate(want)
    assert G.shape[0] == len(want) == sum(widths) and len(set(widths)) > 1          # more than one cluster's width
    d = G.sum(axis=1)
    err = np.linalg.norm(d - want) / np.linalg.norm(want)
    print(f"{proj}: {pairs} pairs, widths {sorted(set(widths))}, |G 1 - W^T R| / |W^T R| = {err:.2e}")
    assert err < TOL


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_sampling_properties(proj, tmp_path, monkeypatch):
    from burgers_hip import pod
    X, centres, bases, Ug, runs, s = builder_case(proj)
    N, dt, E, _ = CASES["uniform-256"]
    rows, xi = s.rows.numpy(), s.xi.numpy()
    print(f"{proj}: {s.m} rows of {N}, training residual {s.residual:.2e} over {s.pairs} pairs")
    assert s.rows.dtype == torch.int32 and s.xi.dtype == torch.float64 and s.projection == proj.lower() and s.tau == TAU
    assert (xi >= 0.0).all() and np.isfinite(xi).all()
    assert np.all(np.diff(rows) > 0) and rows[0] == 0 and xi[0] == 1.0 and rows[-1] < N
    max_r, max_m, max_mg, max_c = pod.hyper_local_rom_limits()
    assert (max_r, max_m, max_mg, max_c) == (40, 256, 64, 64)
    assert MIN_ROWS <= s.m <= max_m == 256
    assert s.pairs == 3 * 20                                                # every 10th of 200 steps, three runs
    G, pairs = pod.local_row_sampling_system(X, centres, bases, Ug, hl.MG, runs, dt, proj.lower(), E, True, 10)
    d = G.sum(axis=1)
    res = np.linalg.norm(G[:, rows] @ xi - d) / np.linalg.norm(d)
    assert pairs == s.pairs and res <= TAU and abs(res - s.residual) <= 1e-12
    # save / load: bit-equal
    back = pod.load_row_sampling(pod.save_row_sampling(str(tmp_path), s))
    assert torch.equal(back.rows, s.rows) and torch.equal(back.xi, s.xi) and back.rows.dtype == torch.int32
    assert (back.projection, back.residual, back.pairs, back.tau) == (s.projection, s.residual, s.pairs, s.tau)
    # too few rows allowed: refused with a message that says so
    with pytest.raises(ValueError, match="max_rows"):
        pod.build_local_row_sampling(X, centres, bases, Ug, hl.MG, runs, dt, proj, E=E, max_rows=20)
    with pytest.raises(ValueError):
        pod.build_local_row_sampling(X, centres, bases, Ug, hl.MG, runs, dt, "galerkin-ish")
    with pytest.raises(ValueError):
        pod.build_local_row_sampling(X, centres, {c: b for c, b in bases.items() if c != 3}, Ug, hl.MG, runs, dt, proj)
    with pytest.raises(ValueError):
        pod.build_local_row_sampling(X, centres, bases, Ug[:-1], hl.MG, runs, dt, proj)
    with pytest.raises(ValueError):
        pod.build_local_row_sampling(X, centres, bases, Ug, hl.MG, runs, dt, proj, tau=0.0)
    # min_rows defaults to 3 x the widest basis, max_rows to the kernel's limit
    seen = {}
    monkeypatch.setattr(pod, "_fit_row_sampling", lambda G, pairs, projection, tau, min_rows, max_rows: seen.update(lo=min_rows, hi=max_rows))
    pod.build_local_row_sampling(X, centres, bases, Ug, hl.MG, runs, dt, proj, stride=100)
    assert seen == dict(lo=120, hi=256)
