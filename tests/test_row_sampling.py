"""The offline side of the hyper-reduced POD PROM, without a GPU: pod.build_row_sampling (NNLS-sampled mesh rows and
weights) and the numpy restatement of the weighted-row iteration (tests/hyper_ref.py), which with all rows and unit weights
must be the oracle's pod_prom_burgers."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from hyper_ref import hyper_prom, training_runs
from loop_cases import TOL, built_library, pod_basis

N, R, DT, TAU = 96, 17, 0.2, 1e-4


@pytest.fixture(scope="module")
def case():
    built_library()                                   # the builder asks the library for the kernel's row limit
    X, Phi = pod_basis(N, DT, R)
    return X, Phi, training_runs(N, DT)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_sampling_properties(case, proj, tmp_path):
    from burgers_hip import pod
    X, Phi, runs = case
    s = pod.build_row_sampling(X, Phi, runs, DT, proj, tau=TAU)
    rows, xi = s.rows.numpy(), s.xi.numpy()
    print(f"{proj}: {s.m} rows of {N}, training residual {s.residual:.2e} over {s.pairs} pairs")
    assert s.rows.dtype == torch.int32 and s.xi.dtype == torch.float64 and s.projection == proj.lower()
    assert (xi >= 0.0).all() and np.isfinite(xi).all()
    assert np.all(np.diff(rows) > 0) and rows[0] == 0 and xi[0] == 1.0 and rows[-1] < N
    assert s.m >= 3 * R and s.m <= pod.hyper_rom_limits()[1]               # min_rows defaults to 3 r
    assert s.pairs == 9 * 20                                                # every 10th of 200 steps, nine runs
    # the training residual, recomputed here from the training matrix
    G, pairs = pod.row_sampling_system(X, Phi, runs, DT, proj.lower(), 0.0, True, 10)
    d = G.sum(axis=1)
    assert G.shape == (pairs * R, N)
    res = np.linalg.norm(G[:, rows] @ xi - d) / np.linalg.norm(d)
    assert res <= TAU and abs(res - s.residual) <= 1e-12
    # the same input twice gives the same output
    again = pod.build_row_sampling(X, Phi, runs, DT, proj, tau=TAU)
    assert torch.equal(again.rows, s.rows) and torch.equal(again.xi, s.xi) and again.residual == s.residual
    # tensors in, and a larger min_rows is honoured
    more = pod.build_row_sampling(torch.as_tensor(X), torch.as_tensor(Phi), [(torch.as_tensor(h), a, b) for h, a, b in runs], DT,
                                  proj, tau=TAU, min_rows=s.m + 5)
    assert more.m >= s.m + 5 and more.residual <= TAU
    # save / load: bit-equal
    back = pod.load_row_sampling(pod.save_row_sampling(str(tmp_path), s))
    assert torch.equal(back.rows, s.rows) and torch.equal(back.xi, s.xi) and back.rows.dtype == torch.int32
    assert (back.projection, back.residual, back.pairs, back.tau) == (s.projection, s.residual, s.pairs, s.tau)
    # too few rows allowed: refused with a message that says so
    with pytest.raises(ValueError, match="max_rows"):
        pod.build_row_sampling(X, Phi, runs, DT, proj, tau=TAU, max_rows=20)
    with pytest.raises(ValueError):
        pod.build_row_sampling(X, Phi, runs, DT, "galerkin-ish")
    with pytest.raises(ValueError):
        pod.build_row_sampling(X, Phi[:-1], runs, DT, proj)


def test_training_assembly_is_the_oracles(case):
    """pod.picard_rows (the closed forms the builder trains on) against the oracle's assembly of the same state."""
    from burgers_hip import pod
    from oracle import burgers_ref as br
    X, Phi, runs = case
    hist, mu1, mu2 = runs[4]
    Un, U0 = Phi @ (Phi.T @ hist[:, 30]), Phi @ (Phi.T @ hist[:, 31])
    for E in (0.0, 0.01):
        lo, di, up, Rr = pod.picard_rows(X, U0, Un, mu1, mu2, DT, E, True)
        M3, K3 = br.mass_tridiag(X), br.diffusion_tridiag(X)
        lo_o, di_o, up_o = br.system_tridiag(M3, K3, br.convection_tridiag(X, U0), DT, E)
        b = br.tridiag_matvec(*M3, Un) + DT * br.forcing_vector(X, mu2) - DT * br.supg_term(X, U0, mu2)
        b[0] = mu1
        Ro = br.tridiag_matvec(lo_o, di_o, up_o, U0) - b
        for mine, theirs in ((lo, lo_o), (di, di_o), (up, up_o)):
            assert np.abs(mine - theirs).max() <= 1e-13 * np.abs(di_o).max()
        assert np.abs(Rr - Ro).max() <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("n,r,dt,nT", [(96, 17, 0.2, 12), (256, 17, 0.05, 40)])
def test_restatement_with_all_rows_is_the_oracle(n, r, dt, nT, proj):
    from oracle import burgers_ref as br
    X, Phi = pod_basis(n, dt, r)
    mu1, mu2 = 4.6, 0.021
    U, ito = br.pod_prom_burgers(X, dt, nT, np.ones(n), mu1, 0.0, mu2, Phi, projection=proj, return_iters=True)
    assert ito.max() < 20
    Q, it = hyper_prom(X, dt, nT, np.ones(n), mu1, 0.0, mu2, Phi, proj, np.arange(n), np.ones(n))
    err = rel_l2(Phi @ Q[:, 1:], U[:, 1:])
    print(f"N={n} r={r} {proj}: rel-L2 {err:.2e}, iterations {it.tolist()} / {ito.tolist()}")
    assert err < TOL
    assert np.array_equal(it, ito)
    assert np.array_equal(Q[:, 0], Phi.T @ np.ones(n))
