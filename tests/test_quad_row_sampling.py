"""The offline side of the hyper-reduced quadratic-manifold PROM, without a GPU: pod.build_quad_row_sampling (NNLS-sampled
mesh rows and weights on training pairs on the manifold) and the numpy restatement of the weighted-row, carried-q iteration
(tests/hyper_quad_ref.py), which with all rows and unit weights must be the oracle's pod_quadratic_manifold, and on the
builder's default sampling must stay close to the oracle's full PROM."""
import numpy as np
import pytest
import torch

import hyper_quad_ref as hq
from conftest import rel_l2
from hyper_ref import training_runs
from loop_cases import TOL, built_library, draw

TAU = 1e-5                     # the builder's default


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", sorted(hq.CASES))
def test_restatement_with_all_rows_is_the_oracle(case, proj):
    """Also what lets the loop drop the re-projection: q <- q + dq without q = Phi^T u^n is the oracle's iteration, because
    Phi^T H = 0 for a manifold fitted on the residual of the projection (measured here: below 1e-11)."""
    from oracle import burgers_ref as br
    N, dt, n, E, _ = hq.CASES[case]
    X, Phi, H = hq.case_data(case)
    assert np.abs(Phi.T @ H).max() < 1e-11
    mu1, mu2 = draw(3)
    for s in range(3):
        U, ito = br.pod_quadratic_manifold(X, dt, hq.NT, np.ones(N), mu1[s], E, mu2[s], Phi, H, projection=proj, return_iters=True)
        assert ito.max() < hq.CAP                       # a condition on the input: no step of the oracle's hits the cap
        Q, it = hq.hyper_quad_prom(X, dt, hq.NT, np.ones(N), mu1[s], E, mu2[s], Phi, H, proj, np.arange(N), np.ones(N))
        err = rel_l2(hq.decode(Phi, H, Q, np.ones(N)), U)
        print(f"{case} {proj} sample {s}: rel-L2 {err:.2e}, iterations {it.tolist()} / {ito.tolist()}")
        assert err < TOL
        assert np.array_equal(it, ito)
        assert np.array_equal(Q[:, 0], Phi.T @ np.ones(N))


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_sampling_properties(proj, tmp_path):
    from burgers_hip import pod
    built_library()                                   # the builder asks the library for the kernel's row limit
    case = "full-256"
    N, dt, n, E, _ = hq.CASES[case]
    X, Phi, H = hq.case_data(case)
    runs = training_runs(N, dt, E)
    s = hq.builder_sampling(case, proj)
    rows, xi = s.rows.numpy(), s.xi.numpy()
    nodes = np.unique(np.clip(rows[:, None] + np.arange(-1, 2)[None, :], 0, N - 1))
    print(f"{proj}: {s.m} rows of {N}, {len(nodes)} stencil nodes, training residual {s.residual:.2e} over {s.pairs} pairs")
    assert s.rows.dtype == torch.int32 and s.xi.dtype == torch.float64 and s.projection == proj.lower() and s.tau == TAU
    assert (xi >= 0.0).all() and np.isfinite(xi).all()
    assert np.all(np.diff(rows) > 0) and rows[0] == 0 and xi[0] == 1.0 and rows[-1] < N
    max_n, max_m, max_nodes = pod.hyper_quad_rom_limits()
    assert 3 * n <= s.m <= max_m and len(nodes) <= max_nodes                # min_rows defaults to 3 n, max_rows to the kernel's
    assert s.pairs == 9 * 20                                                # every 10th of 200 steps, nine runs
    # the training residual, recomputed here from the training matrix
    G, pairs = pod.quad_row_sampling_system(X, Phi, H, runs, dt, proj.lower(), E, 10)
    d = G.sum(axis=1)
    assert G.shape == (pairs * n, N) and pairs == s.pairs
    res = np.linalg.norm(G[:, rows] @ xi - d) / np.linalg.norm(d)
    assert res <= TAU and abs(res - s.residual) <= 1e-12
    # the same input twice gives the same output (tensors in)
    again = pod.build_quad_row_sampling(torch.as_tensor(X), torch.as_tensor(Phi), torch.as_tensor(H),
                                        [(torch.as_tensor(h), a, b) for h, a, b in runs], dt, proj, E=E)
    assert torch.equal(again.rows, s.rows) and torch.equal(again.xi, s.xi) and again.residual == s.residual
    # a larger min_rows is honoured
    more = pod.build_quad_row_sampling(X, Phi, H, runs, dt, proj, E=E, min_rows=s.m + 5)
    assert more.m >= s.m + 5 and more.residual <= TAU
    # save / load: bit-equal
    back = pod.load_row_sampling(pod.save_row_sampling(str(tmp_path), s))
    assert torch.equal(back.rows, s.rows) and torch.equal(back.xi, s.xi) and back.rows.dtype == torch.int32
    assert (back.projection, back.residual, back.pairs, back.tau) == (s.projection, s.residual, s.pairs, s.tau)
    # too few rows allowed: refused with a message that says so
    with pytest.raises(ValueError, match="max_rows"):
        pod.build_quad_row_sampling(X, Phi, H, runs, dt, proj, E=E, max_rows=20)
    with pytest.raises(ValueError):
        pod.build_quad_row_sampling(X, Phi, H, runs, dt, "galerkin-ish")
    with pytest.raises(ValueError):
        pod.build_quad_row_sampling(X, Phi[:-1], H, runs, dt, proj)
    with pytest.raises(ValueError):
        pod.build_quad_row_sampling(X, Phi, H[:, :-1], runs, dt, proj)
    with pytest.raises(ValueError):
        pod.build_quad_row_sampling(X, Phi, H, runs, dt, proj, tau=0.0)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_sampled_restatement_against_the_full_prom(proj):
    """The builder's default sampling (tau = 1e-5, min_rows = 3 n = 120) at N = 1024, n = 40, dt = 0.0125: 8 steps at two
    parameter points against the oracle's full PROM.  The bound 2.4e-3 is one fifth of this PROM's own rel-L2 distance to the
    FOM at those points over those steps, measured with the oracle on the CPU: 1.21e-2 and 1.32e-2 (Galerkin), 1.23e-2 and
    1.36e-2 (LSPG); the smallest of them is taken.  Measured: 3.5e-11 / 5.9e-11 (Galerkin, 120 rows, 147 stencil nodes) and
    6.7e-12 / 1.6e-11 (LSPG, 120 rows, 150 nodes) -- on this mesh the training matrix has numerical rank 110, so 120 rows fit
    it exactly.  No step may hit the cap where the full PROM does not; here every count equals the full PROM's."""
    from oracle import burgers_ref as br
    built_library()
    N, dt, _, E, _ = hq.MID
    X, Phi, H = hq.case_data(hq.MID)
    s = hq.builder_sampling(hq.MID, proj)
    for mu1, mu2 in ((4.6, 0.021), (5.3, 0.017)):
        U, ito = br.pod_quadratic_manifold(X, dt, 8, np.ones(N), mu1, E, mu2, Phi, H, projection=proj, return_iters=True)
        Q, it = hq.hyper_quad_prom(X, dt, 8, np.ones(N), mu1, E, mu2, Phi, H, proj, s.rows.numpy(), s.xi.numpy())
        err = rel_l2(hq.decode(Phi, H, Q, np.ones(N)), U)
        print(f"{proj} mu = ({mu1}, {mu2}): m = {s.m}, rel-L2 {err:.2e}, iterations {it.tolist()} / {ito.tolist()}")
        assert err < 1.21e-2 / 5.0
        assert not np.any((it >= hq.CAP) & (ito < hq.CAP))
