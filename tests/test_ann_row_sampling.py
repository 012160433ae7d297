"""The offline side of the hyper-reduced POD-ANN PROM, without a GPU: pod.build_ann_row_sampling (NNLS-sampled mesh rows and
weights on training pairs on the closure manifold) and the numpy restatement of the weighted-row POD-ANN iteration
(tests/hyper_ann_ref.py), which with all rows and unit weights must be the oracle's pod_ann_prom, and on the builder's
sampling of the committed closure must stay close to the oracle's full PROM."""
import numpy as np
import pytest
import torch

import ann_wide_cases as aw
import hyper_ann_ref as har
from conftest import rel_l2
from hyper_ref import training_runs
from loop_cases import TOL, built_library, draw

TAU = 1e-4


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", sorted(har.CASES))
def test_restatement_with_all_rows_is_the_oracle(case, proj):
    """Also what lets the loop drop the re-projection: q_p <- q_p + dq without q_p = U_p^T u^n is the oracle's iteration
    for orthonormal [U_p U_s]."""
    from oracle import burgers_ref as br
    N, dt, n, nbar, _, _, _, E, _ = har.CASES[case]
    X, Up, Us, model = har.case_data(case)
    Ws, bs = aw.weights(model)
    mu1, mu2 = draw(3)
    for s in range(3):
        U, ito = br.pod_ann_prom(X, dt, har.NT, np.ones(N), mu1[s], E, mu2[s], Up, Us, Ws, bs, projection=proj, return_iters=True)
        assert ito.max() < 50
        Q, Qs, it = har.hyper_ann_prom(X, dt, har.NT, np.ones(N), mu1[s], E, mu2[s], Up, Us, Ws, bs, proj, np.arange(N), np.ones(N))
        err = rel_l2(har.decode(Up, Us, Q, Qs, np.ones(N)), U)
        print(f"{case} {proj} sample {s}: rel-L2 {err:.2e}, iterations {it.tolist()} / {ito.tolist()}")
        assert err < TOL
        assert np.array_equal(it, ito)
        assert np.array_equal(Q[:, 0], Up.T @ np.ones(N))


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_sampling_properties(proj, tmp_path):
    from burgers_hip import pod
    built_library()                                   # the builder asks the library for the kernel's row limit
    X, Up, Us, model, _, _, dt = har.committed()
    N, n = Up.shape
    runs = training_runs(N, dt)
    s = har.committed_sampling(proj)
    rows, xi = s.rows.numpy(), s.xi.numpy()
    nodes = np.unique(np.clip(rows[:, None] + np.arange(-1, 2)[None, :], 0, N - 1))
    print(f"{proj}: {s.m} rows of {N}, {len(nodes)} stencil nodes, training residual {s.residual:.2e} over {s.pairs} pairs")
    assert s.rows.dtype == torch.int32 and s.xi.dtype == torch.float64 and s.projection == proj.lower()
    assert (xi >= 0.0).all() and np.isfinite(xi).all()
    assert np.all(np.diff(rows) > 0) and rows[0] == 0 and xi[0] == 1.0 and rows[-1] < N
    limits = pod.hyper_ann_rom_limits()
    assert 3 * n <= s.m <= limits[4] and len(nodes) <= limits[5]           # min_rows defaults to 3 n, max_rows to the kernel's
    assert s.pairs == 9 * 20                                                # every 10th of 200 steps, nine runs
    # the training residual, recomputed here from the training matrix
    G, pairs = pod.ann_row_sampling_system(X, Up, Us, model, runs, dt, proj.lower(), 0.0, True, 10)
    d = G.sum(axis=1)
    assert G.shape == (pairs * n, N) and pairs == s.pairs
    res = np.linalg.norm(G[:, rows] @ xi - d) / np.linalg.norm(d)
    assert res <= TAU and abs(res - s.residual) <= 1e-12
    # the same input twice gives the same output (tensors in)
    again = pod.build_ann_row_sampling(torch.as_tensor(X), torch.as_tensor(Up), torch.as_tensor(Us), model,
                                       [(torch.as_tensor(h), a, b) for h, a, b in runs], dt, proj, tau=TAU)
    assert torch.equal(again.rows, s.rows) and torch.equal(again.xi, s.xi) and again.residual == s.residual
    # a larger min_rows is honoured
    more = pod.build_ann_row_sampling(X, Up, Us, model, runs, dt, proj, tau=TAU, min_rows=s.m + 5)
    assert more.m >= s.m + 5 and more.residual <= TAU
    # save / load: bit-equal
    back = pod.load_row_sampling(pod.save_row_sampling(str(tmp_path), s))
    assert torch.equal(back.rows, s.rows) and torch.equal(back.xi, s.xi) and back.rows.dtype == torch.int32
    assert (back.projection, back.residual, back.pairs, back.tau) == (s.projection, s.residual, s.pairs, s.tau)
    # too few rows allowed: refused with a message that says so
    with pytest.raises(ValueError, match="max_rows"):
        pod.build_ann_row_sampling(X, Up, Us, model, runs, dt, proj, tau=TAU, max_rows=20)
    with pytest.raises(ValueError):
        pod.build_ann_row_sampling(X, Up, Us, model, runs, dt, "galerkin-ish")
    with pytest.raises(ValueError):
        pod.build_ann_row_sampling(X, Up[:-1], Us, model, runs, dt, proj)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_sampled_restatement_against_the_full_prom(proj):
    """The builder's sampling of the committed closure, with the default min_rows: 40 steps at two parameter points against the
    oracle's full PROM.  The bound 1e-2 is the PROM's own distance to the FOM (4.7e-2 / 5.2e-2) divided by five.  No step
    may hit the cap where the full PROM does not."""
    from oracle import burgers_ref as br
    built_library()
    X, Up, Us, _, Ws, bs, dt = har.committed()
    N = len(X)
    s = har.committed_sampling(proj)
    for mu1, mu2 in ((4.6, 0.021), (5.3, 0.017)):
        U, ito = br.pod_ann_prom(X, dt, 40, np.ones(N), mu1, 0.0, mu2, Up, Us, Ws, bs, projection=proj, return_iters=True)
        Q, Qs, it = har.hyper_ann_prom(X, dt, 40, np.ones(N), mu1, 0.0, mu2, Up, Us, Ws, bs, proj, s.rows.numpy(), s.xi.numpy())
        err = rel_l2(har.decode(Up, Us, Q, Qs, np.ones(N)), U)
        print(f"{proj} mu = ({mu1}, {mu2}): m = {s.m}, rel-L2 {err:.2e}, iterations {int(it.sum())} / {int(ito.sum())}")
        assert err < 1e-2
        assert not np.any((it >= 50) & (ito < 50))               # (LSPG: the first step hits the cap in both)
