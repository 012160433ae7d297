"""The offline side of the hyper-reduced POD-RBF PROM, without a GPU: pod.build_rbf_row_sampling (NNLS-sampled mesh rows and
weights on training pairs on the closure manifold), the host closure it evaluates, and the numpy restatement of the
weighted-row POD-RBF iteration (tests/hyper_rbf_ref.py), which with all rows and unit weights must be the oracle's
pod_rbf_prom, must not depend on the order of its sums in the cases the GPU tests use, and on the builder's sampling of the
committed closure must stay close to the oracle's full PROM."""
import functools

import numpy as np
import pytest
import torch

import hyper_rbf_ref as hrr
from conftest import rel_l2
from hyper_ref import training_runs
from loop_cases import TOL, built_library, draw

TAU = 1e-4
ONES = lambda N: np.ones(N)


@pytest.mark.parametrize("kernel", ["gaussian", "imq"])
def test_host_closure_is_the_oracle(kernel):
    """Value and Jacobian of pod._rbf_host_closure against oracle.burgers_ref.rbf_value / rbf_jacobian: 1e-13 (rel-L2) at the
    committed closure, the fixture's own point and 5 points of the training manifold; also with a degenerate range (the
    dx / dy floors), the points moved to the middle of that range so that they stay among the centres."""
    from burgers_hip import pod
    from oracle import burgers_ref as br
    X, dt, cl = hrr.committed(kernel)
    Up, Us, Xt, W, eps, x_min, x_max, y_min, y_max = cl
    S = training_runs(512, dt)[4][0]
    pts = np.concatenate([hrr.lc.golden()["qp_" + kernel][None], (Up.T @ S[:, 10::40]).T])
    for floors in (False, True):
        a, b, c, d = (v.copy() for v in (x_min, x_max, y_min, y_max))
        if floors:
            b[3] = a[3]; d[5] = c[5]
            pts[:, 3] = a[3] + 0.5                    # dx = 1 there: the scaled coordinate 0, among the centres
        value, jacobian = pod._rbf_host_closure(Xt, W, eps, a, b, c, d, kernel)
        V, J = value(pts), jacobian(pts)
        assert V.shape == (len(pts), 79) and J.shape == (len(pts), 79, 17)
        for k, q in enumerate(pts):
            ev = rel_l2(V[k], br.rbf_value(q, Xt, W, eps, kernel, a, b, c, d))
            ej = rel_l2(J[k], br.rbf_jacobian(q, Xt, W, eps, kernel, a, b, c, d))
            assert ev < 1e-13 and ej < 1e-13, (kernel, floors, k, ev, ej)
    with pytest.raises(ValueError):
        pod._rbf_host_closure(Xt, W, eps, x_min, x_max, y_min, y_max, "cubic")
    with pytest.raises(ValueError):
        pod._rbf_host_closure(Xt, W[:-1], eps, x_min, x_max, y_min, y_max, kernel)


@pytest.mark.parametrize("proj,kernel", [("Galerkin", "gaussian"), ("LSPG", "imq"), ("Galerkin", "imq"), ("LSPG", "gaussian")])
@pytest.mark.parametrize("case", sorted(hrr.CASES))
def test_restatement_with_all_rows_is_the_oracle(case, proj, kernel):
    """Also what lets the loop drop the re-projection: q_p <- q_p + dq without q_p = U_p^T U0 is the oracle's iteration for
    orthonormal [U_p U_s].  perturbed-96 is the graded, diffusive case (E = 0.01)."""
    from oracle import burgers_ref as br
    X, dt, E, cl = hrr.case_data(case, kernel)
    N = len(X)
    mu1, mu2 = draw(3)
    for s in range(3):
        U, ito = br.pod_rbf_prom(X, dt, 4, ONES(N), mu1[s], E, mu2[s], *cl, projection=proj, kernel=kernel, return_iters=True)
        Q, Qs, it = hrr.hyper_rbf_prom(X, dt, 4, ONES(N), mu1[s], E, mu2[s], *cl, proj, kernel, np.arange(N), ONES(N))
        err = rel_l2(hrr.decode(cl[0], cl[1], Q, Qs, ONES(N)), U)
        print(f"{case} {proj} {kernel} sample {s}: rel-L2 {err:.2e}, iterations {it.tolist()} / {ito.tolist()}")
        assert err < TOL
        assert np.array_equal(it, ito)
        assert np.array_equal(Q[:, 0], cl[0].T @ ONES(N))


def test_the_gpu_cases_do_not_depend_on_the_order_of_the_sums():
    """Every case the GPU tests use: the restatement's iteration counts are identical summing the rows forwards, backwards
    and with U_p, U_s, W perturbed by 1 + 4e-16 N(0, 1), and its trajectory moves by less than 1e-12.  That is what entitles
    the GPU tests to demand equal counts (the pattern of tests/test_rbf_long_rom_abi.py)."""
    built_library()
    worst = 0.0
    for name, X, dt, E, cl, proj, kernel, rows, xi, mus, steps in hrr.restatement_cases():
        N = len(X)
        for m1, m2 in zip(*mus):
            run = lambda c, **kw: hrr.hyper_rbf_prom(X, dt, steps, ONES(N), m1, E, m2, *c, proj, kernel, rows, xi, **kw)
            Q, Qs, it = run(cl)
            U = hrr.decode(cl[0], cl[1], Q, Qs, ONES(N))
            for label, (Q2, Qs2, it2) in (("backwards", run(cl, backwards=True)), ("perturbed", run(hrr.perturbed(cl)))):
                d = rel_l2(hrr.decode(cl[0], cl[1], Q2, Qs2, ONES(N)), U)
                worst = max(worst, d)
                print(f"{name} {proj} {kernel} mu = ({m1:.3f}, {m2:.4f}) {label}: spread {d:.1e}, iterations {it.tolist()} / {it2.tolist()}")
                assert np.array_equal(it, it2), (name, proj, label)
                assert d < 1e-12, (name, proj, label, d)
    print(f"largest spread {worst:.1e}")


@pytest.mark.parametrize("proj,kernel", [("Galerkin", "gaussian"), ("LSPG", "imq")])
def test_sampling_properties(proj, kernel, tmp_path):
    from burgers_hip import pod
    built_library()                                   # the builder asks the library for the kernel's row limit
    X, dt, cl = hrr.committed(kernel)
    Up = cl[0]
    N, n = Up.shape
    runs = training_runs(N, dt)
    s = hrr.committed_sampling(kernel, proj)
    rows, xi = s.rows.numpy(), s.xi.numpy()
    nodes = np.unique(np.clip(rows[:, None] + np.arange(-1, 2)[None, :], 0, N - 1))
    print(f"{proj} {kernel}: {s.m} rows of {N}, {len(nodes)} stencil nodes, training residual {s.residual:.2e} over {s.pairs} pairs")
    assert s.rows.dtype == torch.int32 and s.xi.dtype == torch.float64 and s.projection == proj.lower()
    assert (xi >= 0.0).all() and np.isfinite(xi).all()
    assert np.all(np.diff(rows) > 0) and rows[0] == 0 and xi[0] == 1.0 and rows[-1] < N
    limits = pod.hyper_rbf_rom_limits()
    assert limits == (20, 128, 65536, 256, 768)
    assert 200 <= s.m <= limits[3] and len(nodes) <= limits[4]             # min_rows defaults to min(200, N, max_rows)
    assert s.pairs == 9 * 20                                                # every 10th of 200 steps, nine runs
    # the training residual, recomputed here from the training matrix
    G, pairs = pod.rbf_row_sampling_system(X, *cl, kernel, runs, dt, proj.lower(), 0.0, True, 10)
    d = G.sum(axis=1)
    assert G.shape == (pairs * n, N) and pairs == s.pairs
    res = np.linalg.norm(G[:, rows] @ xi - d) / np.linalg.norm(d)
    assert res <= TAU and abs(res - s.residual) <= 1e-12
    # the same input twice gives the same output (tensors in)
    t = torch.as_tensor
    again = pod.build_rbf_row_sampling(t(X), t(cl[0]), t(cl[1]), t(cl[2]), t(cl[3]), cl[4], *(t(v) for v in cl[5:]),
                                       [(t(h), a, b) for h, a, b in runs], dt, proj, kernel=kernel, tau=TAU)
    assert torch.equal(again.rows, s.rows) and torch.equal(again.xi, s.xi) and again.residual == s.residual
    # a larger min_rows is honoured
    more = pod.build_rbf_row_sampling(X, *cl, runs, dt, proj, kernel=kernel, tau=TAU, min_rows=s.m + 5)
    assert more.m >= s.m + 5 and more.residual <= TAU
    # save / load: bit-equal
    back = pod.load_row_sampling(pod.save_row_sampling(str(tmp_path), s))
    assert torch.equal(back.rows, s.rows) and torch.equal(back.xi, s.xi) and back.rows.dtype == torch.int32
    assert (back.projection, back.residual, back.pairs, back.tau) == (s.projection, s.residual, s.pairs, s.tau)
    # too few rows allowed: refused with a message that says so
    with pytest.raises(ValueError, match="max_rows"):
        pod.build_rbf_row_sampling(X, *cl, runs, dt, proj, kernel=kernel, tau=TAU, max_rows=20)
    with pytest.raises(ValueError):
        pod.build_rbf_row_sampling(X, *cl, runs, dt, "galerkin-ish", kernel=kernel)
    with pytest.raises(ValueError):
        pod.build_rbf_row_sampling(X, cl[0][:-1], *cl[1:], runs, dt, proj, kernel=kernel)
    with pytest.raises(ValueError):
        pod.build_rbf_row_sampling(X, cl[0], cl[1], cl[2], cl[3][:-1], *cl[4:], runs, dt, proj, kernel=kernel)
    with pytest.raises(ValueError):
        pod.build_rbf_row_sampling(X, *cl, runs, dt, proj, kernel="cubic")


@functools.lru_cache(maxsize=None)
def sampled_against_oracle(kernel, proj, mu1, mu2, steps=8):
    """(rel-L2 of the sampled restatement against the oracle's full PROM, its counts, the oracle's) on the committed closure."""
    from oracle import burgers_ref as br
    built_library()
    X, dt, cl = hrr.committed(kernel)
    N = len(X)
    s = hrr.committed_sampling(kernel, proj)
    U, ito = br.pod_rbf_prom(X, dt, steps, ONES(N), mu1, 0.0, mu2, *cl, projection=proj, kernel=kernel, return_iters=True)
    Q, Qs, it = hrr.hyper_rbf_prom(X, dt, steps, ONES(N), mu1, 0.0, mu2, *cl, proj, kernel, s.rows.numpy(), s.xi.numpy())
    return rel_l2(hrr.decode(cl[0], cl[1], Q, Qs, ONES(N)), U), it, ito


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("kernel", ["gaussian", "imq"])
def test_sampled_restatement_against_the_full_prom(kernel, proj):
    """The builder's default sampling (200 rows) of the committed closure, 8 steps at two parameter points against the
    oracle's full PROM.  Bound 2e-3: about four times the largest value seen when the method was checked (5.5e-4).  No step
    may hit the cap where the full PROM does not.  Printed here (200 rows each): gaussian Galerkin 7.40e-6, 5.70e-6; gaussian
    LSPG 1.01e-4, 6.94e-5; imq Galerkin 2.05e-4, 8.73e-5; imq LSPG 5.47e-4, 3.82e-4; counts equal to the full PROM's but for
    one step of imq LSPG at (4.6, 0.021) (8 against 9)."""
    for mu1, mu2 in ((4.6, 0.021), (5.1, 0.024)):
        err, it, ito = sampled_against_oracle(kernel, proj, mu1, mu2)
        print(f"{kernel} {proj} mu = ({mu1}, {mu2}): m = {hrr.committed_sampling(kernel, proj).m}, rel-L2 {err:.2e}, "
              f"iterations {it.tolist()} / {ito.tolist()}")
        assert err < 2e-3
        assert not np.any((it >= 30) & (ito < 30))
