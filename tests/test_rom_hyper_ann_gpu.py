"""bg_hyper_ann_rom_run: the hyper-reduced POD-ANN PROM time loop on sampled mesh rows (csrc/rom_hyper_ann.hip), against the
oracle (all rows, unit weights: the loop is then pod_ann_prom itself), against the numpy restatement of the weighted-row
iteration (tests/hyper_ann_ref.py) on a mesh beyond every other POD-ANN loop, and against bg_ann_rom_run on the committed
closure.  reference: FEMBurgers.pod_ann_prom, FEM/fem_burgers.py:1177-1251.

The closure and its Jacobian are float32 in the reference, the oracle and the kernel, so every comparison of a trajectory
is float32-limited: TOL32 = 5e-6 on the decoded history, iteration counts within 1 (the gate of tests/test_ann_fused_gpu.py).
A differently rounded float32 evaluation of the closure moves these trajectories by 2e-9 .. 3e-9 on the CPU."""
import functools

import numpy as np
import pytest
import torch

import ann_wide_cases as aw
import hyper_ann_ref as har
from conftest import mesh, rel_l2
from hyper_ref import training_runs
from loop_cases import draw, to_np

pytestmark = pytest.mark.gpu
ENTRY, NT, TOL32 = har.ENTRY, har.NT, aw.TOL32


def sampling(rows, xi, proj):
    from burgers_hip import pod
    return pod.RowSampling(np.asarray(rows, dtype=np.int32), np.asarray(xi, dtype=np.float64), proj.lower(), 0.0, 0, 0.0)


def run(case, s, proj, mu1, mu2, nT=NT, **kw):
    from burgers_hip import rom
    N, dt, _, _, _, _, _, E, _ = har.CASES[case] if isinstance(case, str) else case
    X, Up, Us, model = har.case_data(case)
    res = rom.pod_ann_run_hyper(X, np.ones(N), mu1, mu2, dt, nT, Up, Us, model, s, rom.PROJ[proj.lower()], E=E, **kw)
    torch.cuda.synchronize()
    return res


def check_against_restatement(res, case, s, proj, mu1, mu2, nT=NT, converges=True):
    """Every sample: rel-L2 of the decoded history against the restatement's below TOL32, q and q_s likewise, counts within 1.
    ``converges``: the restatement stays below the cap in every step, and so does the loop (no flag).  Otherwise the
    comparison ends with the last step before the restatement first hits the cap, summing the rows forwards or backwards:
    an iteration that does not converge wanders, and from there on the restatement's own spread between the two orders of
    the sum (1e-7 .. 1e-2 in these cases, where a converged step has 1e-16) is beyond any gate."""
    from burgers_hip import lib
    N, dt, _, _, _, _, _, E, _ = har.CASES[case] if isinstance(case, str) else case
    X, Up, Us, model = har.case_data(case)
    Ws, bs = aw.weights(model)
    assert res.path == ENTRY and res.plan.m == s.m and bool((res.info == 0).all())
    assert not bool((res.flags & ~lib.BG_FLAG_HIT_CAP).any())
    hist, q, qs, iters = to_np(res.hist), to_np(res.q), to_np(res.q_s), to_np(res.iters)
    for b in range(len(mu1)):
        Q, Qs, it = har.hyper_ann_prom(X, dt, nT, np.ones(N), mu1[b], E, mu2[b], Up, Us, Ws, bs, proj, s.rows.numpy(), s.xi.numpy())
        good = nT
        if converges:
            assert it.max() < 50 and int(res.flags[b]) == 0
        else:
            itb = har.hyper_ann_prom(X, dt, nT, np.ones(N), mu1[b], E, mu2[b], Up, Us, Ws, bs, proj, s.rows.numpy(), s.xi.numpy(),
                                     backwards=True)[2]
            capped = np.flatnonzero((it >= 50) | (itb >= 50))
            good = int(capped[0]) if len(capped) else nT
            assert good >= 1                                                  # something is compared
        c = slice(0, good + 1)
        err = rel_l2(hist[b].T[:, c], har.decode(Up, Us, Q, Qs, np.ones(N))[:, c])
        print(f"N={N} m={s.m} nodes={res.plan.n_nodes} {proj} sample {b}: {good} steps, rel-L2 {err:.2e}, q {rel_l2(q[b].T[:, c], Q[:, c]):.2e}, "
              f"iterations {iters[b].tolist()} / {it.tolist()}")
        assert err < TOL32, (proj, b, err)
        assert rel_l2(q[b].T[:, c], Q[:, c]) < TOL32 and rel_l2(qs[b].T[:, c], Qs[:, c]) < TOL32
        assert np.abs(iters[b, :good] - it[:good]).max() <= 1, (proj, b)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", sorted(har.CASES))
def test_all_rows_with_unit_weights_is_the_oracle(hip, case, proj):
    """full-256: m = N = 256, the row limit, a uniform mesh read as a non-uniform one.  perturbed-96: a non-uniform mesh with
    diffusion and n = 8."""
    from burgers_hip import lib
    from oracle import burgers_ref as br
    N, dt, n, nbar, _, _, _, E, _ = har.CASES[case]
    X, Up, Us, model = har.case_data(case)
    Ws, bs = aw.weights(model)
    mu1, mu2 = draw(3)
    res = run(case, sampling(np.arange(N), np.ones(N), proj), proj, mu1, mu2)
    assert res.path == ENTRY and res.plan.m == N and res.plan.n_nodes == N
    assert tuple(res.q.shape) == (3, NT + 1, n) and tuple(res.q_s.shape) == (3, NT + 1, nbar)
    assert lib.mesh_is_uniform(X) == (case == "full-256")
    if case == "full-256":
        assert N == lib.limits("bg_hyper_ann_rom_limits", 6)[4]
    hist, iters = to_np(res.hist), to_np(res.iters)
    assert np.array_equal(hist[:, 0], np.ones((3, N)))                      # column 0 is u0 itself
    assert rel_l2(to_np(res.q[:, 0]), np.broadcast_to(Up.T @ np.ones(N), (3, n))) < 1e-14
    assert not bool(res.flags.any()) and bool((res.info == 0).all())
    for s in range(3):
        U, ito = br.pod_ann_prom(X, dt, NT, np.ones(N), mu1[s], E, mu2[s], Up, Us, Ws, bs, projection=proj, return_iters=True)
        err = rel_l2(hist[s].T, U)
        print(f"{case} {proj} sample {s}: rel-L2 {err:.2e}, iterations {iters[s].tolist()} / {ito.tolist()}")
        assert err < TOL32, (case, proj, s, err)
        assert np.abs(iters[s] - ito).max() <= 1
    assert tuple(res.snapshots().shape) == (3, N, NT + 1)


# ---- sampled rows on N = 2049: beyond every other POD-ANN loop -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_sampling(kind, proj):
    """"built": build_ann_row_sampling's rows (training runs 0, 4, 8, every 10th step, min_rows = 120) plus rows added by hand
    with a small weight, so that 0, 1, N - 2, N - 1, an adjacent pair (700, 701) and an isolated row (1500) are present.
    "limits": rows 0, 8, ..., 2040 with weight 8 (row 0: 1): m = 256 and 767 table nodes, both limits at once."""
    from burgers_hip import pod
    N, dt = har.LONG[0], har.LONG[1]
    if kind == "limits":
        rows = np.arange(0, N - 1, 8)
        xi = np.full(len(rows), 8.0); xi[0] = 1.0
        assert len(rows) == 256
        return sampling(rows, xi, proj)
    X, Up, Us, model = har.case_data(har.LONG)
    s = pod.build_ann_row_sampling(X, Up, Us, model, training_runs(N, dt, keep=[0, 4, 8]), dt, proj, stride=10, min_rows=120)
    w = dict(zip(s.rows.tolist(), s.xi.tolist()))
    for extra in (0, 1, N - 2, N - 1, 700, 701, 1500):
        w.setdefault(extra, 0.05)
    rows = np.array(sorted(w), dtype=np.int32)
    assert len(rows) <= pod.hyper_ann_rom_limits()[4]
    return sampling(rows, [w[int(i)] for i in rows], proj)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("kind", ["built", "limits"])
def test_sampled_rows_against_the_restatement(hip, kind, proj):
    from burgers_hip import lib
    s = long_sampling(kind, proj)
    mu1, mu2 = draw(2, seed=11)
    res = run(har.LONG, s, proj, mu1, mu2)
    if kind == "limits":
        assert (res.plan.m, res.plan.n_nodes + 1) == lib.limits("bg_hyper_ann_rom_limits", 6)[4:]      # 256 rows, 767 nodes
    check_against_restatement(res, har.LONG, s, proj, mu1, mu2)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_rows_left_out_of_the_perturbed_mesh(hip, proj):
    """perturbed-96 with rows 10, 50, 51 and 70 left out, unit weights: every node stays in the table, but from row 11 on a
    row that is only a neighbour sits between sampled ones -- it must assemble as nothing (weight 0, not the Dirichlet or
    the last row), and with row 10 gone the table position of a sampled row and its index among the sampled rows differ,
    which all-rows runs hide.
    With these rows gone this closure's iteration often fails to converge, in the restatement as in the loop (the oracle's
    all-rows run needs up to 17 iterations already).  The samples are two of draw(10) at which the LSPG restatement converges
    in all six steps (at most 9 iterations); under Galerkin it hits the cap in step 2 / 3 at every one of the ten, so there
    the comparison covers the first step / the first two (check_against_restatement says why it ends there)."""
    N = har.CASES["perturbed-96"][0]
    rows = np.setdiff1d(np.arange(N), [10, 50, 51, 70])
    s = sampling(rows, np.ones(len(rows)), proj)
    mu1, mu2 = (v[[4, 5]] for v in draw(10))
    res = run("perturbed-96", s, proj, mu1, mu2)
    assert res.plan.m == 92 and res.plan.n_nodes == N
    check_against_restatement(res, "perturbed-96", s, proj, mu1, mu2, converges=False)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_committed_closure_against_the_full_loop(hip, proj):
    """N = 512, the builder's sampling: the hyper-reduced loop against bg_ann_rom_run on the same batch.  The error is at
    most twice the CPU restatement's error against the oracle for the same sampling and samples."""
    from burgers_hip import rom
    from oracle import burgers_ref as br
    X, Up, Us, model, Ws, bs, dt = har.committed()
    s = har.committed_sampling(proj)
    B, nT = 4, 12
    mu1, mu2 = draw(B)
    p = rom.PROJ[proj.lower()]
    hyp = rom.pod_ann_run_hyper(X, np.ones(512), mu1, mu2, dt, nT, Up, Us, model, s, p)
    full = rom.pod_ann_run_fused(X, np.ones(512), mu1, mu2, dt, nT, Up, Us, model, p)
    torch.cuda.synchronize()
    assert hyp.path == ENTRY and full.path == "bg_ann_rom_run" and bool((hyp.info == 0).all())
    hh, fh = to_np(hyp.hist), to_np(full.hist)
    for b in range(B):
        U = br.pod_ann_prom(X, dt, nT, np.ones(512), mu1[b], 0.0, mu2[b], Up, Us, Ws, bs, projection=proj)
        Q, Qs, _ = har.hyper_ann_prom(X, dt, nT, np.ones(512), mu1[b], 0.0, mu2[b], Up, Us, Ws, bs, proj, s.rows.numpy(), s.xi.numpy())
        cpu = rel_l2(har.decode(Up, Us, Q, Qs, np.ones(512)), U)
        err = rel_l2(hh[b].T, fh[b].T)
        print(f"{proj} sample {b}: m = {s.m}, nodes = {hyp.plan.n_nodes}, rel-L2 {err:.2e} (restatement against the oracle: {cpu:.2e})")
        assert err <= 2.0 * cpu, (proj, b, err, cpu)


def test_a_trajectory_does_not_depend_on_the_batch(hip):
    """Alone, in a permuted batch, and in a batch larger than the grid: bit-identical."""
    case, proj = "perturbed-96", "LSPG"
    N = har.CASES[case][0]
    rows = np.setdiff1d(np.arange(N), [10, 50, 51, 70])
    s = sampling(rows, np.ones(len(rows)), proj)
    B = 520
    mu1, mu2 = draw(B)
    big = run(case, s, proj, mu1, mu2)
    assert B > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    perm = np.random.default_rng(2).permutation(B)
    shuffled = run(case, big.plan, proj, mu1[perm], mu2[perm])
    assert shuffled.plan is big.plan
    for k in ("q", "q_s", "iters", "flags", "info"):
        assert torch.equal(getattr(shuffled, k), getattr(big, k)[torch.as_tensor(perm, device=big.q.device)]), k
    for b in (0, 7, B - 1):
        alone = run(case, big.plan, proj, mu1[b:b + 1], mu2[b:b + 1])
        for k in ("q", "q_s", "iters", "flags", "info"):
            assert torch.equal(getattr(alone, k)[0], getattr(big, k)[b]), (k, b)
    unbalanced = run(case, big.plan, proj, mu1, mu2, balance=False)
    assert torch.equal(unbalanced.q, big.q) and torch.equal(unbalanced.iters, big.iters)


def test_the_cap_is_flagged(hip):
    from burgers_hip import lib
    N = har.CASES["perturbed-96"][0]
    mu1, mu2 = draw(3)
    res = run("perturbed-96", sampling(np.arange(N), np.ones(N), "LSPG"), "LSPG", mu1, mu2, max_it=2)
    assert bool((res.iters == 2).all()) and bool(((res.flags & lib.BG_FLAG_HIT_CAP) != 0).all())


def test_routing_is_opt_in(hip):
    """pod_ann_run(hyper=) and the facade reach the new entry; a sampling trained for the other projection, another mesh
    and a float64 closure are refused."""
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    case = "perturbed-96"
    N, dt, _, _, _, _, _, E, _ = har.CASES[case]
    X, Up, Us, model = har.case_data(case)
    s = sampling(np.arange(N), np.ones(N), "Galerkin")
    mu1, mu2 = draw(2)
    direct = run(case, s, "Galerkin", mu1, mu2)
    res = rom.pod_ann_run(X, np.ones(N), mu1, mu2, dt, NT, Up, Us, model, projection="Galerkin", E=E, hyper=s)
    assert res.path == ENTRY and torch.equal(res.q, direct.q) and torch.equal(res.hist, direct.hist)
    again = rom.pod_ann_run(X, np.ones(N), mu1, mu2, dt, NT, None, None, None, projection="Galerkin", E=E, hyper=res.plan)
    assert again.plan is res.plan and torch.equal(again.q, direct.q)
    T = mesh(N)[1]
    U = FEMBurgers(X, T).pod_ann_prom(dt, NT, np.ones(N), mu1[0], E, mu2[0], Up, Us, model, projection="Galerkin", hyper=s)
    assert np.array_equal(U, to_np(direct.hist[0]).T)
    with pytest.raises(ValueError):
        rom.pod_ann_run(X, np.ones(N), mu1, mu2, dt, NT, Up, Us, model, projection="LSPG", E=E, hyper=s)
    with pytest.raises(ValueError):
        rom.pod_ann_run(X, np.ones(N), mu1, mu2, dt, NT, Up, Us, model, projection="Galerkin", E=E, hyper=s, ann_dtype=torch.float64)
    X2 = X.copy(); X2[5] += 1e-3
    with pytest.raises(ValueError):
        rom.pod_ann_run_hyper(X2, np.ones(N), mu1, mu2, dt, NT, Up, Us, model, res.plan, rom.PROJ["galerkin"], E=E)
    # without hyper= nothing routes here
    assert rom.pod_ann_run(X, np.ones(N), mu1, mu2, dt, 2, Up, Us, model, projection="Galerkin", E=E).path == "bg_ann_rom_run"
