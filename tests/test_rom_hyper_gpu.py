"""bg_hyper_rom_run: the hyper-reduced POD-PROM time loop on sampled mesh rows (csrc/rom_hyper.hip), against the oracle
(all rows, unit weights: the loop is then pod_prom_burgers itself) and against the numpy restatement of the weighted-row
iteration (tests/hyper_ref.py) on a mesh beyond every other ROM loop.
reference: FEMBurgers.pod_prom_burgers, FEM/fem_burgers.py:709-785.

Bases: the leading r left singular vectors of the FOM snapshots (oracle, C) of the 3 x 3 training grid, 200 steps."""
import functools

import numpy as np
import pytest
import torch

from conftest import mesh, rel_l2
from hyper_ref import hyper_prom, training_runs
from loop_cases import TOL, check_pod_vs_oracle, draw, pod_basis, same, to_np

pytestmark = pytest.mark.gpu
ENTRY = "bg_hyper_rom_run"
NT = 12


def all_rows(N, proj):
    from burgers_hip import pod
    return pod.RowSampling(np.arange(N, dtype=np.int32), np.ones(N), proj.lower(), 0.0, 0, 0.0)


# N = 96 on the perturbed mesh with diffusion (m = 96: three slabs of 32 rows, every branch of the non-uniform assembly) and
# N = 256 at the widest basis and the largest row count the kernel takes (eight slabs).  The oracle converges at both
# (at most 8 iterations of 20), which check_pod_vs_oracle's flag test asserts through the equal counts.
FULL = {"perturbed": (96, 0.2, 17, 0.01, 7), "widest": (256, 0.05, 40, 0.0, None)}


@functools.lru_cache(maxsize=None)
def full_run(case, proj, options=0):
    from burgers_hip import rom
    N, dt, r, E, seed = FULL[case]
    X, Phi = pod_basis(N, dt, r, E=E, seed=seed)
    mu1, mu2 = draw(4)
    res = rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, NT, Phi, all_rows(N, proj), rom.PROJ[proj.lower()], E=E, options=options)
    torch.cuda.synchronize()
    return res, (X, Phi, mu1, mu2, dt, E)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", sorted(FULL))
def test_all_rows_with_unit_weights_is_the_oracle(hip, case, proj):
    from burgers_hip import lib
    res, (X, Phi, mu1, mu2, dt, E) = full_run(case, proj)
    N, r = Phi.shape
    assert res.path == ENTRY and res.plan.m == N and tuple(res.q.shape) == (4, NT + 1, r)
    assert lib.mesh_is_uniform(X) == (case == "widest")
    if case == "widest":
        assert (r, N) == lib.limits("bg_hyper_rom_limits", 2)               # both limits at once
    assert np.array_equal(to_np(res.hist[:, 0]), np.ones((4, N)))           # column 0 is u0 itself
    assert rel_l2(to_np(res.q[:, 0]), np.broadcast_to(Phi.T @ np.ones(N), (4, r))) < 1e-14      # row 0 of q is Phi^T u0
    check_pod_vs_oracle(res, X, dt, NT, mu1, mu2, Phi, proj, E=E)
    assert tuple(res.snapshots().shape) == (4, N, NT + 1)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_forced_pivoting_gives_the_same_result(hip, proj):
    from burgers_hip import lib
    res, (X, Phi, mu1, mu2, dt, E) = full_run("perturbed", proj)
    piv, _ = full_run("perturbed", proj, lib.BG_OPT_FORCE_PIVOTED)
    check_pod_vs_oracle(piv, X, dt, NT, mu1, mu2, Phi, proj, E=E)
    worst = max(rel_l2(a, b) for a, b in zip(to_np(piv.hist), to_np(res.hist)))
    print(f"{proj}: forced pivoting against the fast kernel, worst rel-L2 {worst:.2e}")
    assert worst < TOL and torch.equal(piv.iters, res.iters)


# ---- sampled rows on N = 2049: beyond every other ROM loop ---------------------------------------------------------------------
LN, LDT, LR = 2049, 0.0125, 40


@functools.lru_cache(maxsize=None)
def sampled_case(proj):
    """(X, Phi, sampling): build_row_sampling's rows (three training runs, every 20th step, tau = 1e-3: 120 rows) plus rows added
    by hand with a small weight, so that 0, 1, N - 2, N - 1, an adjacent pair (700, 701) and an isolated row (1500) are
    present and m is odd."""
    from burgers_hip import pod
    X, Phi = pod_basis(LN, LDT, LR)
    s = pod.build_row_sampling(X, Phi, training_runs(LN, LDT, keep=[0, 4, 8]), LDT, proj, tau=1e-3, stride=20)
    w = dict(zip(s.rows.tolist(), s.xi.tolist()))
    for extra in (0, 1, LN - 2, LN - 1, 700, 701, 1500):
        w.setdefault(extra, 0.05)
    if len(w) % 2 == 0:
        w.setdefault(1300, 0.05)
    rows = np.array(sorted(w), dtype=np.int32)
    assert len(rows) % 2 == 1 and len(rows) <= pod.hyper_rom_limits()[1]
    for need in (0, 1, LN - 2, LN - 1, 700, 701, 1500):
        assert need in w
    assert 1499 not in w and 1501 not in w
    return X, Phi, pod.RowSampling(rows, np.array([w[int(i)] for i in rows]), proj.lower(), s.residual, s.pairs, s.tau)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_sampled_rows_against_the_restatement(hip, proj):
    """The gate is max(TOL, 10 d), d the restatement's own spread between summing the rows forwards and backwards (the
    reference's sensitivity to the order of the sum; the kernel's order is a third one).  No iteration count may differ."""
    from burgers_hip import rom
    X, Phi, s = sampled_case(proj)
    B = 3
    mu1, mu2 = draw(B, seed=11)
    res = rom.pod_prom_run_hyper(X, np.ones(LN), mu1, mu2, LDT, NT, Phi, s, rom.PROJ[proj.lower()])
    torch.cuda.synchronize()
    assert res.path == ENTRY and res.plan.m == s.m and not bool(res.flags.any()) and bool((res.info == 0).all())
    q, iters = to_np(res.q), to_np(res.iters)
    for b in range(B):
        Q, it = hyper_prom(X, LDT, NT, np.ones(LN), mu1[b], 0.0, mu2[b], Phi, proj, s.rows.numpy(), s.xi.numpy())
        Qb, itb = hyper_prom(X, LDT, NT, np.ones(LN), mu1[b], 0.0, mu2[b], Phi, proj, s.rows.numpy(), s.xi.numpy(), backwards=True)
        assert it.max() < 20 and itb.max() < 20                              # the restatement converges
        d = rel_l2(Phi @ Qb[:, 1:], Phi @ Q[:, 1:])
        err = rel_l2(to_np(res.hist[b]).T[:, 1:], Phi @ Q[:, 1:])
        print(f"N={LN} r={LR} m={s.m} {proj} sample {b}: d {d:.2e}, rel-L2 {err:.2e}, iterations {iters[b].tolist()} / {it.tolist()}")
        assert err < max(TOL, 10.0 * d), (proj, b, err, d)
        assert rel_l2(q[b].T, Q) < max(TOL, 10.0 * d)
        assert np.array_equal(iters[b], it), (proj, b)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_rows_left_out_of_the_perturbed_mesh(hip, proj):
    """The perturbed mesh of FULL with rows 10, 50, 51 and 70 left out (m = 92, three slabs, unit weights): from row 11 on
    the sampled-row index j and the mesh row i differ, so the kernel's view of the stencil coordinates as x[i-1], x[i], x[i+1]
    (mass row and assembly of the shared row routines) is wrong by a whole node if its offset is, and a forcing load taken at
    j instead of i is another node's; with all rows sampled i == j hides both.
    The gate is test_sampled_rows_against_the_restatement's.  On the CPU the restatement converges in at most 7 of 20
    iterations in all four runs and d is 3e-16 .. 5e-16, so the gate is TOL."""
    from burgers_hip import pod, rom
    N, dt, r, E, seed = FULL["perturbed"]
    X, Phi = pod_basis(N, dt, r, E=E, seed=seed)
    rows = np.setdiff1d(np.arange(N), [10, 50, 51, 70]).astype(np.int32)
    xi = np.ones(len(rows))
    assert len(rows) == 92
    B = 2
    mu1, mu2 = draw(B)
    res = rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, NT, Phi, pod.RowSampling(rows, xi, proj.lower(), 0.0, 0, 0.0),
                                 rom.PROJ[proj.lower()], E=E)
    torch.cuda.synchronize()
    assert res.path == ENTRY and res.plan.m == 92 and not bool(res.flags.any()) and bool((res.info == 0).all())
    q, iters = to_np(res.q), to_np(res.iters)
    for b in range(B):
        Q, it = hyper_prom(X, dt, NT, np.ones(N), mu1[b], E, mu2[b], Phi, proj, rows, xi)
        Qb, itb = hyper_prom(X, dt, NT, np.ones(N), mu1[b], E, mu2[b], Phi, proj, rows, xi, backwards=True)
        assert it.max() < 20 and itb.max() < 20                              # the restatement converges
        d = rel_l2(Phi @ Qb[:, 1:], Phi @ Q[:, 1:])
        err = rel_l2(to_np(res.hist[b]).T[:, 1:], Phi @ Q[:, 1:])
        print(f"N={N} r={r} m=92 {proj} sample {b}: d {d:.2e}, rel-L2 {err:.2e}, iterations {iters[b].tolist()} / {it.tolist()}")
        assert err < max(TOL, 10.0 * d), (proj, b, err, d)
        assert rel_l2(q[b].T, Q) < max(TOL, 10.0 * d)
        assert np.array_equal(iters[b], it), (proj, b)


# ---- limit shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_one_mode(hip, proj):
    from burgers_hip import rom
    N, dt = 96, 0.2
    X, Phi = pod_basis(N, dt, 1)
    mu1, mu2 = draw(2)
    res = rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, 8, Phi, all_rows(N, proj), rom.PROJ[proj.lower()])
    torch.cuda.synchronize()
    check_pod_vs_oracle(res, X, dt, 8, mu1, mu2, Phi, proj)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_as_many_rows_as_modes(hip, proj):
    """r = 17 on m = 17 evenly spread rows.  The iteration does not converge on so few rows (the restatement reaches max_it
    as well), so what is compared is three steps of ONE iteration each, against the restatement under the same cap; the
    gate is test_sampled_rows_against_the_restatement's (d is 4e-11 .. 2e-10 here: the 17 x 17 systems are ill-conditioned)."""
    from burgers_hip import lib, pod, rom
    N, dt, r = 96, 0.2, 17
    X, Phi = pod_basis(N, dt, r)
    rows = np.unique(np.round(np.linspace(0, N - 1, r)).astype(np.int32))
    xi = np.full(r, N / r)
    xi[0] = 1.0
    assert len(rows) == r
    s = pod.RowSampling(rows, xi, proj.lower(), 0.0, 0, 0.0)
    mu1, mu2 = draw(2)
    res = rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, 3, Phi, s, rom.PROJ[proj.lower()], max_it=1)
    torch.cuda.synchronize()
    assert bool((res.info == 0).all()) and bool((res.flags == lib.BG_FLAG_HIT_CAP).all()) and bool((res.iters == 1).all())
    for b in range(2):
        Q, _ = hyper_prom(X, dt, 3, np.ones(N), mu1[b], 0.0, mu2[b], Phi, proj, rows, xi, max_it=1)
        Qb, _ = hyper_prom(X, dt, 3, np.ones(N), mu1[b], 0.0, mu2[b], Phi, proj, rows, xi, max_it=1, backwards=True)
        d, err = rel_l2(Qb[:, 1:], Q[:, 1:]), rel_l2(to_np(res.q[b]).T[:, 1:], Q[:, 1:])
        print(f"m = r = {r} {proj} sample {b}: d {d:.2e}, rel-L2 of q {err:.2e}")
        assert err < max(TOL, 10.0 * d)


def test_row_zero_alone_reports_a_singular_system(hip):
    """m = 1 with only the Dirichlet row: Ar = Phi[0]^T Phi[0] has rank one.  With a basis whose row 0 has a single non-zero
    entry the second pivot is exactly zero, which is what ``info`` reports (np.linalg.solve raises there); nothing faults."""
    from burgers_hip import pod, rom
    N, dt, r = 96, 0.2, 5
    X, Phi = pod_basis(N, dt, r)
    Phi = Phi.copy()
    Phi[0, 1:] = 0.0
    s = pod.RowSampling(np.zeros(1, dtype=np.int32), np.ones(1), "galerkin", 0.0, 0, 0.0)
    mu1, mu2 = draw(3)
    res = rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, 4, Phi, s, rom.PROJ["galerkin"])
    torch.cuda.synchronize()
    assert res.info.tolist() == [2, 2, 2]
    with pytest.raises(rom.SingularReducedSystem):
        rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, 4, Phi, projection="Galerkin", hyper=s)


def test_order_entries_outside_the_batch_are_skipped(hip):
    from burgers_hip import lib, rom
    proj = "LSPG"
    ref, (X, Phi, mu1, mu2, dt, E) = full_run("perturbed", proj)
    plan, B, N, dev = ref.plan, 4, len(X), ref.q.device
    u0d = torch.ones((B, N), dtype=torch.float64, device=dev)
    q0, u0s = (u0d @ plan.Phi).contiguous(), (u0d[:, plan.stencil] * plan.inside).contiguous()
    mu1d, mu2d = torch.as_tensor(mu1, device=dev), torch.as_tensor(mu2, device=dev)
    qh = torch.full((B, NT + 1, plan.r), -7.0, dtype=torch.float64, device=dev)
    iters = torch.zeros((B, NT), dtype=torch.int32, device=dev)
    flags = torch.full((B,), -3, dtype=torch.int32, device=dev)
    info = torch.zeros((B,), dtype=torch.int32, device=dev)
    order = torch.tensor([2, -1, 0, B + 5], dtype=torch.int32, device=dev)
    rc = lib.load().bg_hyper_rom_run(N, B, plan.r, plan.m, NT, rom.PROJ["lspg"], lib.ptr(plan.rows), lib.ptr(plan.xi), lib.ptr(plan.xs),
                                     lib.ptr(plan.PhiS), lib.ptr(q0), lib.ptr(u0s), lib.ptr(mu1d), lib.ptr(mu2d), dt, E, 1e-6, 20,
                                     lib.mesh_options(X, supg=True), lib.ptr(qh), lib.ptr(iters), lib.ptr(flags), lib.ptr(info),
                                     lib.ptr(order), lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    keep = [0, 2]
    assert torch.equal(qh[keep], ref.q[keep]) and torch.equal(iters[keep], ref.iters[keep])
    assert torch.equal(flags[keep], ref.flags[keep]) and bool((info == 0).all())
    assert bool((qh[[1, 3]] == -7.0).all()) and bool((flags[[1, 3]] == -3).all())


def test_plan_reuse_refusals_and_the_empty_batch(hip, monkeypatch):
    from burgers_hip import pod, rom
    first, (X, Phi, mu1, mu2, dt, E) = full_run("perturbed", "Galerkin")
    N = len(X)
    p = rom.PROJ["galerkin"]
    again = rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, NT, None, first.plan, p, E=E)
    torch.cuda.synchronize()
    assert again.plan is first.plan and again.path == ENTRY
    same(again, first)
    assert torch.equal(again.q, first.q)
    empty = rom.pod_prom_run_hyper(X, np.ones(N), np.zeros(0), np.zeros(0), dt, 2, None, first.plan, p, E=E)
    torch.cuda.synchronize()
    assert tuple(empty.q.shape) == (0, 3, first.plan.r) and tuple(empty.hist.shape) == (0, 3, N)

    def no_launch(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(rom, "_device_loop", no_launch)
    dev = first.q.device
    with pytest.raises(ValueError, match="projection"):
        rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, 2, None, first.plan, rom.PROJ["lspg"], E=E)      # trained for the other one
    with pytest.raises(ValueError):
        rom.pod_prom_run_hyper(mesh(N)[0], np.ones(N), mu1, mu2, dt, 2, None, first.plan, p)                 # a plan for another mesh
    with pytest.raises(ValueError):
        rom.pod_prom_run_hyper(mesh(N + 1)[0], np.ones(N + 1), mu1, mu2, dt, 2, None, first.plan, p)
    rs = lambda rows, xi: pod.RowSampling(np.array(rows, dtype=np.int32), np.array(xi, dtype=np.float64), "galerkin", 0.0, 0, 0.0)
    for bad in (rs([0, 5, 5], [1, 1, 1]), rs([0, 7, 3], [1, 1, 1]), rs([0, N], [1, 1]), rs([-1, 3], [1, 1]), rs([0, 3], [1, -0.5]),
                rs([0, 3], [1, np.nan]), rs([], []), rs([0, 3], [1])):
        with pytest.raises(ValueError):
            rom.HyperPodPlan(Phi, bad, X, dev)
    with pytest.raises(ValueError):
        rom.HyperPodPlan(Phi, pod.RowSampling(np.arange(N, dtype=np.int32), np.ones(N), "petrov", 0.0, 0, 0.0), X, dev)      # an unknown projection
    with pytest.raises(ValueError):
        rom.HyperPodPlan(np.concatenate([Phi] * 3, axis=1)[:, :41], all_rows(N, "Galerkin"), X, dev)        # one column too many
    X3, _ = mesh(300)
    with pytest.raises(ValueError):
        rom.HyperPodPlan(np.zeros((300, 4)), all_rows(300, "Galerkin"), X3, dev)                              # more rows than the kernel holds


def test_facade_opt_in_and_unchanged_default(hip):
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    X, Phi, s = sampled_case("LSPG")
    _, T = mesh(LN)
    U = FEMBurgers(X, T).pod_prom_burgers(LDT, 6, np.ones(LN), 4.8, 0.0, 0.021, Phi, projection="LSPG", hyper=s)
    res = rom.pod_prom_run_hyper(X, np.ones(LN), [4.8], [0.021], LDT, 6, Phi, s, rom.PROJ["lspg"])
    torch.cuda.synchronize()
    assert np.asarray(U).shape == (LN, 7) and np.array_equal(np.asarray(U), to_np(res.hist[0]).T)
    with pytest.raises(ValueError):
        FEMBurgers(X, T).pod_prom_burgers(LDT, 2, np.ones(LN), 4.8, 0.0, 0.021, Phi, projection="Galerkin", hyper=s)
    # without ``hyper`` the call takes the route it took before, bit for bit
    N, dt = 96, 0.2
    Xs, Phis = pod_basis(N, dt, 17)
    mu1, mu2 = draw(3)
    default = rom.pod_prom_run(Xs, np.ones(N), mu1, mu2, dt, 4, Phis, projection="LSPG")
    direct = rom.pod_prom_run_fused(Xs, np.ones(N), mu1, mu2, dt, 4, Phis, rom.PROJ["lspg"])
    torch.cuda.synchronize()
    assert default.path == "bg_rom_run"
    same(default, direct)
    Uf = FEMBurgers(Xs, mesh(N)[1]).pod_prom_burgers(dt, 4, np.ones(N), mu1, 0.0, mu2, Phis, projection="LSPG")
    assert np.array_equal(np.asarray(Uf), to_np(default.hist).transpose(0, 2, 1))
    long_default = rom.pod_prom_run(X, np.ones(LN), [4.8], [0.021], LDT, 1, Phi, projection="LSPG")
    assert long_default.path == "library"
