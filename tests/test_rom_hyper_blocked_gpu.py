"""bg_hyper_rom_run_blocked: the hyper-reduced POD-PROM time loop for 97 to 256 modes on up to 1024 sampled mesh rows
(csrc/rom_hyper_blocked.hip), against the oracle (all rows, unit weights: the loop is then pod_prom_burgers itself) and against
the numpy restatement of the weighted-row iteration (tests/hyper_ref.py), with the redo of the samples the guarded pivot-free
blocked elimination hands back.  reference: FEMBurgers.pod_prom_burgers, FEM/fem_burgers.py:709-785.

Bases: the leading r left singular vectors of the FOM snapshots (oracle, C) of the 3 x 3 training grid, 200 steps.  The gates
are the project's: rel-L2 below TOL = 1e-10 with identical iteration counts against the oracle, max(TOL, 10 d) for weighted
rows, d the restatement's forward/backward summation spread (tests/test_rom_hyper_wide_pivot_gpu.py)."""
import functools

import numpy as np
import pytest
import torch

from conftest import mesh, rel_l2
from hyper_ref import hyper_prom, training_runs
from loop_cases import TOL, check_pod_vs_oracle, draw, pod_basis, to_np

pytestmark = pytest.mark.gpu
ENTRY = "bg_hyper_rom_run_blocked"
NT, B_FULL = 6, 3


def sampling(rows, xi, proj):
    from burgers_hip import pod
    return pod.RowSampling(np.asarray(rows, dtype=np.int32), np.asarray(xi, dtype=np.float64), proj.lower(), 0.0, 0, 0.0)


def unit_rows(N, proj):
    return sampling(np.arange(N), np.ones(N), proj)


# ---- all rows, unit weights: the full PROM ---------------------------------------------------------------------------------------
# (N, dt, r, E, mesh seed).  "one_column": r = 97, one live column in the last 16-column tile, m = 160.  "whole_tiles": r = 160,
# ten whole tiles, m = 300 = 37 slabs of 8 and 4 rows.  "full_width": r = 256 on m = 600 rows, beyond the wide loop's 512; two
# sweeps for Galerkin (272 items).  "perturbed": r = 113 on the perturbed mesh with diffusion, every branch of the non-uniform
# assembly.  The oracle converges in 8 .. 18 iterations per step at all four and its largest unpivoted multiplier is
# 0.18 .. 0.72, which check_pod_vs_oracle's flag test and ``redone == 0`` assert.
FULL = {"one_column": (160, 0.2, 97, 0.0, None), "whole_tiles": (300, 0.08, 160, 0.0, None), "full_width": (600, 0.04, 256, 0.0, None),
        "perturbed": (200, 0.16, 113, 0.01, 7)}


@functools.lru_cache(maxsize=None)
def full_run(case, proj, options=0):
    from burgers_hip import rom
    N, dt, r, E, seed = FULL[case]
    X, Phi = pod_basis(N, dt, r, E=E, seed=seed)
    mu1, mu2 = draw(B_FULL)
    res = rom.pod_prom_run_hyper_blocked(X, np.ones(N), mu1, mu2, dt, NT, Phi, unit_rows(N, proj), rom.PROJ[proj.lower()], E=E,
                                         options=options)
    torch.cuda.synchronize()
    return res, (X, Phi, mu1, mu2, dt, E)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", sorted(FULL))
def test_all_rows_with_unit_weights_is_the_oracle(hip, case, proj):
    from burgers_hip import lib, rom
    res, (X, Phi, mu1, mu2, dt, E) = full_run(case, proj)
    N, r = Phi.shape
    assert res.path == ENTRY and isinstance(res.plan, rom.HyperBlockedPodPlan) and res.plan.m == N and res.redone == 0
    assert tuple(res.q.shape) == (B_FULL, NT + 1, r) and tuple(res.plan.PhiS.shape) == ((N + 7) // 8 * 8, 3, (r + 15) // 16 * 16)
    assert lib.mesh_is_uniform(X) == (case != "perturbed")
    assert np.array_equal(to_np(res.hist[:, 0]), np.ones((B_FULL, N)))      # column 0 is u0 itself
    assert rel_l2(to_np(res.q[:, 0]), np.broadcast_to(Phi.T @ np.ones(N), (B_FULL, r))) < 1e-14      # row 0 of q is Phi^T u0
    check_pod_vs_oracle(res, X, dt, NT, mu1, mu2, Phi, proj, E=E)
    assert tuple(res.snapshots().shape) == (B_FULL, N, NT + 1)


def test_at_the_row_limit(hip):
    """As many sampled rows as the kernel holds, read from the library: every per-row array of the kernel is full."""
    from burgers_hip import lib, rom
    _, N = lib.limits("bg_hyper_rom_blocked_limits", 2)
    dt, r = 25.6 / N, 97
    X, Phi = pod_basis(N, dt, r)
    mu1, mu2 = draw(B_FULL)
    res = rom.pod_prom_run_hyper_blocked(X, np.ones(N), mu1, mu2, dt, NT, Phi, unit_rows(N, "LSPG"), rom.PROJ["lspg"])
    torch.cuda.synchronize()
    assert res.path == ENTRY and res.plan.m == N and res.redone == 0
    check_pod_vs_oracle(res, X, dt, NT, mu1, mu2, Phi, "LSPG")


# ---- a genuine hand-back -----------------------------------------------------------------------------------------------------------
# N = 300, dt = 0.08, r = 113: rows = unique([0] + choice(300, 260)) from default_rng(1), m = 261 (a ragged last slab: 5 of 8
# rows), weights 10 ** uniform(-2, 2) from the same generator after the rows (as weighted_rows of
# tests/test_rom_hyper_wide_pivot_gpu.py).  The restatement converges in at most 13 iterations, d <= 3e-14, and its unpivoted
# elimination meets multipliers of 1.83 .. 1.84 (Galerkin) and 2.72 (LSPG): the guard trips and both samples are redone.
@functools.lru_cache(maxsize=None)
def weighted_rows():
    rng = np.random.default_rng(1)
    rows = np.unique(np.concatenate([[0], rng.choice(300, 260, replace=False)]))
    xi = 10.0 ** rng.uniform(-2, 2, len(rows))
    assert len(rows) == 261
    return rows, xi


def restatement(X, dt, nT, mu1, mu2, E, Phi, proj, rows, xi):
    """(Q, iters, d, worst) as in tests/test_rom_hyper_wide_pivot_gpu.py: hyper_prom with the rows summed forwards; d, its rel-L2
    spread against the sum backwards; worst, the largest sub-diagonal multiplier of the unpivoted elimination over the forward
    run's systems.  Both runs must converge."""
    N = len(X)
    worst = 0.0
    real = np.linalg.solve

    def wrapped(A, b):
        nonlocal worst
        W = np.array(A, dtype=np.float64)
        for k in range(len(W) - 1):
            m = W[k + 1:, k] / W[k, k]
            worst = max(worst, float(np.abs(m).max()))
            W[k + 1:] -= np.outer(m, W[k])
        return real(A, b)
    np.linalg.solve = wrapped
    try:
        Q, it = hyper_prom(X, dt, nT, np.ones(N), mu1, E, mu2, Phi, proj, rows, xi)
    finally:
        np.linalg.solve = real
    Qb, itb = hyper_prom(X, dt, nT, np.ones(N), mu1, E, mu2, Phi, proj, rows, xi, backwards=True)
    assert it.max() < 20 and itb.max() < 20
    return Q, it, rel_l2(Phi @ Qb[:, 1:], Phi @ Q[:, 1:]), worst


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_marked_samples_are_redone_and_agree_with_the_restatement(hip, proj):
    from burgers_hip import rom
    N, dt, r, nT = 300, 0.08, 113, 4
    X, Phi = pod_basis(N, dt, r)
    rows, xi = weighted_rows()
    mu1, mu2 = draw(2)
    res = rom.pod_prom_run_hyper_blocked(X, np.ones(N), mu1, mu2, dt, nT, Phi, sampling(rows, xi, proj), rom.PROJ[proj.lower()])
    torch.cuda.synchronize()
    assert res.path == ENTRY and res.plan.m == 261 and res.plan.m % 8 == 5
    assert not bool(res.flags.any()) and bool((res.info == 0).all())
    q, iters = to_np(res.q), to_np(res.iters)
    for b in range(2):
        Q, it, d, worst = restatement(X, dt, nT, mu1[b], mu2[b], 0.0, Phi, proj, rows, xi)
        err = rel_l2(to_np(res.hist[b]).T[:, 1:], Phi @ Q[:, 1:])
        print(f"N={N} r={r} m=261 {proj} sample {b}: d {d:.2e}, rel-L2 {err:.2e}, multiplier {worst:.3f}, iterations {iters[b].tolist()} / {it.tolist()}")
        assert worst >= 1.01, (proj, b, worst)
        assert err < max(TOL, 10.0 * d), (proj, b, err, d)
        assert rel_l2(q[b].T, Q) < max(TOL, 10.0 * d)
        assert np.array_equal(iters[b], it), (proj, b)
    assert res.redone == 2


# ---- a fitted sampling on a mesh beyond every full POD loop ---------------------------------------------------------------------------
# N = 2049, dt = 0.0125, r = 97: build_row_sampling on three training runs, every 20th step, tau = 1e-3, filled to 200 rows (the
# "n2049" case of tests/test_rom_hyper_wide_gpu.py with one more mode, the narrowest basis only this loop takes).  Behind the
# first row left out the sampled-row index and the mesh row differ, and the weights are the NNLS's.  Whether the guard trips is
# the restatement's to say: ``redone`` is all of the batch when its own unpivoted elimination meets a multiplier of at least
# 1.01 and none of it at or below 0.99 (inputs in between, or on both sides, would test rounding and are refused).
@functools.lru_cache(maxsize=None)
def sampled_case(proj):
    from burgers_hip import pod
    N, dt, r = 2049, 0.0125, 97
    X, Phi = pod_basis(N, dt, r)
    return X, Phi, pod.build_row_sampling(X, Phi, training_runs(N, dt, keep=[0, 4, 8]), dt, proj, tau=1e-3, stride=20, min_rows=200)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_sampled_rows_above_1024_nodes_against_the_restatement(hip, proj):
    from burgers_hip import rom
    X, Phi, s = sampled_case(proj)
    N, dt, nT, B = len(X), 0.0125, NT, 2
    assert s.m == 200
    mu1, mu2 = draw(B, seed=11)
    res = rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, nT, Phi, proj, hyper=s, blocked=True)      # routed by width and the opt-in
    torch.cuda.synchronize()
    assert res.path == ENTRY and res.plan.m == 200 and not bool(res.flags.any()) and bool((res.info == 0).all())
    rows, xi = s.rows.numpy(), s.xi.numpy()
    q, iters, worsts = to_np(res.q), to_np(res.iters), []
    for b in range(B):
        Q, it, d, worst = restatement(X, dt, nT, mu1[b], mu2[b], 0.0, Phi, proj, rows, xi)
        err = rel_l2(to_np(res.hist[b]).T[:, 1:], Phi @ Q[:, 1:])
        print(f"N={N} r=97 m=200 {proj} sample {b}: d {d:.2e}, rel-L2 {err:.2e}, multiplier {worst:.3f}, iterations {iters[b].tolist()} / {it.tolist()}")
        assert err < max(TOL, 10.0 * d), (proj, b, err, d)
        assert rel_l2(q[b].T, Q) < max(TOL, 10.0 * d)
        assert np.array_equal(iters[b], it), (proj, b)
        worsts.append(worst)
    assert not any(0.99 < w < 1.01 for w in worsts), worsts
    assert all(w >= 1.01 for w in worsts) or all(w <= 0.99 for w in worsts), worsts
    assert res.redone == (B if max(worsts) >= 1.01 else 0), (res.redone, worsts)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_forced_pivoting_redoes_every_sample_and_agrees(hip, proj):
    from burgers_hip import lib
    res, _ = full_run("whole_tiles", proj)
    piv, _ = full_run("whole_tiles", proj, lib.BG_OPT_FORCE_PIVOTED)
    assert piv.redone == B_FULL and res.redone == 0 and bool((piv.info == 0).all()) and piv.path == ENTRY
    assert not bool(piv.flags.any()) and torch.equal(piv.iters, res.iters)
    worst = max(rel_l2(a, b) for a, b in zip(to_np(piv.hist), to_np(res.hist)))
    print(f"{proj}: every sample redone by the weighted-row library iteration against the device loop, worst rel-L2 {worst:.2e}")
    assert worst < 1e-11


# ---- more samples than workgroups, one slot reused, the raw ABI ------------------------------------------------------------------
def test_batch_behaviour_on_two_slots(hip):
    from burgers_hip import lib, rom
    N, dt, r, E, _ = FULL["one_column"]
    X, Phi = pod_basis(N, dt, r)
    B = 5
    mu1, mu2 = draw(B, seed=9)
    p = rom.PROJ["lspg"]
    dev = torch.device("cuda", torch.cuda.current_device())
    plan = rom.HyperBlockedPodPlan(Phi, unit_rows(N, "LSPG"), X, dev, slots=2)
    assert plan.slots == 2 and tuple(plan.work.shape) == (2, 112 * 128)
    run = lambda u0, m1, m2, nT, **kw: rom.pod_prom_run_hyper_blocked(X, u0, m1, m2, dt, nT, None, plan, p, **kw)
    ref = run(np.ones(N), mu1, mu2, NT)
    flat = run(np.ones(N), mu1, mu2, NT, balance=False)
    one = run(np.ones(N), mu1[4:], mu2[4:], NT)
    torch.cuda.synchronize()
    assert ref.plan is plan and ref.path == ENTRY and ref.redone == 0 and not bool(ref.flags.any()) and bool((ref.info == 0).all())
    for k in ("q", "iters", "flags", "info"):
        assert torch.equal(getattr(flat, k), getattr(ref, k)), k                  # the order of the slots is scheduling only
        assert torch.equal(getattr(one, k)[0], getattr(ref, k)[4]), k             # sample 4 alone, in a slot others used before
    # A run in two halves.  The first half is the run in one, bit for bit.  The second cannot be through the public wrapper: the
    # restart is not the loop's own state.  It starts from the decoded u = Phi q, re-projects it (q0 = Phi^T Phi q: q up to the
    # rounding of two products of length N = 160 and r = 97, about (N + r) eps |q| = 6e-14 |q| at worst) and assembles its first
    # iteration at u itself where the run in one lifts PhiS q (the same sums in another order, again a few eps).  With equal
    # iteration counts the four remaining steps are one smooth map of that start, and an implicit step of this convection
    # problem does not amplify a perturbation of its start by more than a small factor.  The gate is 1e-12, sixteen times the
    # worst-case 6e-14, on every later snapshot, with identical iteration counts: looser than equal bits, a hundred times
    # tighter than the project's TOL.
    head = run(np.ones(N), mu1, mu2, 2)
    tail = run(to_np(head.hist[:, -1]), mu1, mu2, NT - 2)
    torch.cuda.synchronize()
    assert torch.equal(head.q, ref.q[:, :3]) and torch.equal(head.iters, ref.iters[:, :2])
    assert torch.equal(tail.iters, ref.iters[:, 2:])
    worst = max(rel_l2(a, b) for a, b in zip(to_np(tail.hist[:, 1:]), to_np(ref.hist[:, 3:])))
    print(f"the second half restarted from the decoded state against the run in one, worst rel-L2 {worst:.2e}")
    assert worst < 1e-12
    # two entries of order outside [0, B): their samples keep what the caller put there
    u0d = torch.ones((B, N), dtype=torch.float64, device=dev)
    q0, u0s = (u0d @ plan.Phi).contiguous(), (u0d[:, plan.stencil] * plan.inside).contiguous()
    mu1d, mu2d = torch.as_tensor(mu1, device=dev), torch.as_tensor(mu2, device=dev)
    qh = torch.full((B, NT + 1, r), -7.0, dtype=torch.float64, device=dev)
    iters = torch.zeros((B, NT), dtype=torch.int32, device=dev)
    flags = torch.full((B,), -3, dtype=torch.int32, device=dev)
    info = torch.zeros((B,), dtype=torch.int32, device=dev)
    order = torch.arange(B, dtype=torch.int32, device=dev)
    order[1], order[3] = -1, B + 5
    rc = lib.load().bg_hyper_rom_run_blocked(N, B, r, plan.m, NT, p, lib.ptr(plan.rows), lib.ptr(plan.xi), lib.ptr(plan.xs),
                                             lib.ptr(plan.PhiS), lib.ptr(q0), lib.ptr(u0s), lib.ptr(mu1d), lib.ptr(mu2d), dt, E, 1e-6, 20,
                                             lib.mesh_options(X, supg=True), lib.ptr(plan.work), plan.slots, lib.ptr(qh),
                                             lib.ptr(iters), lib.ptr(flags), lib.ptr(info), lib.ptr(order), lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    keep = [0, 2, 4]
    assert torch.equal(qh[keep], ref.q[keep]) and torch.equal(iters[keep], ref.iters[keep])
    assert torch.equal(flags[keep], ref.flags[keep]) and bool((info == 0).all())
    assert bool((qh[[1, 3]] == -7.0).all()) and bool((flags[[1, 3]] == -3).all()) and bool((iters[[1, 3]] == 0).all())


# ---- an exactly singular reduced system --------------------------------------------------------------------------------------------
def test_zero_mode_is_reported_as_singular(hip):
    from burgers_hip import rom
    N, dt, r, _, _ = FULL["one_column"]
    X, Phi = pod_basis(N, dt, r)
    Phi = Phi.copy()
    Phi[:, 50] = 0.0                                     # row and column 50 of every Galerkin system are exactly zero
    mu1, mu2 = draw(B_FULL)
    res = rom.pod_prom_run_hyper_blocked(X, np.ones(N), mu1, mu2, dt, 3, Phi, unit_rows(N, "Galerkin"), rom.PROJ["galerkin"])
    torch.cuda.synchronize()
    assert res.redone == 0 and to_np(res.info).tolist() == [51] * B_FULL
    with pytest.raises(rom.SingularReducedSystem):
        rom.check_singular(res)


# ---- routing and refusals ----------------------------------------------------------------------------------------------------------
def test_routing_is_opt_in_and_refusals_come_before_launch(hip, monkeypatch):
    from burgers_hip import lib, rom
    from fem_burgers import FEMBurgers
    N, dt, r, _, _ = FULL["one_column"]
    X, Phi = pod_basis(N, dt, r)
    _, T = mesh(N)
    s = unit_rows(N, "LSPG")
    p = rom.PROJ["lspg"]
    dev = torch.device("cuda", torch.cuda.current_device())
    U = FEMBurgers(X, T).pod_prom_burgers(dt, 4, np.ones(N), 4.8, 0.0, 0.021, Phi, projection="LSPG", hyper=s, blocked=True)
    res = rom.pod_prom_run_hyper_blocked(X, np.ones(N), [4.8], [0.021], dt, 4, Phi, s, p)
    by_plan = rom.pod_prom_run_hyper(X, np.ones(N), [4.8], [0.021], dt, 4, None, res.plan, p)      # the plan picks the loop
    torch.cuda.synchronize()
    assert res.path == ENTRY and np.asarray(U).shape == (N, 5) and np.array_equal(np.asarray(U), to_np(res.hist[0]).T)
    assert by_plan.path == ENTRY and by_plan.plan is res.plan and torch.equal(by_plan.q, res.q)
    small = rom.pod_prom_run(X, np.ones(N), [4.8], [0.021], dt, 2, Phi[:, :64], "LSPG", hyper=s, blocked=True)
    assert small.path == "bg_hyper_rom_run_wide"                                   # blocked changes nothing for a basis the wide loop takes
    mu1, mu2 = draw(2)

    def no_launch(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(rom, "_device_loop", no_launch)
    with pytest.raises(ValueError):                                                # without blocked=True: refused as before
        FEMBurgers(X, T).pod_prom_burgers(dt, 2, np.ones(N), 4.8, 0.0, 0.021, Phi, projection="LSPG", hyper=s)
    with pytest.raises(ValueError):
        rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, 2, Phi, s, p)
    with pytest.raises(ValueError):                                                # there is no repair kernel
        rom.pod_prom_run_hyper_blocked(X, np.ones(N), mu1, mu2, dt, 2, None, res.plan, p, pivot="device")
    with pytest.raises(ValueError):
        rom.pod_prom_run(X, np.ones(N), mu1, mu2, dt, 2, Phi, "LSPG", hyper=s, blocked=True, pivot="device")
    with pytest.raises(ValueError):
        rom.pod_prom_run_hyper_blocked(X, np.ones(N), mu1, mu2, dt, 2, None, res.plan, p, pivot="both")
    wide = rom.HyperWidePodPlan(Phi[:, :64], s, X, dev)
    narrow = rom.HyperPodPlan(Phi[:, :17], s, X, dev)
    for other in (wide, narrow):                                                   # the other loops' plans
        with pytest.raises(ValueError):
            rom.pod_prom_run_hyper_blocked(X, np.ones(N), mu1, mu2, dt, 2, None, other, p)
    with pytest.raises(ValueError):                                                # and this loop's plan with them
        rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, 2, None, res.plan, p)
    with pytest.raises(ValueError, match="projection"):                            # trained for the other projection
        rom.pod_prom_run_hyper_blocked(X, np.ones(N), mu1, mu2, dt, 2, None, res.plan, rom.PROJ["galerkin"])
    Xn = X.copy(); Xn[5] += 0.1
    with pytest.raises(ValueError):                                                # a plan for another mesh
        rom.pod_prom_run_hyper_blocked(Xn, np.ones(N), mu1, mu2, dt, 2, None, res.plan, p)
    with pytest.raises(ValueError):
        rom.pod_prom_run_hyper_blocked(mesh(N + 1)[0], np.ones(N + 1), mu1, mu2, dt, 2, None, res.plan, p)
    max_r, max_m = lib.limits("bg_hyper_rom_blocked_limits", 2)
    with pytest.raises(ValueError):
        rom.HyperBlockedPodPlan(np.zeros((N, max_r + 1)), s, X, dev)               # one column too many
    Xm, _ = mesh(max_m + 1)
    with pytest.raises(ValueError):
        rom.HyperBlockedPodPlan(np.zeros((max_m + 1, 100)), unit_rows(max_m + 1, "LSPG"), Xm, dev)      # one row too many
    with pytest.raises(ValueError):
        rom.HyperBlockedPodPlan(Phi, s, X, dev, slots=0)
