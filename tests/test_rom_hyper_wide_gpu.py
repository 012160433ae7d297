"""bg_hyper_rom_run_wide: the hyper-reduced POD-PROM time loop for 41 to 96 modes on up to 512 sampled mesh rows
(csrc/rom_hyper_wide.hip), against the oracle (all rows, unit weights: the loop is then pod_prom_burgers itself) and against
the numpy restatement of the weighted-row iteration (tests/hyper_ref.py), with the redo of the samples the guarded
pivot-free solve hands back.  reference: FEMBurgers.pod_prom_burgers, FEM/fem_burgers.py:709-785.

Bases: the leading r left singular vectors of the FOM snapshots (oracle, C) of the 3 x 3 training grid, 200 steps."""
import functools

import numpy as np
import pytest
import torch

from conftest import mesh, rel_l2
from hyper_ref import hyper_prom, training_runs
from loop_cases import TOL, check_pod_vs_oracle, draw, pod_basis, to_np

pytestmark = pytest.mark.gpu
ENTRY = "bg_hyper_rom_run_wide"
NT = 12


def unit_rows(rows, proj):
    from burgers_hip import pod
    rows = np.asarray(rows, dtype=np.int32)
    return pod.RowSampling(rows, np.ones(len(rows)), proj.lower(), 0.0, 0, 0.0)


# "limits": the widest basis on the largest row count the kernel takes (32 slabs of 16 rows), both limits at once.
# "odd_width": r = 77 is no multiple of 4 (one live column in the last block of lane index 3, dead blocks behind it) and
# m = 300 leaves the last slab ragged (12 of 16 rows).  "perturbed": r = 41 -- one live column beyond the narrow loop's 40 -- on
# the perturbed mesh with diffusion, every branch of the non-uniform assembly.  The oracle converges at all three with
# multipliers of at most 0.38, which check_pod_vs_oracle's flag test and ``redone == 0`` assert.
FULL = {"limits": (512, 0.05, 96, 0.0, None), "odd_width": (300, 0.08, 77, 0.0, None), "perturbed": (160, 0.2, 41, 0.01, 7)}
B_FULL = 3


@functools.lru_cache(maxsize=None)
def full_run(case, proj, options=0):
    from burgers_hip import rom
    N, dt, r, E, seed = FULL[case]
    X, Phi = pod_basis(N, dt, r, E=E, seed=seed)
    mu1, mu2 = draw(B_FULL)
    res = rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, NT, Phi, unit_rows(np.arange(N), proj), rom.PROJ[proj.lower()],
                                      E=E, options=options)
    torch.cuda.synchronize()
    return res, (X, Phi, mu1, mu2, dt, E)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", sorted(FULL))
def test_all_rows_with_unit_weights_is_the_oracle(hip, case, proj):
    from burgers_hip import lib
    res, (X, Phi, mu1, mu2, dt, E) = full_run(case, proj)
    N, r = Phi.shape
    assert res.path == ENTRY and res.plan.m == N and tuple(res.q.shape) == (B_FULL, NT + 1, r) and res.redone == 0
    assert lib.mesh_is_uniform(X) == (case != "perturbed")
    if case == "limits":
        assert (r, N) == lib.limits("bg_hyper_rom_wide_limits", 2)          # both limits at once
    assert np.array_equal(to_np(res.hist[:, 0]), np.ones((B_FULL, N)))      # column 0 is u0 itself
    assert rel_l2(to_np(res.q[:, 0]), np.broadcast_to(Phi.T @ np.ones(N), (B_FULL, r))) < 1e-14      # row 0 of q is Phi^T u0
    check_pod_vs_oracle(res, X, dt, NT, mu1, mu2, Phi, proj, E=E)
    assert tuple(res.snapshots().shape) == (B_FULL, N, NT + 1)


# ---- the restatement, with the multipliers the unpivoted elimination of its own systems meets ------------------------------------
def restatement(X, dt, nT, mu1, mu2, E, Phi, proj, rows, xi):
    """(Q, iters, d, worst): hyper_prom with the rows summed forwards; d, its rel-L2 spread against the sum backwards (the
    reference's sensitivity to the order of the sum; the kernel's order is a third one); worst, the largest sub-diagonal
    multiplier of the unpivoted elimination over the forward run's systems (np.linalg.solve wrapped as
    loop_cases.max_multiplier wraps it).  Both runs must converge."""
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


def check_against_restatement(res, X, dt, nT, mu1, mu2, E, Phi, proj, rows, xi, label):
    """The project's gate for sampled rows: rel-L2 below max(TOL, 10 d) for the decoded history and for q, no iteration count
    different, no flag and no sample left marked; ``redone`` is all of the batch when the restatement's own elimination meets
    a multiplier above 1 and none of it otherwise (inputs within 1 % of the guard's threshold, or on both sides of it, are
    refused: they would test rounding, not the loop)."""
    B = len(mu1)
    assert res.path == ENTRY and not bool(res.flags.any()) and bool((res.info == 0).all())
    q, iters, worsts = to_np(res.q), to_np(res.iters), []
    for b in range(B):
        Q, it, d, worst = restatement(X, dt, nT, mu1[b], mu2[b], E, Phi, proj, rows, xi)
        err = rel_l2(to_np(res.hist[b]).T[:, 1:], Phi @ Q[:, 1:])
        print(f"{label} {proj} sample {b}: d {d:.2e}, rel-L2 {err:.2e}, multiplier {worst:.3f}, iterations {iters[b].tolist()} / {it.tolist()}")
        assert err < max(TOL, 10.0 * d), (proj, b, err, d)
        assert rel_l2(q[b].T, Q) < max(TOL, 10.0 * d)
        assert np.array_equal(iters[b], it), (proj, b)
        worsts.append(worst)
    assert not any(0.99 < w < 1.01 for w in worsts), worsts
    assert all(w >= 1.01 for w in worsts) or all(w <= 0.99 for w in worsts), worsts
    assert res.redone == (B if max(worsts) >= 1.01 else 0), (res.redone, worsts)


LEFT_OUT = {"limits": [3, 200, 201, 300, 509], "perturbed": [10, 50, 51, 70, 158]}


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", sorted(LEFT_OUT))
def test_rows_left_out_against_the_restatement(hip, case, proj):
    """Unit weights with five rows left out: behind the first of them the sampled-row index j and the mesh row i differ, so a
    stencil coordinate or a forcing load taken at j instead of i is another node's; with all rows sampled i == j hides that.
    "limits": m = 507, beyond the narrow loop's 256 with a ragged last slab (11 of 16 rows); "perturbed": the non-uniform mesh."""
    from burgers_hip import rom
    N, dt, r, E, seed = FULL[case]
    X, Phi = pod_basis(N, dt, r, E=E, seed=seed)
    rows = np.setdiff1d(np.arange(N), LEFT_OUT[case]).astype(np.int32)
    assert len(rows) == N - 5 and (case != "limits" or (len(rows) == 507 and len(rows) % 16 == 11))
    mu1, mu2 = draw(2)
    res = rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, NT, Phi, unit_rows(rows, proj), rom.PROJ[proj.lower()], E=E)
    torch.cuda.synchronize()
    assert res.plan.m == len(rows)
    check_against_restatement(res, X, dt, NT, mu1, mu2, E, Phi, proj, rows, np.ones(len(rows)), f"N={N} r={r} m={len(rows)}")


# ---- sampled rows ------------------------------------------------------------------------------------------------------------
# (N, dt, r, min_rows, steps, B): build_row_sampling on three training runs, every 20th step, tau = 1e-3.  "n600": the default
# 3 r fill, 192 rows.  "n2049": beyond every full POD loop, r = 96 with 200 rows (the 3 r fill is out of reach on three
# runs); its LSPG systems meet multipliers above 1, so that batch comes back marked and is redone.
SAMPLED = {"n600": (600, 0.04, 64, None, NT, 3), "n2049": (2049, 0.0125, 96, 200, 6, 2)}


@functools.lru_cache(maxsize=None)
def sampled_case(case, proj):
    from burgers_hip import pod
    N, dt, r, min_rows, _, _ = SAMPLED[case]
    X, Phi = pod_basis(N, dt, r)
    s = pod.build_row_sampling(X, Phi, training_runs(N, dt, keep=[0, 4, 8]), dt, proj, tau=1e-3, stride=20, min_rows=min_rows)
    return X, Phi, s


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", sorted(SAMPLED))
def test_sampled_rows_against_the_restatement(hip, case, proj):
    from burgers_hip import rom
    N, dt, r, min_rows, nT, B = SAMPLED[case]
    X, Phi, s = sampled_case(case, proj)
    assert s.m == (3 * r if min_rows is None else min_rows)
    mu1, mu2 = draw(B, seed=11)
    res = rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, nT, Phi, s, rom.PROJ[proj.lower()])      # routed by width
    torch.cuda.synchronize()
    assert res.plan.m == s.m and isinstance(res.plan, rom.HyperWidePodPlan)
    check_against_restatement(res, X, dt, nT, mu1, mu2, 0.0, Phi, proj, s.rows.numpy(), s.xi.numpy(), f"N={N} r={r} m={s.m}")
    if case == "n600":
        assert res.redone == 0


# ---- the hand-back, the narrow loop's sizes, the raw ABI -------------------------------------------------------------------------
@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_forced_pivoting_redoes_every_sample_and_agrees(hip, proj):
    from burgers_hip import lib
    res, (X, Phi, mu1, mu2, dt, E) = full_run("perturbed", proj)
    piv, _ = full_run("perturbed", proj, lib.BG_OPT_FORCE_PIVOTED)
    assert piv.redone == B_FULL and res.redone == 0 and bool((piv.info == 0).all()) and piv.path == ENTRY
    check_pod_vs_oracle(piv, X, dt, NT, mu1, mu2, Phi, proj, E=E)
    worst = max(rel_l2(a, b) for a, b in zip(to_np(piv.hist), to_np(res.hist)))
    print(f"{proj}: every sample redone by the weighted-row library iteration against the device loop, worst rel-L2 {worst:.2e}")
    assert worst < TOL and torch.equal(piv.iters, res.iters)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_forty_modes_agree_with_the_narrow_loop(hip, proj):
    from burgers_hip import rom
    N, dt, r = 256, 0.05, 40
    X, Phi = pod_basis(N, dt, r)
    mu1, mu2 = draw(3)
    s, p = unit_rows(np.arange(N), proj), rom.PROJ[proj.lower()]
    wide = rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, NT, Phi, s, p)
    narrow = rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, NT, Phi, s, p)
    torch.cuda.synchronize()
    assert (wide.path, narrow.path) == (ENTRY, "bg_hyper_rom_run") and wide.redone == 0
    assert not bool(wide.flags.any()) and not bool(narrow.flags.any())
    worst = max(rel_l2(a, b) for a, b in zip(to_np(wide.hist), to_np(narrow.hist)))
    print(f"{proj}: r = 40 through the wide loop against the narrow loop, worst rel-L2 {worst:.2e}")
    assert worst < TOL and torch.equal(wide.iters, narrow.iters)


def test_order_entries_outside_the_batch_are_skipped(hip):
    from burgers_hip import lib, rom
    ref, (X, Phi, mu1, mu2, dt, E) = full_run("perturbed", "LSPG")
    assert ref.redone == 0
    plan, B, N, dev = ref.plan, B_FULL, len(X), ref.q.device
    u0d = torch.ones((B, N), dtype=torch.float64, device=dev)
    q0, u0s = (u0d @ plan.Phi).contiguous(), (u0d[:, plan.stencil] * plan.inside).contiguous()
    mu1d, mu2d = torch.as_tensor(mu1, device=dev), torch.as_tensor(mu2, device=dev)
    qh = torch.full((B, NT + 1, plan.r), -7.0, dtype=torch.float64, device=dev)
    iters = torch.zeros((B, NT), dtype=torch.int32, device=dev)
    flags = torch.full((B,), -3, dtype=torch.int32, device=dev)
    info = torch.zeros((B,), dtype=torch.int32, device=dev)
    order = torch.tensor([2, -1, B + 5], dtype=torch.int32, device=dev)
    rc = lib.load().bg_hyper_rom_run_wide(N, B, plan.r, plan.m, NT, rom.PROJ["lspg"], lib.ptr(plan.rows), lib.ptr(plan.xi),
                                          lib.ptr(plan.xs), lib.ptr(plan.PhiS), lib.ptr(q0), lib.ptr(u0s), lib.ptr(mu1d), lib.ptr(mu2d),
                                          dt, E, 1e-6, 20, lib.mesh_options(X, supg=True), lib.ptr(qh), lib.ptr(iters), lib.ptr(flags),
                                          lib.ptr(info), lib.ptr(order), lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(qh[2], ref.q[2]) and torch.equal(iters[2], ref.iters[2]) and int(flags[2]) == int(ref.flags[2])
    assert bool((info == 0).all())
    assert bool((qh[[0, 1]] == -7.0).all()) and bool((flags[[0, 1]] == -3).all())


def test_plan_reuse_refusals_and_the_empty_batch(hip, monkeypatch):
    from burgers_hip import pod, rom
    first, (X, Phi, mu1, mu2, dt, E) = full_run("perturbed", "Galerkin")
    N = len(X)
    p = rom.PROJ["galerkin"]
    assert isinstance(first.plan, rom.HyperWidePodPlan)
    again = rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, NT, None, first.plan, p, E=E)      # the plan picks the loop
    torch.cuda.synchronize()
    assert again.plan is first.plan and again.path == ENTRY and again.redone == 0
    assert torch.equal(again.q, first.q) and torch.equal(again.iters, first.iters) and torch.equal(again.flags, first.flags)
    empty = rom.pod_prom_run_hyper_wide(X, np.ones(N), np.zeros(0), np.zeros(0), dt, 2, None, first.plan, p, E=E)
    torch.cuda.synchronize()
    assert tuple(empty.q.shape) == (0, 3, first.plan.r) and tuple(empty.hist.shape) == (0, 3, N) and empty.redone == 0

    def no_launch(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(rom, "_device_loop", no_launch)
    dev = first.q.device
    with pytest.raises(ValueError, match="projection"):
        rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, 2, None, first.plan, rom.PROJ["lspg"], E=E)      # trained for the other one
    with pytest.raises(ValueError):
        rom.pod_prom_run_hyper_wide(mesh(N)[0], np.ones(N), mu1, mu2, dt, 2, None, first.plan, p)                 # a plan for another mesh
    with pytest.raises(ValueError):
        rom.pod_prom_run_hyper_wide(mesh(N + 1)[0], np.ones(N + 1), mu1, mu2, dt, 2, None, first.plan, p)
    narrow = rom.HyperPodPlan(Phi[:, :17], unit_rows(np.arange(N), "Galerkin"), X, dev)
    with pytest.raises(ValueError):
        rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, 2, None, narrow, p, E=E)                         # the other loop's plan
    rs = lambda rows, xi: pod.RowSampling(np.array(rows, dtype=np.int32), np.array(xi, dtype=np.float64), "galerkin", 0.0, 0, 0.0)
    for bad in (rs([0, 5, 5], [1, 1, 1]), rs([0, 7, 3], [1, 1, 1]), rs([0, N], [1, 1]), rs([-1, 3], [1, 1]), rs([0, 3], [1, -0.5]),
                rs([0, 3], [1, np.nan]), rs([], []), rs([0, 3], [1])):
        with pytest.raises(ValueError):
            rom.HyperWidePodPlan(Phi, bad, X, dev)
    with pytest.raises(ValueError):
        rom.HyperWidePodPlan(Phi, pod.RowSampling(np.arange(N, dtype=np.int32), np.ones(N), "petrov", 0.0, 0, 0.0), X, dev)      # an unknown projection
    with pytest.raises(ValueError):
        rom.HyperWidePodPlan(np.zeros((N, 97)), unit_rows(np.arange(N), "Galerkin"), X, dev)                      # one column too many
    X5, _ = mesh(513)
    with pytest.raises(ValueError):
        rom.HyperWidePodPlan(np.zeros((513, 4)), unit_rows(np.arange(513), "Galerkin"), X5, dev)                  # one row too many
    with pytest.raises(ValueError):
        rom.pod_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, 2, np.zeros((N, 97)), unit_rows(np.arange(N), "Galerkin"), p)


def test_facade_at_96_modes_and_the_narrow_route_unchanged(hip):
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    N, dt, r, E, _ = FULL["limits"]
    X, Phi = pod_basis(N, dt, r)
    _, T = mesh(N)
    s = unit_rows(np.arange(N), "LSPG")
    U = FEMBurgers(X, T).pod_prom_burgers(dt, 4, np.ones(N), 4.8, 0.0, 0.021, Phi, projection="LSPG", hyper=s)
    res = rom.pod_prom_run_hyper_wide(X, np.ones(N), [4.8], [0.021], dt, 4, Phi, s, rom.PROJ["lspg"])
    torch.cuda.synchronize()
    assert res.path == ENTRY and np.asarray(U).shape == (N, 5) and np.array_equal(np.asarray(U), to_np(res.hist[0]).T)
    with pytest.raises(ValueError):
        FEMBurgers(X, T).pod_prom_burgers(dt, 2, np.ones(N), 4.8, 0.0, 0.021, Phi, projection="Galerkin", hyper=s)
    # a sampling with a basis the narrow loop takes still goes there
    N2, dt2 = 96, 0.2
    X2, Phi2 = pod_basis(N2, dt2, 17)
    mu1, mu2 = draw(2)
    small = rom.pod_prom_run_hyper(X2, np.ones(N2), mu1, mu2, dt2, 3, Phi2, unit_rows(np.arange(N2), "LSPG"), rom.PROJ["lspg"])
    torch.cuda.synchronize()
    assert small.path == "bg_hyper_rom_run" and type(small.plan) is rom.HyperPodPlan and not hasattr(small, "redone")
