"""bg_hyper_rom_run_wide with BG_OPT_PIVOT_ON_DEVICE (``pivot="device"``): the repair kernel that redoes, with the pivoted
96 x 96 solve wide_solve_pivoted, the samples the guarded pivot-free elimination hands back (csrc/rom_hyper_wide.hip,
csrc/rom_wide_device.hpp).  Against the numpy restatement of the weighted-row iteration (tests/hyper_ref.py) on samplings whose
reduced systems need genuine row exchanges, against the oracle with every sample forced through the repair kernel, against
the default route bit for bit where nothing is marked, and on an exactly singular reduced system.
reference: FEMBurgers.pod_prom_burgers, FEM/fem_burgers.py:709-785."""
import functools

import numpy as np
import pytest
import torch

from conftest import mesh, rel_l2
from hyper_ref import hyper_prom
from loop_cases import TOL, check_pod_vs_oracle, draw, pod_basis, to_np

pytestmark = pytest.mark.gpu
ENTRY = "bg_hyper_rom_run_wide"


def sampling(rows, xi, proj):
    from burgers_hip import pod
    return pod.RowSampling(np.asarray(rows, dtype=np.int32), np.asarray(xi, dtype=np.float64), proj.lower(), 0.0, 0, 0.0)


# ---- genuine row exchanges -------------------------------------------------------------------------------------------------------
# (N, dt, r, size): rows = unique([0] + choice(N, size)), weights 10 ** uniform(-3, 3) from default_rng(1).  With six decades
# between the weights the reduced systems are far from diagonally dominant: the unpivoted elimination of the restatement's own
# systems meets multipliers of 1.71 .. 1.74 (W300) and 4.71 .. 5.13 (W512), LAPACK exchanges more than 30 and 50 .. 68 rows
# per system, and every step converges in at most 10 iterations.
WEIGHTED = {"W300": (300, 0.08, 77, 231, 232), "W512": (512, 0.05, 96, 400, 401)}
NT_W = 6


@functools.lru_cache(maxsize=None)
def weighted_rows(case):
    N, _, _, size, m = WEIGHTED[case]
    rng = np.random.default_rng(1)
    rows = np.unique(np.concatenate([[0], rng.choice(N, size, replace=False)]))
    xi = 10.0 ** rng.uniform(-3, 3, len(rows))
    assert len(rows) == m
    return rows, xi


def restatement(X, dt, nT, mu1, mu2, E, Phi, proj, rows, xi):
    """(Q, iters, d, worst) as in test_rom_hyper_wide_gpu.py: hyper_prom with the rows summed forwards; d, its rel-L2 spread
    against the sum backwards; worst, the largest sub-diagonal multiplier of the unpivoted elimination over the forward run's
    systems.  Both runs must converge."""
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
    different, no flag, info 0 everywhere; and the precondition of these cases, a multiplier of at least 1.01 in the
    restatement's own unpivoted elimination, so that the fast kernel hands the sample back."""
    assert res.path == ENTRY and not bool(res.flags.any()) and bool((res.info == 0).all())
    q, iters = to_np(res.q), to_np(res.iters)
    for b in range(len(mu1)):
        Q, it, d, worst = restatement(X, dt, nT, mu1[b], mu2[b], E, Phi, proj, rows, xi)
        err = rel_l2(to_np(res.hist[b]).T[:, 1:], Phi @ Q[:, 1:])
        print(f"{label} {proj} sample {b}: d {d:.2e}, rel-L2 {err:.2e}, multiplier {worst:.3f}, iterations {iters[b].tolist()} / {it.tolist()}")
        assert worst >= 1.01, (proj, b, worst)
        assert err < max(TOL, 10.0 * d), (proj, b, err, d)
        assert rel_l2(q[b].T, Q) < max(TOL, 10.0 * d)
        assert np.array_equal(iters[b], it), (proj, b)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", sorted(WEIGHTED))
def test_row_exchanges_on_the_device_against_the_restatement_and_the_host_route(hip, case, proj):
    from burgers_hip import rom
    N, dt, r, _, m = WEIGHTED[case]
    X, Phi = pod_basis(N, dt, r)
    rows, xi = weighted_rows(case)
    mu1, mu2 = draw(2)
    s, p = sampling(rows, xi, proj), rom.PROJ[proj.lower()]
    dev = rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, NT_W, Phi, s, p, pivot="device")
    host = rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, NT_W, None, dev.plan, p, pivot="host")
    torch.cuda.synchronize()
    assert dev.plan.m == m and dev.redone == 0
    check_against_restatement(dev, X, dt, NT_W, mu1, mu2, 0.0, Phi, proj, rows, xi, f"{case} N={N} r={r} m={m}")
    assert host.redone == 2 and bool((host.info == 0).all()) and not bool(host.flags.any())      # the fast kernel marked them
    worst = max(rel_l2(a, b) for a, b in zip(to_np(dev.hist), to_np(host.hist)))
    print(f"{case} {proj}: the repair kernel against the host-side redo, worst rel-L2 {worst:.2e}")
    assert worst < TOL and torch.equal(dev.iters, host.iters)


# ---- every sample through the repair kernel: the three all-rows cases of test_rom_hyper_wide_gpu.py -------------------------------
FULL = {"limits": (512, 0.05, 96, 0.0, None), "odd_width": (300, 0.08, 77, 0.0, None), "perturbed": (160, 0.2, 41, 0.01, 7)}
B_FULL, NT = 3, 12


def unit_rows(N, proj):
    return sampling(np.arange(N), np.ones(N), proj)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", sorted(FULL))
def test_forced_pivoting_on_the_device_is_the_oracle(hip, case, proj):
    from burgers_hip import lib, rom
    N, dt, r, E, seed = FULL[case]
    X, Phi = pod_basis(N, dt, r, E=E, seed=seed)
    mu1, mu2 = draw(B_FULL)
    res = rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, NT, Phi, unit_rows(N, proj), rom.PROJ[proj.lower()], E=E,
                                      options=lib.BG_OPT_FORCE_PIVOTED, pivot="device")
    torch.cuda.synchronize()
    assert res.path == ENTRY and res.redone == 0 and tuple(res.q.shape) == (B_FULL, NT + 1, r)
    check_pod_vs_oracle(res, X, dt, NT, mu1, mu2, Phi, proj, E=E)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_unmarked_samples_are_left_alone(hip, proj):
    from burgers_hip import rom
    N, dt, r, E, _ = FULL["odd_width"]
    X, Phi = pod_basis(N, dt, r)
    mu1, mu2 = draw(B_FULL)
    s, p = unit_rows(N, proj), rom.PROJ[proj.lower()]
    default = rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, NT, Phi, s, p)
    dev = rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, NT, None, default.plan, p, pivot="device")
    torch.cuda.synchronize()
    assert default.redone == 0 and dev.redone == 0
    for k in ("q", "iters", "flags", "info"):
        assert torch.equal(getattr(dev, k), getattr(default, k)), k


# ---- an exactly singular reduced system --------------------------------------------------------------------------------------------
def test_zero_mode_is_reported_as_singular(hip):
    from burgers_hip import rom
    N, dt, r, _, _ = WEIGHTED["W300"]
    X, Phi = pod_basis(N, dt, r)
    Phi = Phi.copy()
    Phi[:, 50] = 0.0                                     # row and column 50 of every Galerkin system are exactly zero
    rows, xi = weighted_rows("W300")
    mu1, mu2 = draw(2)
    res = rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, 3, Phi, sampling(rows, xi, "Galerkin"), rom.PROJ["galerkin"],
                                      pivot="device")
    torch.cuda.synchronize()
    assert res.redone == 0 and to_np(res.info).tolist() == [51, 51]
    with pytest.raises(rom.SingularReducedSystem):
        rom.check_singular(res)
    from fem_burgers import FEMBurgers
    _, T = mesh(N)
    with pytest.raises(rom.SingularReducedSystem):
        FEMBurgers(X, T).pod_prom_burgers(dt, 3, np.ones(N), mu1[0], 0.0, mu2[0], Phi, hyper=sampling(rows, xi, "Galerkin"), pivot="device")


# ---- order entries outside the batch, both kernels -----------------------------------------------------------------------------------
def test_order_entries_outside_the_batch_are_skipped_by_both_kernels(hip):
    from burgers_hip import lib, rom
    N, dt, r, _, _ = WEIGHTED["W300"]
    X, Phi = pod_basis(N, dt, r)
    rows, xi = weighted_rows("W300")
    B = 3
    mu1, mu2 = draw(B)
    p = rom.PROJ["lspg"]
    ref = rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, NT_W, Phi, sampling(rows, xi, "LSPG"), p, pivot="device")
    host = rom.pod_prom_run_hyper_wide(X, np.ones(N), mu1, mu2, dt, NT_W, None, ref.plan, p)
    torch.cuda.synchronize()
    assert host.redone == B and bool((ref.info == 0).all())           # every sample goes through both kernels
    plan, dev = ref.plan, ref.q.device
    u0d = torch.ones((B, N), dtype=torch.float64, device=dev)
    q0, u0s = (u0d @ plan.Phi).contiguous(), (u0d[:, plan.stencil] * plan.inside).contiguous()
    mu1d, mu2d = torch.as_tensor(mu1, device=dev), torch.as_tensor(mu2, device=dev)
    qh = torch.full((B, NT_W + 1, plan.r), -7.0, dtype=torch.float64, device=dev)
    iters = torch.zeros((B, NT_W), dtype=torch.int32, device=dev)
    flags = torch.full((B,), -3, dtype=torch.int32, device=dev)
    info = torch.tensor([lib.BG_INFO_NEEDS_PIVOTING, lib.BG_INFO_NEEDS_PIVOTING, 0], dtype=torch.int32, device=dev)
    order = torch.tensor([2, -1, B + 5], dtype=torch.int32, device=dev)
    rc = lib.load().bg_hyper_rom_run_wide(N, B, plan.r, plan.m, NT_W, p, lib.ptr(plan.rows), lib.ptr(plan.xi), lib.ptr(plan.xs),
                                          lib.ptr(plan.PhiS), lib.ptr(q0), lib.ptr(u0s), lib.ptr(mu1d), lib.ptr(mu2d), dt, 0.0, 1e-6, 20,
                                          lib.mesh_options(X, supg=True) | lib.BG_OPT_PIVOT_ON_DEVICE, lib.ptr(qh), lib.ptr(iters),
                                          lib.ptr(flags), lib.ptr(info), lib.ptr(order), lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(qh[2], ref.q[2]) and torch.equal(iters[2], ref.iters[2]) and int(flags[2]) == int(ref.flags[2])
    assert info.tolist() == [lib.BG_INFO_NEEDS_PIVOTING, lib.BG_INFO_NEEDS_PIVOTING, 0]      # no slot names samples 0 and 1, marked or not
    assert bool((qh[[0, 1]] == -7.0).all()) and bool((flags[[0, 1]] == -3).all()) and bool((iters[[0, 1]] == 0).all())
