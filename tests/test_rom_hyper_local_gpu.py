"""bg_hyper_local_rom_run: the hyper-reduced local POD time loop on sampled mesh rows (csrc/rom_hyper_local.hip), against the
oracle (all rows, unit weights: the loop is then local_prom_burgers itself) and against the numpy restatement of its
semantics (tests/hyper_local_ref.py) on a mesh no full local loop takes.
reference: FEMBurgers.local_prom_burgers, FEM/fem_burgers.py:979-1079.

Clustering: hyper_local_ref.dense_clustering -- 11 clusters with non-nested orthonormal bases of 8 .. 40 columns, 12 global
modes.  Runs: u0 = 1, 40 steps, mu in hyper_local_ref.MUS."""
import functools
import types

import numpy as np
import pytest
import torch

import hyper_local_ref as hl
from conftest import mesh, rel_l2
from hyper_ref import training_runs
from loop_cases import TOL, draw, to_np

pytestmark = pytest.mark.gpu
ENTRY = "bg_hyper_local_rom_run"
NT = hl.NT
MU1, MU2 = [m[0] for m in hl.MUS], [m[1] for m in hl.MUS]
# N = 96 on the perturbed mesh with diffusion (m = 96: three slabs of 32 rows, every branch of the non-uniform assembly) and
# N = 256 at the largest row count the kernel takes (eight slabs); both run through widths 8 .. 40.
FULL = {"perturbed": (96, 0.07, 0.01, 3), "widest": (256, 0.05, 0.0, None)}


@functools.lru_cache(maxsize=None)
def full_run(case, proj, options=0):
    from burgers_hip import rom
    N, dt, E, seed = FULL[case]
    X, centres, bases, Ug = hl.dense_clustering(N, dt, E, seed)
    res = rom.local_prom_run_hyper(X, np.ones(N), MU1, MU2, dt, NT, centres, bases, Ug, hl.MG, hl.all_rows(N, proj),
                                   rom.PROJ[proj.lower()], E=E, options=options)
    torch.cuda.synchronize()
    return res, (X, centres, bases, Ug, dt, E)


@functools.lru_cache(maxsize=None)
def oracle_run(case, proj, b):
    """(U, iters, clusters) of the oracle, with the conditions the tests rely on asserted on its own output."""
    from oracle import burgers_ref as br
    N, dt, E, seed = FULL[case]
    X, centres, bases, Ug = hl.dense_clustering(N, dt, E, seed)
    U, it, cl = br.local_prom_burgers(X, dt, NT, np.ones(N), MU1[b], E, MU2[b], centres, bases, Ug, hl.MG, projection=proj,
                                      return_iters=True)
    _, _, _, _, margin = hl.hyper_local_prom(X, dt, NT, np.ones(N), MU1[b], E, MU2[b], centres, bases, Ug, hl.MG, proj,
                                             np.arange(N), np.ones(N))
    sw = int((np.diff(cl) != 0).sum())
    print(f"{case} {proj} sample {b}: the oracle switches {sw} times, iterates up to {int(it.max())}, tie margin {margin:.1e}")
    assert sw >= 4 and it.max() < 20 and margin >= 1e-8
    return U, it, cl


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", sorted(FULL))
def test_all_rows_with_unit_weights_is_the_oracle(hip, case, proj):
    from burgers_hip import lib
    res, (X, centres, bases, Ug, dt, E) = full_run(case, proj)
    N = len(X)
    assert res.path == ENTRY and res.plan.m == N and tuple(res.q.shape) == (2, NT + 1, 40) and tuple(res.clusters.shape) == (2, NT)
    assert lib.mesh_is_uniform(X) == (case == "widest")
    if case == "widest":
        assert (40, N) == lib.limits("bg_hyper_local_rom_limits", 4)[:2]        # the widest basis and the row limit at once
    assert bool((res.info == 0).all()) and not bool(res.flags.any())
    hist, q = to_np(res.hist), to_np(res.q)
    assert np.array_equal(hist[:, 0], np.ones((2, N)))                          # column 0 is u0 itself
    for b in range(2):
        U, it, cl = oracle_run(case, proj, b)
        err = rel_l2(hist[b].T, U)
        print(f"N={N} {proj} sample {b}: rel-L2 {err:.2e}, iterations {to_np(res.iters[b]).tolist()}")
        assert np.array_equal(to_np(res.clusters[b]), cl), (proj, b)
        assert np.array_equal(to_np(res.iters[b]), it), (proj, b)
        assert err < TOL, (proj, b, err)
        c0 = int(cl[0])
        w0 = bases[c0].shape[1]
        assert c0 == 0 and w0 == 8                                              # the run starts in the narrowest cluster
        assert rel_l2(q[b, 0, :w0], bases[c0].T @ np.ones(N)) < 1e-14 and not q[b, 0, w0:].any()      # entry 0 is Phi_c0^T u0
        for n in range(NT):                                                     # zero beyond the step's width
            assert not q[b, n + 1, bases[int(cl[n])].shape[1]:].any()
    assert tuple(res.snapshots().shape) == (2, N, NT + 1)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_forced_pivoting_gives_the_same_result(hip, proj):
    from burgers_hip import lib
    res, _ = full_run("perturbed", proj)
    piv, _ = full_run("perturbed", proj, lib.BG_OPT_FORCE_PIVOTED)
    for b in range(2):
        oracle_run("perturbed", proj, b)                                        # the runs contract: below the cap
    worst = max(rel_l2(a, b) for a, b in zip(to_np(piv.hist), to_np(res.hist)))
    print(f"{proj}: forced pivoting against the fast kernel, worst rel-L2 {worst:.2e}")
    assert bool((piv.info == 0).all()) and not bool(piv.flags.any())
    assert worst < TOL and torch.equal(piv.iters, res.iters) and torch.equal(piv.clusters, res.clusters)


# ---- sampled rows on N = 1025: a mesh no full local loop takes --------------------------------------------------------------
LN, LDT = 1025, 0.025


@functools.lru_cache(maxsize=None)
def sampled_case(proj):
    """(X, centres, bases, Ug, sampling): build_local_row_sampling's rows (training runs 0, 4, 8, every 10th step, the
    defaults tau = 1e-4 and min_rows = 120) plus rows added by hand with a small weight, so that 1, N - 2, N - 1, an adjacent
    pair (700, 701) and an isolated row (500) are present and m is no multiple of 32."""
    from burgers_hip import pod
    X, centres, bases, Ug = hl.dense_clustering(LN, LDT)
    s = pod.build_local_row_sampling(X, centres, bases, Ug, hl.MG, training_runs(LN, LDT, keep=[0, 4, 8]), LDT, proj)
    w = dict(zip(s.rows.tolist(), s.xi.tolist()))
    assert 0 in w
    for extra in (1, LN - 2, LN - 1, 700, 701, 500):
        w.setdefault(extra, 0.05)
    for extra in (300, 301):
        if len(w) % 32 == 0:
            w.setdefault(extra, 0.05)
    rows = np.array(sorted(w), dtype=np.int32)
    assert len(rows) % 32 != 0 and len(rows) <= pod.hyper_local_rom_limits()[1]
    return X, centres, bases, Ug, pod.RowSampling(rows, np.array([w[int(i)] for i in rows]), proj.lower(), s.residual, s.pairs, s.tau)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_sampled_rows_against_the_restatement(hip, proj):
    """The gate is max(TOL, 10 d), d the restatement's own spread between summing the rows forwards and backwards (the
    reference's sensitivity to the order of the sum; the kernel's order is a third one).  The cluster paths must be equal,
    and the iteration counts wherever the two orders of the restatement agree on them."""
    from burgers_hip import rom
    X, centres, bases, Ug, s = sampled_case(proj)
    res = rom.local_prom_run_hyper(X, np.ones(LN), MU1, MU2, LDT, NT, centres, bases, Ug, hl.MG, s, rom.PROJ[proj.lower()])
    torch.cuda.synchronize()
    assert res.path == ENTRY and res.plan.m == s.m and bool((res.info == 0).all())
    hist, iters, clusters = to_np(res.hist), to_np(res.iters), to_np(res.clusters)
    rows, xi = s.rows.numpy(), s.xi.numpy()
    for b in range(2):
        U, Q, it, cl, margin = hl.hyper_local_prom(X, LDT, NT, np.ones(LN), MU1[b], 0.0, MU2[b], centres, bases, Ug, hl.MG, proj, rows, xi)
        Ub, _, itb, clb, marginb = hl.hyper_local_prom(X, LDT, NT, np.ones(LN), MU1[b], 0.0, MU2[b], centres, bases, Ug, hl.MG, proj,
                                                       rows, xi, backwards=True)
        sw = int((np.diff(cl) != 0).sum())
        d = rel_l2(Ub[:, 1:], U[:, 1:])
        err = rel_l2(hist[b].T[:, 1:], U[:, 1:])
        print(f"N={LN} m={s.m} {proj} sample {b}: d {d:.2e}, rel-L2 {err:.2e}, {sw} switches, tie margin {min(margin, marginb):.1e}, "
              f"iterations {iters[b].tolist()} / {it.tolist()}")
        # conditions on the input, from the restatement's own output
        assert sw >= 4 and it.max() < 20 and itb.max() < 20 and min(margin, marginb) >= 1e-8 and np.array_equal(cl, clb)
        assert np.array_equal(clusters[b], cl), (proj, b)
        assert err < max(TOL, 10.0 * d), (proj, b, err, d)
        assert rel_l2(to_np(res.q[b]).T, Q) < max(TOL, 10.0 * d)
        agree = it == itb
        assert np.array_equal(iters[b][agree], it[agree]), (proj, b)
        assert not bool(res.flags[b])


# ---- one cluster: the POD loop -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_one_cluster_is_the_hyper_reduced_pod_loop(hip, proj):
    """C = 1: no pick can change anything, so the loop is bg_hyper_rom_run on the same basis and sampling."""
    from burgers_hip import pod, rom
    N, dt, E, seed = FULL["perturbed"]
    X, centres, bases, Ug = hl.dense_clustering(N, dt, E, seed)
    Phi = bases[2]                                                              # 17 columns
    rows = np.setdiff1d(np.arange(N), [10, 50, 51, 70]).astype(np.int32)
    s = pod.RowSampling(rows, np.linspace(0.5, 1.5, len(rows)), proj.lower(), 0.0, 0, 0.0)
    p = rom.PROJ[proj.lower()]
    loc = rom.local_prom_run_hyper(X, np.ones(N), MU1, MU2, dt, NT, centres[:1], {0: Phi}, Ug, hl.MG, s, p, E=E)
    podr = rom.pod_prom_run_hyper(X, np.ones(N), MU1, MU2, dt, NT, Phi, s, p, E=E)
    torch.cuda.synchronize()
    worst = max(rel_l2(a, b) for a, b in zip(to_np(loc.hist), to_np(podr.hist)))
    print(f"{proj}: C = 1 against bg_hyper_rom_run, worst rel-L2 {worst:.2e}, bitwise equal q: {torch.equal(loc.q, podr.q)}")
    assert bool((loc.info == 0).all()) and bool((podr.info == 0).all()) and int(podr.iters.max()) < 20
    assert worst < TOL and torch.equal(loc.iters, podr.iters) and not bool(loc.clusters.any())


# ---- scheduling changes nothing ------------------------------------------------------------------------------------------------
def raw_run(plan, X, mu1, mu2, dt, E, proj, order=None, fill=None):
    """The C entry point on a plan's operands with u0 = 1: (q, iters, flags, info, clusters), ``fill`` in q and flags before the call."""
    from burgers_hip import lib, rom
    dev, N, B = plan.stack.device, plan.N, len(mu1)
    u0d = torch.ones((B, N), dtype=torch.float64, device=dev)
    qg0, pu0 = plan.project(u0d)
    u0s = (u0d[:, plan.stencil] * plan.inside).contiguous()
    mu1d, mu2d = torch.as_tensor(np.asarray(mu1, dtype=np.float64), device=dev), torch.as_tensor(np.asarray(mu2, dtype=np.float64), device=dev)
    q = torch.full((B, NT + 1, plan.rmax), 0.0 if fill is None else fill[0], dtype=torch.float64, device=dev)
    iters = torch.zeros((B, NT), dtype=torch.int32, device=dev)
    flags = torch.full((B,), 0 if fill is None else fill[1], dtype=torch.int32, device=dev)
    info = torch.zeros((B,), dtype=torch.int32, device=dev)
    clusters = torch.full((B, NT), -1, dtype=torch.int32, device=dev)
    od = None if order is None else torch.tensor(order, dtype=torch.int32, device=dev)
    rc = lib.load().bg_hyper_local_rom_run(
        N, B, plan.C, plan.rmax, plan.mg, plan.m, NT, rom.PROJ[proj.lower()], lib.ptr(plan.rows), lib.ptr(plan.xi), lib.ptr(plan.xs),
        lib.ptr(plan.PhiS), lib.ptr(plan.widths), lib.ptr(plan.trans), lib.ptr(plan.pick), lib.ptr(plan.centres), lib.ptr(qg0),
        lib.ptr(pu0), lib.ptr(u0s), lib.ptr(mu1d), lib.ptr(mu2d), dt, E, 1e-6, 20, lib.mesh_options(X, supg=True), lib.ptr(q),
        lib.ptr(iters), lib.ptr(flags), lib.ptr(info), lib.ptr(clusters), lib.ptr(od), lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    return q, iters, flags, info, clusters


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_a_trajectory_does_not_depend_on_its_neighbours(hip, proj):
    """Sample 0 of the parity run alone, in a reversed ``order``, and as sample 577 of 600 drawn parameters run in slot order:
    more samples than resident workgroups, so its workgroup has worked on another sample before, one that ended in another
    cluster and left its table pointer, width, q_g and switch values behind."""
    from burgers_hip import rom
    ref, (X, centres, bases, Ug, dt, E) = full_run("perturbed", proj)
    plan, N = ref.plan, len(X)
    alone = raw_run(plan, X, MU1[:1], MU2[:1], dt, E, proj)
    rev = raw_run(plan, X, MU1, MU2, dt, E, proj, order=[1, 0])
    mu1, mu2 = draw(600, seed=5)
    mu1[577], mu2[577] = MU1[0], MU2[0]
    many = rom.local_prom_run_hyper(X, np.ones(N), mu1, mu2, dt, NT, None, None, None, hl.MG, plan, rom.PROJ[proj.lower()], E=E,
                                    balance=False)
    torch.cuda.synchronize()
    grid = 2 * torch.cuda.get_device_properties(ref.q.device).multi_processor_count
    if grid <= 577:                                                            # (512 on the MI355X: slot 577 is the second of its workgroup)
        assert int(many.clusters[577 - grid, -1]) != int(many.clusters[577, 0])      # which comes from another cluster
    assert bool((many.info == 0).all())
    print(f"{proj}: entry 0 of sample 577 equal to the run alone: {torch.equal(many.q[577, 0], ref.q[0, 0])}")
    for name, (q, iters, clusters) in (("alone", (alone[0][0], alone[1][0], alone[4][0])), ("reversed", (rev[0][0], rev[1][0], rev[4][0])),
                                       ("batch of 600", (many.q[577], many.iters[577], many.clusters[577]))):
        assert torch.equal(q, ref.q[0]) and torch.equal(iters, ref.iters[0]) and torch.equal(clusters, ref.clusters[0]), name
    assert torch.equal(rev[0][1], ref.q[1]) and torch.equal(rev[4][1], ref.clusters[1])


def test_order_entries_outside_the_batch_are_skipped(hip):
    proj = "LSPG"
    ref, (X, centres, bases, Ug, dt, E) = full_run("perturbed", proj)
    mu1, mu2 = [MU1[0], MU1[1], MU1[0], MU1[1]], [MU2[0], MU2[1], MU2[1], MU2[0]]
    q, iters, flags, info, clusters = raw_run(ref.plan, X, mu1, mu2, dt, E, proj, order=[1, -1, 0, 4 + 5], fill=(-7.0, -3))
    assert torch.equal(q[:2], ref.q) and torch.equal(iters[:2], ref.iters) and torch.equal(clusters[:2], ref.clusters)
    assert torch.equal(flags[:2], ref.flags) and bool((info == 0).all())
    assert bool((q[2:] == -7.0).all()) and bool((flags[2:] == -3).all()) and bool((clusters[2:] == -1).all())


def test_plan_reuse_refusals_and_the_empty_batch(hip, monkeypatch):
    from burgers_hip import rom
    first, (X, centres, bases, Ug, dt, E) = full_run("perturbed", "Galerkin")
    N = len(X)
    p = rom.PROJ["galerkin"]
    again = rom.local_prom_run_hyper(X, np.ones(N), MU1, MU2, dt, NT, None, None, None, hl.MG, first.plan, p, E=E)
    torch.cuda.synchronize()
    assert again.plan is first.plan and again.path == ENTRY
    for k in ("q", "iters", "flags", "info", "clusters", "hist"):
        assert torch.equal(getattr(again, k), getattr(first, k)), k
    empty = rom.local_prom_run_hyper(X, np.ones(N), np.zeros(0), np.zeros(0), dt, 2, None, None, None, hl.MG, first.plan, p, E=E)
    torch.cuda.synchronize()
    assert tuple(empty.q.shape) == (0, 3, 40) and tuple(empty.hist.shape) == (0, 3, N) and tuple(empty.clusters.shape) == (0, 2)

    def no_launch(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(rom, "_device_loop", no_launch)
    with pytest.raises(ValueError, match="projection"):
        rom.local_prom_run_hyper(X, np.ones(N), MU1, MU2, dt, 2, None, None, None, hl.MG, first.plan, rom.PROJ["lspg"], E=E)
    with pytest.raises(ValueError):
        rom.local_prom_run_hyper(mesh(N)[0], np.ones(N), MU1, MU2, dt, 2, None, None, None, hl.MG, first.plan, p)      # another mesh
    with pytest.raises(ValueError):
        rom.local_prom_run_hyper(mesh(N + 1)[0], np.ones(N + 1), MU1, MU2, dt, 2, None, None, None, hl.MG, first.plan, p)


def test_facade_opt_in_and_unchanged_default(hip):
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    X, centres, bases, Ug, s = sampled_case("LSPG")
    _, T = mesh(LN)
    km = types.SimpleNamespace(cluster_centers_=centres)
    U = FEMBurgers(X, T).local_prom_burgers(LDT, 6, np.ones(LN), 4.8, 0.0, 0.021, km, bases, Ug, hl.MG, projection="LSPG", hyper=s)
    res = rom.local_prom_run_hyper(X, np.ones(LN), [4.8], [0.021], LDT, 6, centres, bases, Ug, hl.MG, s, rom.PROJ["lspg"])
    torch.cuda.synchronize()
    assert np.asarray(U).shape == (LN, 7) and np.array_equal(np.asarray(U), to_np(res.hist[0]).T)
    with pytest.raises(ValueError):
        FEMBurgers(X, T).local_prom_burgers(LDT, 2, np.ones(LN), 4.8, 0.0, 0.021, km, bases, Ug, hl.MG, projection="Galerkin", hyper=s)
    # without ``hyper`` the call takes the route it took before, bit for bit
    N, dt, E, seed = FULL["widest"]
    Xs, cs, bs, Us = hl.dense_clustering(N, dt, E, seed)
    default = rom.local_prom_run(Xs, np.ones(N), MU1, MU2, dt, 4, cs, bs, Us, hl.MG, projection="LSPG", fused=True)
    direct = rom.local_prom_run_fused(Xs, np.ones(N), MU1, MU2, dt, 4, cs, bs, Us, hl.MG, projection="LSPG")
    torch.cuda.synchronize()
    assert default.path == "bg_local_rom_run"
    for k in ("hist", "iters", "flags", "info", "clusters"):
        assert torch.equal(getattr(default, k), getattr(direct, k)), k
    Uf = FEMBurgers(Xs, mesh(N)[1]).local_prom_burgers(dt, 4, np.ones(N), MU1, 0.0, MU2, types.SimpleNamespace(cluster_centers_=cs),
                                                       bs, Us, hl.MG, projection="LSPG", fused=True)
    assert np.array_equal(np.asarray(Uf), to_np(default.hist).transpose(0, 2, 1))
    long_default = rom.local_prom_run(X, np.ones(LN), [4.8], [0.021], LDT, 1, centres, bases, Ug, hl.MG, projection="LSPG")
    assert long_default.path == "host"
