"""bg_hyper_quad_rom_run: the hyper-reduced quadratic-manifold PROM time loop on sampled mesh rows (csrc/quad_hyper.hip, the
body of csrc/quad_device.hpp), against the oracle (all rows, unit weights: the loop is then pod_quadratic_manifold itself)
and against the numpy restatement of the weighted-row, carried-q iteration (tests/hyper_quad_ref.py) on meshes beyond every
other quadratic-manifold loop and at the edges of the table.  reference: FEMBurgers.pod_quadratic_manifold,
FEM/fem_burgers.py:1081-1175.

Everything is fp64.  Against the oracle the gate is TOL = 1e-10 on the decoded history with every iteration count equal.
Against the restatement it is max(1e-10, 10 d), d being the restatement's own spread between summing the rows forwards and
backwards, computed in the test (measured on the CPU: 1.6e-14 … 2.2e-14 at N = 2049, 6e-15 … 2.5e-14 at N = 96, both
projections), counts identical."""
import functools

import numpy as np
import pytest
import torch

import hyper_quad_ref as hq
from conftest import mesh, rel_l2
from loop_cases import TOL, draw, to_np

pytestmark = pytest.mark.gpu
ENTRY, NT = hq.ENTRY, hq.NT
KEYS = ("q", "iters", "flags", "info")


def sampling(rows, xi, proj):
    from burgers_hip import pod
    return pod.RowSampling(np.asarray(rows, dtype=np.int32), np.asarray(xi, dtype=np.float64), proj.lower(), 0.0, 0, 0.0)


def stencil_nodes(rows, N):
    rows = np.asarray(rows, dtype=np.int64)
    return np.unique(np.clip(rows[:, None] + np.arange(-1, 2)[None, :], 0, N - 1))


def run(case, s, proj, mu1, mu2, nT=NT, **kw):
    from burgers_hip import rom
    N, dt, _, E, _ = hq._case(case)
    X, Phi, H = hq.case_data(case)
    res = rom.quadratic_run_hyper(X, np.ones(N), mu1, mu2, dt, nT, Phi, H, s, rom.PROJ[proj.lower()], E=E, **kw)
    torch.cuda.synchronize()
    return res


def check_against_restatement(res, case, s, proj, mu1, mu2, nT=NT):
    """Every sample: rel-L2 of the decoded history against the restatement's within max(1e-10, 10 d), q likewise, every count
    equal and below the cap, no flag."""
    N, dt, n, E, _ = hq._case(case)
    X, Phi, H = hq.case_data(case)
    rows, xi = s.rows.numpy(), s.xi.numpy()
    assert res.path == ENTRY and res.plan.m == s.m and res.plan.n_nodes == len(stencil_nodes(rows, N))
    assert bool((res.info == 0).all()) and not bool(res.flags.any())
    assert tuple(res.q.shape) == (len(mu1), nT + 1, n)
    hist, q, iters = to_np(res.hist), to_np(res.q), to_np(res.iters)
    for b in range(len(mu1)):
        Q, it = hq.hyper_quad_prom(X, dt, nT, np.ones(N), mu1[b], E, mu2[b], Phi, H, proj, rows, xi)
        Qb, itb = hq.hyper_quad_prom(X, dt, nT, np.ones(N), mu1[b], E, mu2[b], Phi, H, proj, rows, xi, backwards=True)
        U = hq.decode(Phi, H, Q, np.ones(N))
        d = rel_l2(hq.decode(Phi, H, Qb, np.ones(N)), U)
        gate = max(TOL, 10.0 * d)
        err, errq = rel_l2(hist[b].T, U), rel_l2(q[b].T, Q)
        print(f"N={N} {proj} sample {b}: m = {s.m}, nodes = {res.plan.n_nodes}, rel-L2 {err:.2e} (q: {errq:.2e}), spread {d:.2e}, "
              f"iterations {iters[b].tolist()} / {it.tolist()}")
        assert it.max() < hq.CAP and np.array_equal(it, itb)      # a condition on the input: the restatement converges
        assert err <= gate and errq <= gate, (proj, b, err, errq, gate)
        assert np.array_equal(iters[b], it), (proj, b)
        assert np.array_equal(hist[b, 0], np.ones(N))             # column 0 is u0 itself
        assert np.array_equal(q[b, 0], to_np(res._keep[5])[b])    # ... and row 0 of q the q0 the loop was given


# ---- all rows, unit weights: the oracle itself ------------------------------------------------------------------------------
@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("case", sorted(hq.CASES))
def test_all_rows_with_unit_weights_is_the_oracle(hip, case, proj):
    """full-256: N = m = 256, the row limit, four full slabs of table nodes; B = 6, so the second group has two padding
    waves.  perturbed-96: a partial slab on a non-uniform mesh with E > 0 and n = 17, not a multiple of 4."""
    from burgers_hip import lib
    from oracle import burgers_ref as br
    N, dt, n, E, _ = hq.CASES[case]
    X, Phi, H = hq.case_data(case)
    B = 6 if case == "full-256" else 3
    mu1, mu2 = draw(B)
    res = run(case, sampling(np.arange(N), np.ones(N), proj), proj, mu1, mu2)
    assert res.path == ENTRY and res.plan.m == N and res.plan.n_nodes == N and tuple(res.q.shape) == (B, NT + 1, n)
    assert lib.mesh_is_uniform(X) == (case == "full-256")
    if case == "full-256":
        assert N == lib.limits("bg_hyper_quad_rom_limits", 3)[1]
    hist, iters = to_np(res.hist), to_np(res.iters)
    assert bool((res.info == 0).all()) and not bool(res.flags.any())
    for s in range(B):
        U, ito = br.pod_quadratic_manifold(X, dt, NT, np.ones(N), mu1[s], E, mu2[s], Phi, H, projection=proj, return_iters=True)
        err = rel_l2(hist[s].T, U)
        print(f"{case} {proj} sample {s}: rel-L2 {err:.2e}, iterations {iters[s].tolist()} / {ito.tolist()}")
        assert err <= TOL, (case, proj, s, err)
        assert np.array_equal(iters[s], ito)
    assert np.array_equal(hist[:, 0], np.ones((B, N)))
    assert tuple(res.snapshots().shape) == (B, N, NT + 1) and res.newton_steps == int(iters.sum())


# ---- sampled rows beyond every other quadratic-manifold loop ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def limits_sampling(proj):
    """The builder's default sampling at N = 1024 (120 rows, about 150 stencil nodes) plus isolated rows placed by hand, every
    fifth mesh row from 200 on that is at least three rows from any other, weight 0.01, up to m = 256: both limits at once
    and a table of 513 .. 768 nodes, the second description of the kernel."""
    N = hq.MID[0]
    s = hq.builder_sampling(hq.MID, proj)
    w = dict(zip(s.rows.tolist(), s.xi.tolist()))
    for c in range(200, N - 2, 5):
        if len(w) < 256 and min(abs(c - r) for r in w) >= 3:
            w[c] = 0.01
    rows = np.array(sorted(w), dtype=np.int32)
    return sampling(rows, [w[int(i)] for i in rows], proj)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_builder_sampling_on_2049_nodes_against_the_restatement(hip, proj):
    s = hq.builder_sampling(hq.LONG, proj)
    mu1, mu2 = draw(2, seed=11)
    res = run(hq.LONG, s, proj, mu1, mu2, nT=4)
    assert res.plan.n_nodes <= 512
    check_against_restatement(res, hq.LONG, s, proj, mu1, mu2, nT=4)


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_both_limits_at_once_against_the_restatement(hip, proj):
    from burgers_hip import lib
    s = limits_sampling(proj)
    mu1, mu2 = draw(2, seed=11)
    res = run(hq.MID, s, proj, mu1, mu2, nT=4)
    max_n, max_m, max_nodes = lib.limits("bg_hyper_quad_rom_limits", 3)
    assert res.plan.n == max_n and res.plan.m == max_m and 512 < res.plan.n_nodes <= max_nodes
    check_against_restatement(res, hq.MID, s, proj, mu1, mu2, nT=4)


# ---- the edges of the table, N = 96 ------------------------------------------------------------------------------------------
def edge_rows(name):
    N = hq.CASES["perturbed-96"][0]
    return {
        "63-and-64": np.setdiff1d(np.arange(N), [10]),           # both sides of the slab boundary sampled; table position != index
        "63-only": np.setdiff1d(np.arange(N), [64]),             # the last row of slab 0 takes its right neighbour from s_unext
        "64-only": np.setdiff1d(np.arange(N), [63]),             # the first row of slab 1 takes its left neighbour from slab 0
        "no-last-row": np.arange(N - 1),                         # row N - 1 only a neighbour: not the mesh's last row
        "64-nodes": np.arange(63),                               # a table of exactly one slab; its last node only a neighbour
        "65-nodes": np.arange(64),                               # one node into the second slab
        "left-out": np.setdiff1d(np.arange(N), [10, 50, 51, 70]),
    }[name]


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
@pytest.mark.parametrize("name", ["63-and-64", "63-only", "64-only", "no-last-row", "64-nodes", "65-nodes", "left-out"])
def test_table_edges_against_the_restatement(hip, name, proj):
    """Unit weights on perturbed-96 (row N - 1 is sampled in every case but "no-last-row", "64-nodes" and "65-nodes")."""
    N = hq.CASES["perturbed-96"][0]
    rows = edge_rows(name)
    s = sampling(rows, np.ones(len(rows)), proj)
    mu1, mu2 = draw(2, seed=11)
    res = run("perturbed-96", s, proj, mu1, mu2)
    if name.endswith("-nodes"):
        assert res.plan.n_nodes == int(name[:2])
    check_against_restatement(res, "perturbed-96", s, proj, mu1, mu2)


# ---- scheduling does not change a bit ----------------------------------------------------------------------------------------
def test_a_trajectory_does_not_depend_on_the_batch(hip):
    """Alone, permuted, in a batch of 21 (five full groups and one wave), with the samples in their given order, and with a
    reused plan: bit-identical in q and counts."""
    case, proj = "perturbed-96", "LSPG"
    rows = edge_rows("left-out")
    s = sampling(rows, np.ones(len(rows)), proj)
    B = 21
    mu1, mu2 = draw(B)
    big = run(case, s, proj, mu1, mu2)
    perm = np.random.default_rng(2).permutation(B)
    shuffled = run(case, big.plan, proj, mu1[perm], mu2[perm])
    assert shuffled.plan is big.plan
    for k in KEYS:
        assert torch.equal(getattr(shuffled, k), getattr(big, k)[torch.as_tensor(perm, device=big.q.device)]), k
    for b in (0, 7, B - 1):
        alone = run(case, big.plan, proj, mu1[b:b + 1], mu2[b:b + 1])
        for k in KEYS:
            assert torch.equal(getattr(alone, k)[0], getattr(big, k)[b]), (k, b)
    unbalanced = run(case, big.plan, proj, mu1, mu2, balance=False)
    fresh = run(case, s, proj, mu1, mu2)
    for k in KEYS:
        assert torch.equal(getattr(unbalanced, k), getattr(big, k)) and torch.equal(getattr(fresh, k), getattr(big, k)), k
    assert fresh.plan is not big.plan and torch.equal(fresh.hist, big.hist)


def test_order_entries_outside_the_batch_are_skipped(hip):
    """The raw entry point with ``order`` entries outside [0, B): those slots store nothing (a wave without a sample, and a
    whole group without one), the other samples are bit-equal to the plain run."""
    from burgers_hip import lib, rom
    case, proj = "perturbed-96", "Galerkin"
    N, dt, n, E, _ = hq.CASES[case]
    rows = edge_rows("left-out")
    B, nT = 6, 3
    mu1, mu2 = draw(B)
    ref = run(case, sampling(rows, np.ones(len(rows)), proj), proj, mu1, mu2, nT=nT)
    plan, dev = ref.plan, ref.q.device
    u0d = torch.ones((B, N), dtype=torch.float64, device=dev)
    q0, u0n = rom._project_rows(u0d, plan.Phi), u0d[:, plan.nodes].contiguous()
    mu1d, mu2d = torch.as_tensor(mu1, device=dev), torch.as_tensor(mu2, device=dev)
    for entries, keep in (([0, -1, 2, 3, B + 5, 5], [0, 2, 3, 5]), ([-1, B + 5, B, -5, 4, 5], [4, 5])):
        lost = sorted(set(range(B)) - set(keep))
        qh = torch.full((B, nT + 1, n), -7.0, dtype=torch.float64, device=dev)
        iters = torch.full((B, nT), -2, dtype=torch.int32, device=dev)
        flags = torch.full((B,), -3, dtype=torch.int32, device=dev)
        info = torch.full((B,), -4, dtype=torch.int32, device=dev)
        order = torch.as_tensor(entries, dtype=torch.int32, device=dev)
        rc = lib.load().bg_hyper_quad_rom_run(N, B, n, plan.m, plan.n_nodes, nT, rom.PROJ[proj.lower()], lib.ptr(plan.xn),
                                              lib.ptr(plan.node), lib.ptr(plan.pos), lib.ptr(plan.xi), lib.ptr(plan.Phif),
                                              lib.ptr(plan.H3f), lib.ptr(q0), lib.ptr(u0n), lib.ptr(mu1d), lib.ptr(mu2d), dt, E,
                                              1e-6, hq.CAP, 0, lib.ptr(qh), lib.ptr(iters), lib.ptr(flags), lib.ptr(info),
                                              lib.ptr(order), lib.stream_ptr(dev))
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(qh[keep], ref.q[keep]) and torch.equal(iters[keep], ref.iters[keep])
        assert torch.equal(flags[keep], ref.flags[keep]) and torch.equal(info[keep], ref.info[keep])
        assert bool((qh[lost] == -7.0).all()) and bool((iters[lost] == -2).all())
        assert bool((flags[lost] == -3).all()) and bool((info[lost] == -4).all())


# ---- the public entry points -------------------------------------------------------------------------------------------------
def test_routing_is_opt_in(hip):
    """quadratic_run(hyper=) and the facade reach the new entry and return the reference's layout; a sampling trained for the
    other projection and a plan for another mesh are refused; without hyper= nothing routes here."""
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    case = "perturbed-96"
    N, dt, n, E, _ = hq.CASES[case]
    X, Phi, H = hq.case_data(case)
    s = sampling(np.arange(N), np.ones(N), "Galerkin")
    mu1, mu2 = draw(2)
    direct = run(case, s, "Galerkin", mu1, mu2)
    res = rom.quadratic_run(X, np.ones(N), mu1, mu2, dt, NT, Phi, H, projection="Galerkin", E=E, hyper=s)
    assert res.path == ENTRY and torch.equal(res.q, direct.q) and torch.equal(res.hist, direct.hist)
    again = rom.quadratic_run(X, np.ones(N), mu1, mu2, dt, NT, None, None, projection="Galerkin", E=E, hyper=res.plan)
    assert again.plan is res.plan and torch.equal(again.q, direct.q)
    fem = FEMBurgers(X, mesh(N)[1])
    U = fem.pod_quadratic_manifold(dt, NT, np.ones(N), mu1[0], E, mu2[0], Phi, H, projection="Galerkin", hyper=s)
    alone = run(case, s, "Galerkin", mu1[:1], mu2[:1])            # q does not depend on the batch; the decode GEMM's shape does
    assert torch.equal(alone.q[0], direct.q[0]) and rel_l2(to_np(alone.hist[0]), to_np(direct.hist[0])) < 1e-14
    assert U.shape == (N, NT + 1) and np.array_equal(U, to_np(alone.hist[0]).T)
    assert np.array_equal(fem.last_iters, to_np(direct.iters[0]))
    with pytest.raises(ValueError):
        rom.quadratic_run(X, np.ones(N), mu1, mu2, dt, NT, Phi, H, projection="LSPG", E=E, hyper=s)
    X2 = X.copy(); X2[5] += 1e-3
    with pytest.raises(ValueError):
        rom.quadratic_run_hyper(X2, np.ones(N), mu1, mu2, dt, NT, Phi, H, res.plan, rom.PROJ["galerkin"], E=E)
    assert rom.quadratic_run(X, np.ones(N), mu1, mu2, dt, 2, Phi, H, projection="Galerkin", E=E).path == "bg_quad_rom_run"
