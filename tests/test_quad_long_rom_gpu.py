"""bg_quad_rom_run_long: the device-side quadratic-manifold PROM time loop for meshes of 513 .. 1024 nodes, n <= 40
(csrc/quad_long.hip), against the oracle and the host-driven batched iteration (the default route for N > 512).
reference: FEMBurgers.pod_quadratic_manifold, FEM/fem_burgers.py:1081-1175.

Manifolds: Phi = the leading n left singular vectors of the FOM snapshots S (oracle, C) of the 3 x 3 training grid, 200
steps; H = compute_H(build_Q(q), S - Phi q, alpha = 1e-2) with q = Phi^T S (oracle/burgers_ref.py)."""
import functools

import numpy as np
import pytest
import torch

from conftest import mesh, rel_l2
from loop_cases import draw, same, training_snapshots
from oracle import burgers_ref as br

pytestmark = pytest.mark.gpu
TOL = 1e-10        # BASELINE north_star: <= 1e-10 relative L2 vs the reference
CAP = 25           # newton_itmax of the reference
ENTRY = "bg_quad_rom_run_long"


@functools.lru_cache(maxsize=None)
def _manifold(N, dt, n, E=0.0, seed=None):
    X, S, U = training_snapshots(N, dt, E, seed)
    Phi = np.ascontiguousarray(U[:, :n])
    q = Phi.T @ S
    H = np.ascontiguousarray(br.compute_H(br.build_Q(q), S - Phi @ q, 1e-2))
    return X, Phi, H


def _check_vs_oracle(res, X, dt, nT, mu1, mu2, Phi, H, proj, E=0.0, samples=None, tol=TOL, itmax=CAP, capped=False):
    """Every listed sample (default: all): the oracle's own counts are below the cap (a capped step amplifies rounding,
    so such inputs are excluded by the choice of input), rel-L2 of the history <= tol, every iteration count equal."""
    hist, iters = res.hist.cpu().numpy(), res.iters.cpu().numpy()
    for s in (range(len(mu1)) if samples is None else samples):
        U, ito = br.pod_quadratic_manifold(X, dt, nT, np.ones(len(X)), mu1[s], E, mu2[s], Phi, H, projection=proj,
                                           newton_itmax=itmax, return_iters=True)
        err = rel_l2(hist[s].T, U)
        print(f"N={len(X)} n={Phi.shape[1]} {proj} sample {s}: rel-L2 {err:.2e}, iterations {iters[s].tolist()} / {np.asarray(ito).tolist()}")
        if not capped:
            assert int(np.max(ito)) < itmax, (proj, s, "the oracle itself hits the cap on this input")
        assert err <= tol, (proj, s, err)
        assert np.array_equal(iters[s], ito), (proj, s)
    if not capped:
        assert not bool(res.flags.any())
    assert bool((res.info == 0).all())


CASES = [(1024, 0.025, 40, "LSPG"), (1024, 0.025, 40, "Galerkin"), (1024, 0.025, 21, "LSPG"), (1024, 0.025, 21, "Galerkin"),
         (1000, 0.025, 33, "LSPG"), (1000, 0.025, 33, "Galerkin"), (768, 0.03, 30, "LSPG"), (768, 0.03, 30, "Galerkin"),
         (600, 0.04, 40, "LSPG"), (600, 0.04, 40, "Galerkin"), (513, 0.05, 21, "LSPG")]     # (513, 0.05, 21) Galerkin: the reference hits its cap


@pytest.mark.parametrize("N,dt,n,proj", CASES)
def test_parity_with_the_oracle(hip, N, dt, n, proj):
    from burgers_hip import rom
    X, Phi, H = _manifold(N, dt, n)
    mu1, mu2 = draw(6)
    res = rom.quadratic_run(X, np.ones(N), mu1, mu2, dt, 12, Phi, H, projection=proj, long_mesh=True)
    torch.cuda.synchronize()
    assert res.path == ENTRY
    _check_vs_oracle(res, X, dt, 12, mu1, mu2, Phi, H, proj)


@pytest.mark.parametrize("proj", ["LSPG", "Galerkin"])
def test_at_batch_size_against_the_host_driven_route(hip, proj):
    """B = 1024 on N = 1024, n = 40: identical counts and flags against the default route, rel-L2 per sample, 16 samples
    against the oracle; the sample order, a permuted batch and a single-sample launch do not change a bit."""
    from burgers_hip import rom
    N, dt, nT, B = 1024, 0.025, 4, 1024
    X, Phi, H = _manifold(N, dt, 40)
    mu1, mu2 = draw(B)
    p = rom.PROJ[proj.lower()]
    res = rom.quadratic_run(X, np.ones(N), mu1, mu2, dt, nT, Phi, H, projection=proj, long_mesh=True)
    ref = rom.quadratic_run(X, np.ones(N), mu1, mu2, dt, nT, Phi, H, projection=proj)
    plain = rom.quadratic_run_long(X, np.ones(N), mu1, mu2, dt, nT, res.plan, p, balance=False)
    perm = np.random.default_rng(8).permutation(B)
    shuf = rom.quadratic_run_long(X, np.ones(N), mu1[perm], mu2[perm], dt, nT, res.plan, p)
    one = rom.quadratic_run_long(X, np.ones(N), mu1[777], mu2[777], dt, nT, res.plan, p)
    torch.cuda.synchronize()
    assert res.path == ENTRY and ref.path == "host" and plain.path == ENTRY
    differ = torch.nonzero((res.iters != ref.iters).any(1)).flatten().tolist()
    for s in differ[:8]:
        print(f"{proj}: sample {s} (mu1 {mu1[s]:.6f}, mu2 {mu2[s]:.6f}): counts {res.iters[s].tolist()} / host {ref.iters[s].tolist()}")
    assert torch.equal(res.iters, ref.iters) and torch.equal(res.flags, ref.flags), (proj, differ)
    fh, hh = res.hist.cpu().numpy(), ref.hist.cpu().numpy()
    worst = max(rel_l2(fh[s], hh[s]) for s in range(B))
    print(f"{proj}: worst rel-L2 against the host-driven route over {B} samples {worst:.2e}")
    assert worst <= TOL
    _check_vs_oracle(res, X, dt, nT, mu1, mu2, Phi, H, proj, samples=range(0, B, B // 16))
    same(plain, res)
    permd = torch.as_tensor(perm, device=res.hist.device)
    assert torch.equal(res.hist[permd], shuf.hist) and torch.equal(res.iters[permd], shuf.iters)
    assert torch.equal(res.hist[777], one.hist[0]) and torch.equal(res.iters[777], one.iters[0])


@pytest.mark.parametrize("proj", ["LSPG", "Galerkin"])
@pytest.mark.parametrize("case", ["diffusion", "nonuniform"])
def test_diffusion_and_nonuniform_mesh(hip, case, proj):
    from burgers_hip import lib, rom
    N, dt, nT = 1024, 0.025, 12
    E, seed = (0.01, None) if case == "diffusion" else (0.0, 21)
    X, Phi, H = _manifold(N, dt, 40, E=E, seed=seed)
    assert lib.mesh_is_uniform(X) == (seed is None)
    mu1, mu2 = draw(3)
    res = rom.quadratic_run(X, np.ones(N), mu1, mu2, dt, nT, Phi, H, projection=proj, E=E, long_mesh=True)
    torch.cuda.synchronize()
    assert res.path == ENTRY
    _check_vs_oracle(res, X, dt, nT, mu1, mu2, Phi, H, proj, E=E)


def test_iteration_cap(hip):
    """"Newton did not converge" (:1171) is a flag, not an error; counts equal the cap."""
    from burgers_hip import lib, rom
    N, dt = 1024, 0.025
    X, Phi, H = _manifold(N, dt, 40)
    mu1, mu2 = draw(3)
    r = rom.quadratic_run(X, np.ones(N), mu1, mu2, dt, 3, Phi, H, newton_itmax=2, long_mesh=True)
    torch.cuda.synchronize()
    assert r.path == ENTRY
    assert bool((r.flags & lib.BG_FLAG_HIT_CAP).ne(0).all()) and bool((r.iters == 2).all())
    # two Newton iterations from u0 = 1 leave the state far from the manifold's fixed point: the unconverged iteration
    # amplifies rounding differences (2.6e-10 measured in test_quad_fused_gpu.py at N = 512), hence 1e-8 here only
    _check_vs_oracle(r, X, dt, 3, mu1, mu2, Phi, H, "LSPG", tol=1e-8, itmax=2, capped=True)


def _synthetic_manifold(N, n, seed, scale=2e-3):
    """A smooth orthonormal basis and a small quadratic tensor (the construction of test_quad_fused_gpu.py)."""
    rng = np.random.default_rng(seed)
    xi = np.linspace(0, 1, N)
    cols = [np.ones(N), xi] + [np.tanh((xi - c0) * 10) for c0 in np.linspace(0.1, 0.9, n - 2)]
    Phi = np.linalg.qr(np.stack(cols, 1))[0]
    H = scale * rng.standard_normal((N, n * (n + 1) // 2))
    H -= Phi @ (Phi.T @ H)
    return Phi, H


def test_reduced_solve_pivots_like_numpy_and_singular_system(hip):
    """The construction of test_quad_fused_reduced_solve_pivots_like_numpy at N = 640: a tangent basis whose reduced system
    needs row exchanges; and an exactly singular system (a repeated basis column) raises LinAlgError like numpy (:1161)."""
    from burgers_hip import rom
    N, n = 640, 5
    Phi, H = _synthetic_manifold(N, n, seed=11)
    rng = np.random.default_rng(2)
    Mix = np.eye(n) + 3.0 * np.triu(rng.standard_normal((n, n)), 1)
    Phi2 = np.ascontiguousarray((Phi @ Mix)[:, ::-1])
    X, _ = mesh(N)
    Ar = Phi2.T @ Phi2                                          # LSPG at A ~ M: the diagonal is NOT the column maximum
    assert np.abs(Ar[1:, 0]).max() > abs(Ar[0, 0])
    mu1, mu2 = np.array([4.7, 5.1, 5.3]), np.full(3, 0.02)
    r = rom.quadratic_run(X, np.ones(N), mu1, mu2, 0.04, 3, Phi2, 0.0 * H, projection="LSPG", long_mesh=True)
    torch.cuda.synchronize()
    assert r.path == ENTRY
    _check_vs_oracle(r, X, 0.04, 3, mu1, mu2, Phi2, 0.0 * H, "LSPG", tol=1e-9)
    Phi3 = Phi.copy(); Phi3[:, 3] = Phi3[:, 1]
    with pytest.raises(np.linalg.LinAlgError):
        rom.quadratic_run(X, np.ones(N), 4.7, 0.02, 0.04, 2, Phi3, 0.0 * H, projection="Galerkin", long_mesh=True)


def test_plan_reuse_restart_and_refusals(hip, monkeypatch):
    from burgers_hip import rom
    N, dt = 1024, 0.025
    X, Phi, H = _manifold(N, dt, 40)
    mu1, mu2 = draw(5, seed=9)
    dev = torch.device("cuda", torch.cuda.current_device())
    p = rom.PROJ["lspg"]
    first = rom.quadratic_run_long(X, np.ones(N), mu1, mu2, dt, 5, (Phi, H), p)
    again = rom.quadratic_run_long(X, np.ones(N), mu1, mu2, dt, 5, first.plan, p)
    torch.cuda.synchronize()
    assert isinstance(first.plan, rom.QuadLongPlan) and again.plan is first.plan and again.path == ENTRY
    assert torch.equal(first.plan.Phi.cpu(), torch.as_tensor(Phi))           # the plan holds the basis it was built from
    same(again, first)
    # restart: the second half of a run from the state the first half ended in
    head = rom.quadratic_run_long(X, np.ones(N), mu1, mu2, dt, 2, first.plan, p)
    tail = rom.quadratic_run_long(X, head.hist[:, -1].cpu().numpy(), mu1, mu2, dt, 3, first.plan, p)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([head.hist, tail.hist[:, 1:]], 1), first.hist)
    assert torch.equal(torch.cat([head.iters, tail.iters], 1), first.iters)

    def no_launch(*a, **k):
        raise AssertionError("launched")
    monkeypatch.setattr(rom, "_device_loop", no_launch)
    X6, _ = mesh(600)
    with pytest.raises(ValueError):
        rom.quadratic_run_long(X6, np.ones(600), mu1, mu2, dt, 2, first.plan, p)              # a plan for another N
    other = rom.QuadLongPlan(Phi[:600, :17], H[:600, :17 * 18 // 2], dev)                     # another N and n
    with pytest.raises(ValueError):
        rom.quadratic_run_long(X, np.ones(N), mu1, mu2, dt, 2, other, p)
    with pytest.raises(ValueError):
        rom.QuadLongPlan(np.zeros((N, 41)), np.zeros((N, 41 * 42 // 2)), dev)                 # n = 41
    with pytest.raises(ValueError):
        rom.QuadLongPlan(np.zeros((1025, 8)), np.zeros((1025, 36)), dev)                      # N = 1025
    with pytest.raises(ValueError):
        rom.QuadLongPlan(Phi, H[:, :-1], dev)                                                 # a wrong H width
    with pytest.raises(ValueError):
        rom.quadratic_run_long(X, np.ones(N), mu1, mu2, dt, 2, (Phi, H[:, :-1]), p)


def test_order_entries_outside_the_batch_are_skipped(hip):
    from burgers_hip import lib, rom
    N, dt, B, n = 600, 0.04, 6, 40
    X, Phi, H = _manifold(N, dt, n)
    mu1, mu2 = draw(B, seed=3)
    p = rom.PROJ["galerkin"]
    ref = rom.quadratic_run_long(X, np.ones(N), mu1, mu2, dt, 3, (Phi, H), p)
    dev = ref.hist.device
    L = lib.load()
    u0d = torch.ones((B, N), dtype=torch.float64, device=dev)
    mu1d, mu2d, Xd = torch.as_tensor(mu1, device=dev), torch.as_tensor(mu2, device=dev), torch.as_tensor(X, device=dev)
    hist = torch.full((B, 4, N), -7.0, dtype=torch.float64, device=dev)
    iters = torch.full((B, 3), -7, dtype=torch.int32, device=dev)
    flags = torch.full((B,), -7, dtype=torch.int32, device=dev)
    info = torch.full((B,), -7, dtype=torch.int32, device=dev)
    order = torch.arange(B, dtype=torch.int32, device=dev)
    order[1], order[4] = -1, B + 5
    pl = ref.plan
    rc = L.bg_quad_rom_run_long(N, B, n, 3, p, lib.ptr(Xd), lib.ptr(pl.PhiT), lib.ptr(pl.Phif), lib.ptr(pl.H3f), lib.ptr(u0d),
                                lib.ptr(mu1d), lib.ptr(mu2d), dt, 0.0, 1e-6, 25, lib.mesh_options(X, supg=False), lib.ptr(hist),
                                lib.ptr(iters), lib.ptr(flags), lib.ptr(info), lib.ptr(order), lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    keep = [0, 2, 3, 5]
    assert torch.equal(hist[keep], ref.hist[keep]) and torch.equal(iters[keep], ref.iters[keep])
    assert torch.equal(flags[keep], ref.flags[keep]) and torch.equal(info[keep], ref.info[keep])
    assert bool((hist[[1, 4]] == -7.0).all()) and bool((iters[[1, 4]] == -7).all())
    assert bool((flags[[1, 4]] == -7).all()) and bool((info[[1, 4]] == -7).all())
    # a whole group of four without a valid entry, and a group that is all padding
    order2 = torch.tensor([-1, -3, B, B + 1, 5, 4], dtype=torch.int32, device=dev)
    hist.fill_(-7.0)
    rc = L.bg_quad_rom_run_long(N, B, n, 3, p, lib.ptr(Xd), lib.ptr(pl.PhiT), lib.ptr(pl.Phif), lib.ptr(pl.H3f), lib.ptr(u0d),
                                lib.ptr(mu1d), lib.ptr(mu2d), dt, 0.0, 1e-6, 25, lib.mesh_options(X, supg=False), lib.ptr(hist),
                                lib.ptr(iters), lib.ptr(flags), lib.ptr(info), lib.ptr(order2), lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(hist[[4, 5]], ref.hist[[4, 5]]) and bool((hist[:4] == -7.0).all())


def test_facade_opt_in_and_unchanged_defaults(hip):
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    N, dt = 1024, 0.025
    X, Phi, H = _manifold(N, dt, 40)
    _, T = mesh(N)
    U = FEMBurgers(X, T).pod_quadratic_manifold(dt, 6, np.ones(N), 4.8, 0.0, 0.021, Phi, H, projection="LSPG", long_mesh=True)
    Uo, ito = br.pod_quadratic_manifold(X, dt, 6, np.ones(N), 4.8, 0.0, 0.021, Phi, H, projection="LSPG", return_iters=True)
    assert int(np.max(ito)) < CAP
    assert np.asarray(U).shape == (N, 7) and rel_l2(np.asarray(U), Uo) <= TOL
    default = rom.quadratic_run(X, np.ones(N), [4.8], [0.021], dt, 2, Phi, H, projection="Galerkin")
    assert default.path == "host"
    unfused = rom.quadratic_run(X, np.ones(N), [4.8], [0.021], dt, 2, Phi, H, projection="Galerkin", fused=False, long_mesh=True)
    assert unfused.path == "host"
    X5, Phi5, H5 = _manifold(512, 0.05, 21)
    short = rom.quadratic_run(X5, np.ones(512), [4.8], [0.021], 0.05, 2, Phi5, H5)
    also = rom.quadratic_run(X5, np.ones(512), [4.8], [0.021], 0.05, 2, Phi5, H5, long_mesh=True)
    torch.cuda.synchronize()
    assert short.path == "bg_quad_rom_run" and also.path == "bg_quad_rom_run"
    same(short, also)
