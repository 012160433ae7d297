"""The device-side POD-RBF time loop for meshes of 513 .. 1024 nodes (bg_rbf_rom_run_long, rom.pod_rbf_run_long) against the
oracle and the host-driven batched iteration it replaces.  Gate: rel-L2 < 1e-9, the project's own for this closure (weights
up to 3.6e2 amplify rounding in the decoder), and identical iteration counts; tests/test_rbf_long_rom_abi.py shows on the
CPU that every case here moves by less than 1e-12 under operand noise of 4e-16.  The cases and their bases:
tests/rbf_long_cases.py."""
import numpy as np
import pytest
import torch

import rbf_long_cases as rc
from conftest import load_golden, mesh, rel_l2
from loop_cases import to_np

pytestmark = pytest.mark.gpu
TOL = rc.TOL
LONG = "bg_rbf_rom_run_long"


@pytest.mark.parametrize("name", list(rc.CASES))
def test_oracle_cases(hip, name):
    """Full mesh, one row past bg_rbf_rom_run, sizes that are no multiple of 64 or 8, an odd last row, a graded mesh with
    diffusion, the cap on every step, and the limit shapes n = 20 and nbar = 128 with 2400 centres."""
    from burgers_hip import rom
    X, mus, dt, steps, E, cl, kw = rc.case_inputs(name)
    N = len(X)
    res = rom.pod_rbf_run_long(X, np.ones(N), [m[0] for m in mus], [m[1] for m in mus], dt, steps, *cl, E=E, **kw)
    torch.cuda.synchronize()
    assert res.path == LONG and res.plan.long_mesh and tuple(res.plan.UT.shape) == (cl[0].shape[1] + cl[1].shape[1], 1024)
    assert int(res.info.abs().sum()) == 0
    hist, iters, flags = to_np(res.hist), to_np(res.iters), to_np(res.flags)
    for b, (U, ito) in enumerate(rc.oracle_run(name)):
        err = rel_l2(hist[b].T, U)
        print(f"{name} sample {b}: rel-L2 {err:.2e}, iterations {iters[b].tolist()} / {ito.tolist()}, flags {flags[b]}")
        assert err < TOL, (name, b, err)
        assert np.array_equal(iters[b], ito), (name, b)
        assert bool(flags[b] & 1) == bool((ito >= kw["max_newton"]).any()) and not flags[b] & 2


def test_matches_the_host_path(hip):
    """The bench's (mu1, mu2) draw, B = 64, N = 1024, 6 steps: per-sample parity with the host-driven iteration, the same
    iteration counts and the same flags.  imq / Galerkin at dt = 0.05: by the oracle 59 of the 64 samples run into the
    30-iteration cap and 5 converge at every step; gaussian / LSPG caps all 64 (as do imq / LSPG and gaussian / Galerkin)."""
    import bench
    from burgers_hip import rom
    X = rc.long_mesh(1024)
    mu1, mu2 = bench.mu_shard(64, 1, 0)
    cl = rc.closure(1024, "imq")
    kw = dict(projection="Galerkin", kernel="imq")
    dev = rom.pod_rbf_run(X, np.ones(1024), mu1, mu2, 0.05, 6, *cl, fused=True, long_mesh=True, **kw)
    host = rom.pod_rbf_run(X, np.ones(1024), mu1, mu2, 0.05, 6, *cl, fused=True, **kw)      # without the flag: as before
    torch.cuda.synchronize()
    assert dev.path == LONG and host.path == "host"
    assert int(dev.info.abs().sum()) == 0
    d, h = dev.hist.flatten(1), host.hist.flatten(1)
    worst = float(((d - h).norm(dim=1) / h.norm(dim=1)).max())
    fl = to_np(dev.flags)
    print(f"worst per-sample rel-L2 {worst:.2e}, capped {int((fl & 1).astype(bool).sum())} of 64, "
          f"iterations {int(dev.iters.sum())} / {int(host.iters.sum())}")
    assert torch.equal(dev.iters, host.iters)
    assert torch.equal(dev.flags, host.flags)
    assert (fl & 1).any() and not (fl & 1).all()                      # capped and converged samples both present
    assert not (fl & 2).any()
    assert worst < TOL, worst


def test_persistence_and_order(hip):
    from burgers_hip import lib, rom
    N = 1024
    X = rc.long_mesh(N)
    rng = np.random.default_rng(3)
    B = 600                                                          # more samples than slots: balancing reorders them
    mu1, mu2 = rng.uniform(4.25, 5.5, B), rng.uniform(0.015, 0.03, B)
    cl = rc.closure(N, "gaussian")
    a = rom.pod_rbf_run_long(X, np.ones(N), mu1, mu2, 0.05, 3, *cl, balance=True)
    b = rom.pod_rbf_run_long(X, np.ones(N), mu1, mu2, 0.05, 3, *cl, balance=False)
    c = rom.pod_rbf_run_long(X, np.ones(N), mu1, mu2, 0.05, 3, *cl, plan=a.plan)
    alone = rom.pod_rbf_run_long(X, np.ones(N), mu1[411:412], mu2[411:412], 0.05, 3, *cl, plan=a.plan)
    torch.cuda.synchronize()
    assert a.path == LONG and isinstance(a.plan, rom.RbfFusedPlan) and c.plan is a.plan
    for r in (b, c):
        assert torch.equal(a.hist, r.hist) and torch.equal(a.iters, r.iters) and torch.equal(a.flags, r.flags)
    assert torch.equal(alone.hist[0], a.hist[411]) and torch.equal(alone.iters[0], a.iters[411])
    # untrusted order entries: slots naming a sample outside [0, B) are skipped, the rows no slot names keep their content
    plan = a.plan
    dev = a.hist.device
    Xd = torch.as_tensor(X, device=dev)
    u0 = torch.ones((4, N), dtype=torch.float64, device=dev)
    m1, m2 = torch.as_tensor(mu1[:4], device=dev), torch.as_tensor(mu2[:4], device=dev)
    hist = torch.full((4, 4, N), -7.0, dtype=torch.float64, device=dev)
    iters = torch.zeros((4, 3), dtype=torch.int32, device=dev)
    flags = torch.full((4,), -3, dtype=torch.int32, device=dev)
    info = torch.zeros((4,), dtype=torch.int32, device=dev)
    order = torch.as_tensor([1, 4, 0, -3], dtype=torch.int32, device=dev)
    rc_ = lib.load().bg_rbf_rom_run_long(N, 4, plan.n, plan.nbar, plan.Ns, 3, lib.BG_PROJ_LSPG, plan.kind, lib.ptr(Xd),
                                         lib.ptr(plan.UT), lib.ptr(plan.XtT), lib.ptr(plan.Wd), lib.ptr(plan.bias),
                                         lib.ptr(plan.x_min), lib.ptr(plan.dx), plan.eps, lib.ptr(u0), lib.ptr(m1), lib.ptr(m2),
                                         0.05, 0.0, 1e-6, 30, lib.BG_OPT_SUPG, lib.ptr(hist), lib.ptr(iters), lib.ptr(flags),
                                         lib.ptr(info), lib.ptr(order), lib.stream_ptr(dev))
    assert rc_ == lib.BG_OK
    torch.cuda.synchronize()
    assert torch.equal(hist[:2], a.hist[:2]) and torch.equal(iters[:2], a.iters[:2]) and torch.equal(flags[:2], a.flags[:2])
    assert bool((hist[2:] == -7.0).all()) and not iters[2:].any() and bool((flags[2:] == -3).all())


def test_plans_and_refusals(hip):
    from burgers_hip import rom
    dev = torch.device("cuda", torch.cuda.current_device())
    X6, X7 = rc.long_mesh(600), rc.long_mesh(700)
    cl6, cl7 = rc.closure(600, "gaussian"), rc.closure(700, "gaussian")
    mu1, mu2 = [4.75, 5.2], [0.02, 0.016]
    p6 = rom.RbfFusedPlan(*cl6, "gaussian", dev, long_mesh=True)
    assert p6.ok
    with pytest.raises(ValueError):                                  # a plan for another mesh size
        rom.pod_rbf_run_long(X7, np.ones(700), mu1, mu2, 0.05, 1, *cl7, plan=p6)
    p16 = rom.RbfFusedPlan(cl6[0][:, :16], cl6[1], cl6[2][:, :16], cl6[3], 1.0, cl6[5][:16], cl6[6][:16], cl6[7], cl6[8],
                           "gaussian", dev, long_mesh=True)
    with pytest.raises(ValueError):                                  # ... for another n
        rom.pod_rbf_run_long(X6, np.ones(600), mu1, mu2, 0.05, 1, *cl6, plan=p16)
    with pytest.raises(ValueError):                                  # ... for the other entry point
        rom.pod_rbf_run_long(X6, np.ones(600), mu1, mu2, 0.05, 1, *cl6, plan=rom.RbfFusedPlan(*cl6, "gaussian", dev))
    with pytest.raises(ValueError):
        rom.pod_rbf_run_fused(X6, np.ones(600), mu1, mu2, 0.05, 1, *cl6, plan=p6)
    # a closure beyond the limits (nbar = 130): no device loop, and pod_rbf_run(fused=True, long_mesh=True) takes the host path
    Up, Us, Xt, W, eps, x_min, x_max, y_min, y_max = cl6
    ext = (Up, np.concatenate([Us, Us[:, :51]], 1), Xt, np.concatenate([W, np.zeros((300, 51))], 1), eps, x_min, x_max,
           np.concatenate([y_min, np.zeros(51)]), np.concatenate([y_max, np.zeros(51)]))
    assert rom.pod_rbf_run_long(X6, np.ones(600), mu1, mu2, 0.05, 1, *ext) is None
    assert rom.pod_rbf_run(X6, np.ones(600), mu1, mu2, 0.05, 1, *ext, fused=True, long_mesh=True).path == "host"
    # a mesh bg_rbf_rom_run covers: the long plan declines it, and long_mesh=True changes nothing
    g = load_golden("rbf_n17.npz")
    X5, _ = mesh(512)
    cl5 = (g["U_p"], g["U_s"], g["X_train"], g["W_gaussian"], float(g["eps_gaussian"]), g["x_min"], g["x_max"], g["y_min"],
           g["y_max"])
    assert not rom.RbfFusedPlan(*cl5, "gaussian", dev, long_mesh=True).ok
    assert rom.pod_rbf_run_long(X5, np.ones(512), mu1, mu2, 0.05, 2, *cl5) is None
    with_flag = rom.pod_rbf_run(X5, np.ones(512), mu1, mu2, 0.05, 2, *cl5, fused=True, long_mesh=True)
    without = rom.pod_rbf_run(X5, np.ones(512), mu1, mu2, 0.05, 2, *cl5, fused=True)
    torch.cuda.synchronize()
    assert with_flag.path == "bg_rbf_rom_run" and without.path == "bg_rbf_rom_run"
    assert torch.equal(with_flag.hist, without.hist) and torch.equal(with_flag.iters, without.iters)
    assert torch.equal(with_flag.flags, without.flags)


def test_facade(hip):
    from fem_burgers import FEMBurgers
    name = "n1024-imq-lspg"
    X, mus, dt, steps, E, cl, kw = rc.case_inputs(name)
    fem = FEMBurgers(*mesh(1024))
    U = fem.pod_rbf_prom(dt, steps, np.ones(1024), mus[0][0], E, mus[0][1], *cl, projection=kw["projection"],
                         kernel=kw["kernel"], tol_newton=1e-6, max_newton=kw["max_newton"], fused=True, long_mesh=True)
    assert U.shape == (1024, steps + 1) and rel_l2(U, rc.oracle_run(name)[0][0]) < TOL
