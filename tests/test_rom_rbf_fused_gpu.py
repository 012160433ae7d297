"""The device-side POD-RBF time loop (bg_rbf_rom_run, rom.pod_rbf_run_fused) against the reference's live fixture, the
oracle and the host-driven batched iteration it replaces.  The closure weights reach 3.6e2, which amplifies rounding in
the decoder: tolerance 1e-9, as for the host path; iteration counts must be equal."""
import numpy as np
import pytest
import torch

from conftest import load_golden, mesh, rel_l2
from oracle import burgers_ref as br

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _closure(g, kernel="gaussian"):
    return (g["U_p"], g["U_s"], g["X_train"], g["W_" + kernel], float(g["eps_" + kernel]), g["x_min"], g["x_max"],
            g["y_min"], g["y_max"])


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("kernel,proj", [("gaussian", "LSPG"), ("imq", "Galerkin")])
def test_live_reference(hip, kernel, proj):
    from burgers_hip import rom
    g = load_golden("rbf_n17.npz")
    X, _ = mesh(512)
    cl = _closure(g, kernel)
    res = rom.pod_rbf_run_fused(X, np.ones(512), [float(g["mu1"]), 5.1], [float(g["mu2"]), 0.024], float(g["At"]),
                                int(g["nT"]), *cl, projection=proj, kernel=kernel, max_newton=20)
    torch.cuda.synchronize()
    assert res.path == "bg_rbf_rom_run"
    assert int(res.info.abs().sum()) == 0
    assert rel_l2(_np(res.hist[0]).T, g["U_" + kernel]) < TOL
    assert np.array_equal(_np(res.iters[0]), g["iters_" + kernel])
    Uo, ito = br.pod_rbf_prom(X, float(g["At"]), int(g["nT"]), np.ones(512), 5.1, 0.0, 0.024, *cl, projection=proj,
                              kernel=kernel, max_newton=20, return_iters=True)
    assert rel_l2(_np(res.hist[1]).T, Uo) < TOL and np.array_equal(_np(res.iters[1]), ito)


def test_matches_the_host_path_at_batch_size(hip):
    """The bench's (mu1, mu2) draw, B = 2048, 12 steps: per-sample parity with the host-driven iteration, the same
    iteration counts and the same flags -- the draw has samples that run into the 30-iteration cap."""
    import bench
    from burgers_hip import rom
    g = load_golden("rbf_n17.npz")
    X, _ = mesh(512)
    mu1, mu2 = bench.mu_shard(2048, 1, 0)
    cl = _closure(g)
    dev = rom.pod_rbf_run_fused(X, np.ones(512), mu1, mu2, 0.05, 12, *cl)
    host = rom.pod_rbf_run(X, np.ones(512), mu1, mu2, 0.05, 12, *cl, fused=False)
    torch.cuda.synchronize()
    assert dev.path == "bg_rbf_rom_run" and host.path == "host"
    assert int(dev.info.abs().sum()) == 0
    assert torch.equal(dev.iters, host.iters)
    assert torch.equal(dev.flags, host.flags)
    fl = _np(dev.flags)
    assert (fl & 1).any() and not (fl & 1).all()                      # capped and converged samples both present
    assert not (fl & 2).any()
    d, h = dev.hist.flatten(1), host.hist.flatten(1)
    worst = float(((d - h).norm(dim=1) / h.norm(dim=1)).max())
    assert worst < TOL, worst


@pytest.mark.parametrize("N", [512, 256])
def test_nonuniform_mesh_and_diffusion(hip, N):
    """Perturbed mesh (BG_OPT_NONUNIFORM) with E != 0; N = 256 takes the 4-rows-per-lane instantiation (every other node
    of the fixture's mesh and basis, the basis rescaled to stay orthonormal)."""
    from burgers_hip import rom
    g = load_golden("rbf_n17.npz")
    X, _ = mesh(512)
    step = 512 // N
    X = X[::step].copy()
    h = X[1] - X[0]
    rng = np.random.default_rng(N)
    X[1:-1] += rng.uniform(-0.2, 0.2, N - 2) * h
    Up, Us = g["U_p"][::step] * np.sqrt(step), g["U_s"][::step] * np.sqrt(step)
    cl = (Up, Us) + _closure(g, "imq")[2:]
    mu1, mu2, E = [4.6, 5.3], [0.018, 0.027], 0.02
    for proj in ("LSPG", "Galerkin"):
        res = rom.pod_rbf_run_fused(X, np.ones(N), mu1, mu2, 0.05, 4, *cl, projection=proj, kernel="imq", E=E)
        torch.cuda.synchronize()
        assert res.path == "bg_rbf_rom_run" and int(res.info.abs().sum()) == 0
        for b in range(2):
            Uo, ito = br.pod_rbf_prom(X, 0.05, 4, np.ones(N), mu1[b], E, mu2[b], *cl, projection=proj, kernel="imq",
                                      return_iters=True)
            assert rel_l2(_np(res.hist[b]).T, Uo) < TOL, (proj, b)
            assert np.array_equal(_np(res.iters[b]), ito), (proj, b)


def test_many_centres(hip):
    """About 2400 centres (eight jittered copies of X_train, weights divided by 8): the centres stream through LDS in
    19 tiles.  The closure itself is checked against the oracle first, then the trajectory and counts."""
    from burgers_hip import rom
    g = load_golden("rbf_n17.npz")
    rng = np.random.default_rng(7)
    Xt = np.concatenate([g["X_train"] + (0 if c == 0 else 1e-3) * rng.standard_normal(g["X_train"].shape) for c in range(8)])
    Wg = np.concatenate([g["W_gaussian"] / 8.0] * 8)
    assert Xt.shape[0] == 2400
    cl = (g["U_p"], g["U_s"], Xt, Wg, float(g["eps_gaussian"]), g["x_min"], g["x_max"], g["y_min"], g["y_max"])
    rbf = rom.RbfClosure(*cl[2:5], "gaussian", *cl[5:], torch.device("cuda", 0))
    qp = np.stack([g["qp_gaussian"], g["qp_gaussian"] * 0.97, g["qp_gaussian"] + 0.01])
    qd = torch.as_tensor(qp, device="cuda")
    val, jac = _np(rbf.value(qd)), _np(rbf.jacobian(qd))
    for b in range(3):
        vo = br.rbf_value(qp[b], *cl[2:5], "gaussian", *cl[5:])
        jo = br.rbf_jacobian(qp[b], *cl[2:5], "gaussian", *cl[5:])
        assert np.abs(val[b] - vo).max() < 1e-10 * max(1.0, np.abs(vo).max())
        assert np.abs(jac[b] - jo).max() < 1e-10 * max(1.0, np.abs(jo).max())
    X, _ = mesh(512)
    mu1, mu2 = [4.75, 5.2], [0.02, 0.016]
    res = rom.pod_rbf_run_fused(X, np.ones(512), mu1, mu2, 0.05, 4, *cl)
    torch.cuda.synchronize()
    assert res.path == "bg_rbf_rom_run" and res.plan.Ns == 2400
    for b in range(2):
        Uo, ito = br.pod_rbf_prom(X, 0.05, 4, np.ones(512), mu1[b], 0.0, mu2[b], *cl, return_iters=True)
        assert rel_l2(_np(res.hist[b]).T, Uo) < TOL and np.array_equal(_np(res.iters[b]), ito), b


def test_order_and_plans(hip):
    from burgers_hip import lib, rom
    g = load_golden("rbf_n17.npz")
    X, _ = mesh(512)
    rng = np.random.default_rng(3)
    B = 600                                                          # more samples than slots: balancing reorders them
    mu1, mu2 = rng.uniform(4.25, 5.5, B), rng.uniform(0.015, 0.03, B)
    cl = _closure(g)
    a = rom.pod_rbf_run_fused(X, np.ones(512), mu1, mu2, 0.05, 3, *cl, balance=True)
    b = rom.pod_rbf_run_fused(X, np.ones(512), mu1, mu2, 0.05, 3, *cl, balance=False)
    c = rom.pod_rbf_run_fused(X, np.ones(512), mu1, mu2, 0.05, 3, *cl, plan=a.plan)
    torch.cuda.synchronize()
    assert isinstance(a.plan, rom.RbfFusedPlan) and c.plan is a.plan
    for r in (b, c):
        assert torch.equal(a.hist, r.hist) and torch.equal(a.iters, r.iters) and torch.equal(a.flags, r.flags)
    # a plan for another mesh size or another n is refused before anything is launched
    X2, _ = mesh(256)
    with pytest.raises(ValueError):
        rom.pod_rbf_run_fused(X2, np.ones(256), mu1[:2], mu2[:2], 0.05, 1, g["U_p"][::2], *cl[1:], plan=a.plan)
    p16 = rom.RbfFusedPlan(g["U_p"][:, :16], g["U_s"], g["X_train"][:, :16], g["W_gaussian"], 1.0, g["x_min"][:16],
                           g["x_max"][:16], g["y_min"], g["y_max"], "gaussian", torch.device("cuda", 0))
    with pytest.raises(ValueError):
        rom.pod_rbf_run_fused(X, np.ones(512), mu1[:2], mu2[:2], 0.05, 1, *cl, plan=p16)
    with pytest.raises(ValueError):                                  # shapes that do not fit together
        rom.RbfFusedPlan(g["U_p"], g["U_s"][:, :50], *cl[2:], "gaussian", torch.device("cuda", 0))
    # a closure beyond bg_rbf_rom_limits (nbar = 130): no device loop, and pod_rbf_run(fused=True) takes the host path
    Us = np.concatenate([g["U_s"], g["U_s"][:, :51]], 1)
    W = np.concatenate([g["W_gaussian"], np.zeros((300, 51))], 1)
    ext = (g["U_p"], Us, g["X_train"], W, float(g["eps_gaussian"]), g["x_min"], g["x_max"],
           np.concatenate([g["y_min"], np.zeros(51)]), np.concatenate([g["y_max"], np.zeros(51)]))
    assert rom.pod_rbf_run_fused(X, np.ones(512), mu1[:2], mu2[:2], 0.05, 1, *ext) is None
    r = rom.pod_rbf_run(X, np.ones(512), mu1[:2], mu2[:2], 0.05, 1, *ext, fused=True)
    assert r.path == "host"
    # untrusted order entries: slots naming a sample outside [0, B) are skipped, the others run as usual
    plan = a.plan
    Xd = torch.as_tensor(X, device="cuda")
    u0 = torch.ones((4, 512), dtype=torch.float64, device="cuda")
    m1 = torch.as_tensor(mu1[:4], device="cuda"); m2 = torch.as_tensor(mu2[:4], device="cuda")
    hist = torch.zeros((4, 4, 512), dtype=torch.float64, device="cuda")
    iters = torch.zeros((4, 3), dtype=torch.int32, device="cuda")
    flags = torch.zeros((4,), dtype=torch.int32, device="cuda"); info = torch.zeros_like(flags)
    order = torch.as_tensor([1, 4, 0, -3], dtype=torch.int32, device="cuda")
    rc = lib.load().bg_rbf_rom_run(512, 4, plan.n, plan.nbar, plan.Ns, 3, lib.BG_PROJ_LSPG, plan.kind, lib.ptr(Xd),
                                   lib.ptr(plan.UT), lib.ptr(plan.XtT), lib.ptr(plan.Wd), lib.ptr(plan.bias), lib.ptr(plan.x_min),
                                   lib.ptr(plan.dx), plan.eps, lib.ptr(u0), lib.ptr(m1), lib.ptr(m2), 0.05, 0.0, 1e-6, 30,
                                   lib.BG_OPT_SUPG, lib.ptr(hist), lib.ptr(iters), lib.ptr(flags), lib.ptr(info),
                                   lib.ptr(order), lib.stream_ptr(torch.device("cuda", 0)))
    assert rc == lib.BG_OK
    torch.cuda.synchronize()
    assert torch.equal(hist[:2], a.hist[:2]) and torch.equal(iters[:2], a.iters[:2])
    assert not hist[2:].any() and not iters[2:].any()


def test_facade(hip):
    from fem_burgers import FEMBurgers
    g = load_golden("rbf_n17.npz")
    X, T = mesh(512)
    fem = FEMBurgers(X, T)
    args = (g["U_p"], g["U_s"], g["X_train"], g["W_gaussian"], float(g["eps_gaussian"]), g["x_min"], g["x_max"],
            g["y_min"], g["y_max"])
    U = fem.pod_rbf_prom(0.05, 4, np.ones(512), 4.75, 0.0, 0.02, *args, projection="LSPG", kernel="gaussian",
                         tol_newton=1e-6, max_newton=20, fused=True)
    assert U.shape == (512, 5) and rel_l2(U, g["U_gaussian"]) < TOL
    with pytest.raises(ValueError):
        fem.pod_rbf_prom(0.05, 1, np.ones(512), 4.75, 0.0, 0.02, *args[:3], g["W_imq"], 1.0, *args[5:],
                         kernel="multiquadric", fused=True)
