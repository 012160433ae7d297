"""The device-side POD-ANN time loop for up to 20 primary modes (bg_ann_rom_run_wide, rom.pod_ann_run_wide,
csrc/rom_ann_wide.hip) against the reference's live fixture, bg_ann_rom_run on the models both take, the host-driven batched
path and the oracle.  reference: FEM/fem_burgers.py:1177-1275.  The closure is evaluated in float32 like the reference's,
so every comparison is float32-limited: the gate and the count rules are those of tests/test_ann_fused_gpu.py.  The cases
and why they are what they are: tests/ann_wide_cases.py; their conditioning: tests/test_ann_wide_rom_abi.py."""
import numpy as np
import pytest
import torch

import ann_wide_cases as aw
from ann_wide_cases import TOL32, WIDE
from conftest import load_golden, mesh, rel_l2
from loop_cases import draw, same, to_np

pytestmark = pytest.mark.gpu


def _golden_model(g):
    import torch.nn as nn
    dims = [5, 32, 64, 128, 256, 256, 91]
    layers = []
    for i in range(6):
        lin = nn.Linear(dims[i], dims[i + 1])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(g[f"W{i}"])); lin.bias.copy_(torch.from_numpy(g[f"b{i}"]))
        layers.append(lin)
        if i < 5:
            layers.append(nn.ELU())
    return nn.Sequential(*layers).eval()


def _worst_per_sample(a, b):
    d, h = a.hist.flatten(1), b.hist.flatten(1)
    return float(((d - h).norm(dim=1) / h.norm(dim=1)).max())


def test_live_reference_through_the_wide_loop(hip):
    """The fixture recorded from the reference's own pod_ann_prom run (n = 5), through the new kernel."""
    from burgers_hip import rom
    g = load_golden("ann_n5.npz")
    X, _ = mesh(512)
    res = rom.pod_ann_run_wide(X, np.ones(512), float(g["mu1"]), float(g["mu2"]), float(g["At"]), int(g["nT"]),
                               g["U_p"], g["U_s"], _golden_model(g), rom.PROJ["lspg"])
    torch.cuda.synchronize()
    assert res.path == WIDE and int(res.info.abs().max()) == 0
    err = rel_l2(to_np(res.hist[0]).T, g["U"])
    print(f"live reference, n = 5: rel-L2 {err:.2e}")
    assert err < TOL32


def _old_against_new(X, Up, Us, model, proj, E, B=40, nT=6):
    from burgers_hip import rom
    mu1, mu2 = draw(B, seed=11)
    N = len(X)
    old = rom.pod_ann_run_fused(X, np.ones(N), mu1, mu2, 0.05, nT, Up, Us, model, rom.PROJ[proj], E=E)
    new = rom.pod_ann_run_wide(X, np.ones(N), mu1, mu2, 0.05, nT, Up, Us, model, rom.PROJ[proj], E=E)
    torch.cuda.synchronize()
    assert old.path == "bg_ann_rom_run" and new.path == WIDE
    assert int(new.info.abs().max()) == 0 and torch.equal(old.flags, new.flags)
    d = (old.iters - new.iters).abs()
    worst = _worst_per_sample(new, old)
    print(f"n = {Up.shape[1]} {proj}: worst rel-L2 old against new {worst:.2e}, steps with another count {int((d > 0).sum())}")
    assert int(d.max()) <= 1 and worst < TOL32


@pytest.mark.parametrize("proj", ["lspg", "galerkin"])
def test_old_against_new_at_n_up_to_8(hip, proj):
    """bg_ann_rom_run and bg_ann_rom_run_wide on identical inputs: the committed n = 5 model, and n = 8 (the old limit)."""
    g = load_golden("ann_n5.npz")
    X, _ = mesh(512)
    _old_against_new(X, g["U_p"], g["U_s"], _golden_model(g), proj, 0.0)
    X8, Up, Us = aw.case_bases(aw.CASE_N8)
    _old_against_new(X8, Up, Us, aw.case_model(aw.CASE_N8), proj, aw.CASE_N8[9])


@pytest.mark.parametrize("proj", ["LSPG", "Galerkin"])
def test_thesis_size_against_host_path_and_oracle(hip, proj):
    """Case A (n = 17, nbar = 79, the reference's second model size) at scale 3.0, where a wrong tangent row moves the
    history by ten times the gate; more samples than workgroups."""
    from burgers_hip import rom
    X, Up, Us = aw.case_bases(aw.CASE_A)
    model = aw.case_model(aw.CASE_A)
    B, nT = 300, 6
    mu1, mu2 = draw(B, seed=11)
    f = rom.pod_ann_run(X, np.ones(512), mu1, mu2, 0.05, nT, Up, Us, model, projection=proj, wide=True)
    b = rom.pod_ann_run(X, np.ones(512), mu1, mu2, 0.05, nT, Up, Us, model, projection=proj, fused=False)
    torch.cuda.synchronize()
    assert f.path == WIDE and b.path == "host"
    assert int(f.info.abs().max()) == 0
    assert torch.equal(f.flags, b.flags) and not bool(f.flags.any())
    fi, bi = to_np(f.iters), to_np(b.iters)
    worst = _worst_per_sample(f, b)
    print(f"case A {proj}: worst rel-L2 against the host path {worst:.2e}, steps with another count {(fi != bi).mean():.4f}")
    assert np.abs(fi - bi).max() <= 1 and (fi != bi).mean() < 0.02
    assert worst < TOL32
    fh = to_np(f.hist)
    for s in (0, 77, 299):
        Uo, ito = aw.oracle(aw.CASE_A, mu1[s], mu2[s], nT, proj)
        err = rel_l2(fh[s].T, Uo)
        print(f"case A {proj} sample {s}: rel-L2 against the oracle {err:.2e}, iterations {fi[s].tolist()} / {ito.tolist()}")
        assert err < TOL32 and np.abs(fi[s] - ito).max() <= 1


@pytest.mark.parametrize("case", aw.SHAPE_CASES, ids=[c[0] for c in aw.SHAPE_CASES])
def test_shapes_activations_and_limits(hip, case):
    """Both row tilings (N <= 256 / <= 512), ragged and odd N, every activation, no-bias layers, the limits n = 20,
    nbar = 128, width 256, 8 layers, all three row counts the closure is compiled for (n = 9, 12 / 13 / 17, 20).  Against the
    host-driven path and (one clean sample, ELU) the oracle; the assertions of test_ann_fused_shapes_and_activations."""
    from burgers_hip import rom
    name, N, n, nbar, hidden, act, bias, seed, scale, E = case
    X, Up, Us = aw.case_bases(case)
    model = aw.case_model(case)
    B, nT = 19, 5
    mu1, mu2 = draw(B, seed=n)
    for proj in ("LSPG", "Galerkin"):
        f = rom.pod_ann_run(X, np.ones(N), mu1, mu2, 0.05, nT, Up, Us, model, projection=proj, E=E, wide=True)
        b = rom.pod_ann_run(X, np.ones(N), mu1, mu2, 0.05, nT, Up, Us, model, projection=proj, E=E, fused=False)
        torch.cuda.synchronize()
        assert f.path == WIDE and b.path == "host"
        fi, bi = to_np(f.iters), to_np(b.iters)
        assert np.abs(fi - bi).max() <= 1
        assert int((f.flags != b.flags).sum().item()) <= 1, (proj, f.flags.tolist(), b.flags.tolist())
        ok = to_np((f.flags == 0) & (b.flags == 0))
        assert ok.mean() >= 0.8, (proj, f.flags.tolist())
        fh, bh = to_np(f.hist), to_np(b.hist)
        errs = [rel_l2(fh[s], bh[s]) for s in np.flatnonzero(ok)]
        print(f"{name} {proj}: worst rel-L2 against the host path {max(errs):.2e}")
        assert max(errs) < TOL32, proj
        if act == "ELU":
            s = int(np.flatnonzero(ok)[0])
            Uo, ito = aw.oracle(case, mu1[s], mu2[s], nT, proj)
            err = rel_l2(fh[s].T, Uo)
            print(f"{name} {proj} sample {s}: rel-L2 against the oracle {err:.2e}")
            assert err < TOL32 and np.abs(fi[s] - ito).max() <= 1


def test_nonuniform_mesh(hip):
    from burgers_hip import rom
    _, Up, Us = aw.case_bases(aw.CASE_A)
    X = aw.nonuniform_mesh()
    mu1 = np.array([4.4, 5.2]); mu2 = np.array([0.017, 0.026])
    f = rom.pod_ann_run(X, np.ones(512), mu1, mu2, 0.05, 5, Up, Us, aw.case_model(aw.CASE_A), wide=True)
    torch.cuda.synchronize()
    assert f.path == WIDE
    for s in range(2):
        Uo, _ = aw.oracle(aw.CASE_A, mu1[s], mu2[s], 5, "LSPG", X=X)
        err = rel_l2(to_np(f.hist[s]).T, Uo)
        print(f"perturbed mesh, sample {s}: rel-L2 against the oracle {err:.2e}")
        assert err < TOL32


def test_edge_cases(hip):
    """nsteps = 0 and B = 0 are no-ops that still fill hist[:, 0]; a run in two halves equals the run in one; order entries
    outside [0, B) are skipped; the balanced order changes no bit."""
    from burgers_hip import lib, rom
    X, Up, Us = aw.case_bases(aw.CASE_A)
    model = aw.case_model(aw.CASE_A)
    p = rom.PROJ["lspg"]
    run = lambda u0, mu1, mu2, nT, **kw: rom.pod_ann_run_wide(X, u0, mu1, mu2, 0.05, nT, Up, Us, model, p, **kw)
    r = run(np.ones(512), [4.5], [0.02], 0)
    torch.cuda.synchronize()
    assert r.path == WIDE and r.hist.shape == (1, 1, 512) and float((r.hist - 1.0).abs().max()) == 0.0
    r = run(np.ones(512), np.zeros(0), np.zeros(0), 3)
    assert r.path == WIDE and r.hist.shape == (0, 4, 512)
    # restart: the second half of a run from the state the first half ended in
    mu1, mu2 = draw(6, seed=9)
    whole = run(np.ones(512), mu1, mu2, 5)
    head = run(np.ones(512), mu1, mu2, 2)
    tail = run(to_np(head.hist[:, -1]), mu1, mu2, 3)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([head.hist, tail.hist[:, 1:]], 1), whole.hist)
    assert torch.equal(torch.cat([head.iters, tail.iters], 1), whole.iters)
    # the raw entry with two entries of ``order`` outside [0, B)
    ref = run(np.ones(512), mu1, mu2, 3)
    plan, UT = ref._keep[-2], ref._keep[-1]
    dev, B = ref.hist.device, 6
    u0d = torch.ones((B, 512), dtype=torch.float64, device=dev)
    mu1d, mu2d, Xd = torch.as_tensor(mu1, device=dev), torch.as_tensor(mu2, device=dev), torch.as_tensor(X, device=dev)
    hist = torch.full((B, 4, 512), -7.0, dtype=torch.float64, device=dev)
    iters = torch.zeros((B, 3), dtype=torch.int32, device=dev)
    flags = torch.full((B,), -3, dtype=torch.int32, device=dev)
    info = torch.zeros((B,), dtype=torch.int32, device=dev)
    order = torch.arange(B, dtype=torch.int32, device=dev)
    order[1], order[4] = -1, B + 5
    rc = lib.load().bg_ann_rom_run_wide(512, B, 17, 79, 3, p, lib.ptr(Xd), lib.ptr(UT), lib.ptr(u0d), lib.ptr(mu1d),
                                        lib.ptr(mu2d), *plan.args, 0.05, 0.0, 1e-6, 50, lib.mesh_options(X, supg=True),
                                        lib.ptr(hist), lib.ptr(iters), lib.ptr(flags), lib.ptr(info), lib.ptr(order),
                                        lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    keep = [0, 2, 3, 5]
    assert torch.equal(hist[keep], ref.hist[keep]) and torch.equal(iters[keep], ref.iters[keep])
    assert torch.equal(flags[keep], ref.flags[keep]) and bool((info == 0).all())
    assert bool((hist[[1, 4]] == -7.0).all()) and bool((flags[[1, 4]] == -3).all())
    # the balanced sample order is a scheduling decision only (more samples than workgroups)
    mu1, mu2 = draw(600, seed=4)
    a = run(np.ones(512), mu1, mu2, 2)
    b = run(np.ones(512), mu1, mu2, 2, balance=False)
    torch.cuda.synchronize()
    same(a, b)


@pytest.mark.parametrize("proj", ["lspg", "galerkin"])
def test_no_tangent_reuse_option_changes_no_bit(hip, proj):
    """BG_OPT_NO_TANGENT_REUSE is accepted; this loop evaluates the closure at every step start either way."""
    from burgers_hip import rom
    X, Up, Us = aw.case_bases(aw.CASE_A)
    model = aw.case_model(aw.CASE_A)
    mu1, mu2 = draw(200, seed=3)
    a = rom.pod_ann_run_wide(X, np.ones(512), mu1, mu2, 0.05, 12, Up, Us, model, rom.PROJ[proj])
    b = rom.pod_ann_run_wide(X, np.ones(512), mu1, mu2, 0.05, 12, Up, Us, model, rom.PROJ[proj],
                             options=hip.BG_OPT_NO_TANGENT_REUSE)
    torch.cuda.synchronize()
    assert a.path == WIDE and b.path == WIDE
    same(a, b)


def test_facade(hip):
    """FEMBurgers.pod_ann_prom(wide=True): an (N, nT + 1) array for scalar parameters, the batched result's sample."""
    from burgers_hip import rom
    from fem_burgers import FEMBurgers
    X, Up, Us = aw.case_bases(aw.CASE_A)
    _, T = mesh(512)
    model = aw.case_model(aw.CASE_A)
    U = FEMBurgers(X, T).pod_ann_prom(0.05, 4, np.ones(512), 4.56, 0.0, 0.019, Up, Us, model, wide=True)
    res = rom.pod_ann_run(X, np.ones(512), [4.4, 4.56], [0.02, 0.019], 0.05, 4, Up, Us, model, wide=True)
    torch.cuda.synchronize()
    assert res.path == WIDE and isinstance(U, np.ndarray) and U.shape == (512, 5)
    assert np.array_equal(U, to_np(res.hist[1]).T)
