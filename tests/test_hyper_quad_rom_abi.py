"""CPU-side checks of bg_hyper_quad_rom_run (the hyper-reduced quadratic-manifold loop on sampled mesh rows): the limits and
sizes it reports, the argument validation that happens before anything is launched and its order, what rom.HyperQuadPlan
refuses before it touches a device, and that nothing routes to the loop unless asked."""
import ctypes

import numpy as np
import pytest

from loop_cases import built_library, host_pointers


@pytest.fixture(scope="module")
def L():
    return built_library()


def test_limits_and_sizes(L):
    from burgers_hip import lib, pod
    out = [ctypes.c_int(-1) for _ in range(3)]
    assert L.bg_hyper_quad_rom_limits(*[ctypes.byref(v) for v in out]) == 0
    assert tuple(v.value for v in out) == (40, 256, 768)
    assert lib.limits("bg_hyper_quad_rom_limits", 3) == pod.hyper_quad_rom_limits() == (40, 256, 768)
    assert L.bg_hyper_quad_rom_limits(None, None, None) == 0
    groups = lambda nodes: (nodes + 3) // 4
    for nodes, covered in ((0, False), (1, True), (512, True), (513, True), (768, True), (769, False), (-1, False)):
        assert L.bg_hyper_quad_rom_workgroups_per_cu(nodes) == (1 if covered else 0), nodes
        assert L.bg_hyper_quad_rom_phif_elems(nodes) == (groups(nodes) * 10 * 16 if covered else 0), nodes
        assert L.bg_hyper_quad_rom_h3f_elems(nodes) == (groups(nodes) * 28 * 64 * 2 if covered else 0), nodes
    # the operand copies are bg_quad_rom_run's, the table in place of the mesh
    assert L.bg_hyper_quad_rom_phif_elems(181) == L.bg_quad_rom_phif_elems(181)
    assert L.bg_hyper_quad_rom_h3f_elems(181) == L.bg_quad_rom_h3f_elems(181)


def test_argument_validation_before_launch_and_its_order(L):
    from burgers_hip import lib
    null = None
    p, ip = host_pointers()
    buf = (ctypes.c_double * 8)()
    aligned = (ctypes.addressof(buf) + 15) & ~15
    dp = lambda addr: ctypes.cast(addr, ctypes.POINTER(ctypes.c_double))

    def run(N=2049, B=4, n=40, m=120, nodes=181, nsteps=2, proj=lib.BG_PROJ_GALERKIN, dt=0.0125, max_it=25, idx=ip, ops=p,
            h3f=None, hist=p, outs=ip):
        h3f = dp(aligned) if h3f is None else h3f
        return L.bg_hyper_quad_rom_run(N, B, n, m, nodes, nsteps, proj, ops, idx, idx, ops, ops, h3f, ops, ops, ops, ops,
                                       dt, 0.0, 1e-6, max_it, 0, hist, outs, outs, outs, null, null)

    for bad in (dict(N=2), dict(n=0), dict(m=0), dict(nodes=0), dict(nsteps=-1), dict(max_it=0), dict(dt=0.0), dict(B=-1)):
        assert run(**bad) == lib.BG_ERR_BAD_ARG, bad
    assert run(proj=9) == lib.BG_ERR_PROJECTION
    assert run(N=L.bg_fom_max_n() + 1) == lib.BG_ERR_UNSUPPORTED_N
    assert run(N=L.bg_fom_max_n(), B=0) == lib.BG_OK               # the whole range of the FOM is covered
    assert run(N=3, m=3, nodes=3, B=0) == lib.BG_OK
    assert run(m=256, nodes=768, B=0) == lib.BG_OK                 # both limits at once
    assert run(n=41) == lib.BG_ERR_UNSUPPORTED_R
    assert run(m=257, nodes=257) == lib.BG_ERR_UNSUPPORTED_R
    assert run(m=256, nodes=769) == lib.BG_ERR_UNSUPPORTED_R
    assert run(N=100, m=101, nodes=101) == lib.BG_ERR_BAD_ARG      # more rows than the mesh has
    assert run(N=150, m=120, nodes=151) == lib.BG_ERR_BAD_ARG      # more table nodes than the mesh has
    assert run(m=120, nodes=119) == lib.BG_ERR_BAD_ARG             # every sampled row is a table node ...
    assert run(m=120, nodes=361) == lib.BG_ERR_BAD_ARG             # ... and brings at most two neighbours
    # the order: bad arguments, projection, mesh, limits, the table's shape
    assert run(N=2, proj=9) == lib.BG_ERR_BAD_ARG
    assert run(proj=9, N=L.bg_fom_max_n() + 1, n=41) == lib.BG_ERR_PROJECTION
    assert run(N=L.bg_fom_max_n() + 1, n=41, m=300, nodes=200) == lib.BG_ERR_UNSUPPORTED_N
    assert run(n=41, m=120, nodes=119) == lib.BG_ERR_UNSUPPORTED_R
    assert run(N=200, m=257, nodes=300) == lib.BG_ERR_UNSUPPORTED_R
    assert run(m=120, nodes=119, B=0) == lib.BG_ERR_BAD_ARG        # the shape is checked for an empty batch too
    assert run(h3f=dp(aligned + 8)) == lib.BG_ERR_BAD_ARG          # H3f not 16-byte aligned
    assert run(ops=null) == lib.BG_ERR_BAD_ARG                     # null operands, B > 0
    assert run(idx=null) == lib.BG_ERR_BAD_ARG
    assert run(hist=null) == lib.BG_ERR_BAD_ARG                    # null outputs, B > 0
    assert run(outs=null) == lib.BG_ERR_BAD_ARG
    assert run(B=0, idx=null, ops=null, h3f=dp(0), hist=null, outs=null) == lib.BG_OK     # empty batch: no pointer is looked at


def test_existing_limits_and_routes_are_unchanged(L):
    from burgers_hip import lib, rom
    assert L.bg_abi_version() == 1
    assert L.bg_quad_rom_max_n() == 40 and L.bg_quad_rom_run_long_max_n() == 1024 and L.bg_quad_rom_run_long_max_r() == 40
    assert lib.limits("bg_hyper_rom_limits", 2) == (40, 256)
    r = rom._ROUTES["bg_hyper_quad_rom_run"]
    assert r.min_n == 3 and rom._limit(r.max_n) == L.bg_fom_max_n() and rom._limit(r.max_r) == 40
    assert r.group == 4 and not r.supg and rom._limit(r.wg_per_cu) == 1
    # quadratic_run without hyper= resolves to the routes it resolved to
    assert rom._quad_route(512, 40) == "bg_quad_rom_run" and rom._quad_route(513, 40) == "host"
    assert rom._quad_route(1024, 40, long_mesh=True) == "bg_quad_rom_run_long" and rom._quad_route(512, 40, long_mesh=True) == "bg_quad_rom_run"
    assert rom._quad_route(1025, 40, long_mesh=True) == "host" and rom._quad_route(2049, 40) == "host"
    assert rom._quad_route(256, 41) == "host" and rom._quad_route(256, 40, fused=False) == "host"


def test_quadratic_run_without_hyper_never_reaches_the_hyper_loop(L, monkeypatch):
    """``hyper=None`` (the default) goes on to the routes of _quad_route; only a sampling or a plan reaches quadratic_run_hyper."""
    from burgers_hip import lib, rom
    seen = []
    monkeypatch.setattr(rom, "quadratic_run_hyper", lambda *a, **k: seen.append("hyper") or (_ for _ in ()).throw(KeyError("hyper")))
    monkeypatch.setattr(lib, "require_device", lambda d: (_ for _ in ()).throw(KeyError("routes")))
    X = np.linspace(0.0, 100.0, 64)
    Phi, H = np.zeros((64, 3)), np.zeros((64, 6))
    with pytest.raises(KeyError, match="routes"):
        rom.quadratic_run(X, np.ones(64), 4.5, 0.02, 0.05, 2, Phi, H)
    assert seen == []
    with pytest.raises(KeyError, match="hyper"):
        rom.quadratic_run(X, np.ones(64), 4.5, 0.02, 0.05, 2, Phi, H, hyper=object())
    assert seen == ["hyper"]


def test_plan_refuses_before_the_device(L):
    """Without a device a plan that reached its device copy raises RuntimeError: ValueError means the checks came first."""
    import torch
    from burgers_hip import pod, rom
    N, n = 600, 5
    k = n * (n + 1) // 2
    X = np.linspace(0.0, 100.0, N)
    rng = np.random.default_rng(3)
    U = np.linalg.qr(rng.standard_normal((N, n + k)))[0]
    Phi, H = U[:, :n], 0.3 * U[:, n:]                              # Phi^T Phi = I, Phi^T H = 0
    samp = lambda rows, xi=None, proj="lspg": pod.RowSampling(np.asarray(rows, dtype=np.int32),
                                                              np.ones(len(rows)) if xi is None else xi, proj, 0.0, 0, 0.0)
    good = samp([0, 7, 8, 300, 599])
    wide = np.linalg.qr(rng.standard_normal((N, 41)))[0]
    bad = [
        (Phi[:, 0], H, good), (Phi, H[:-1], good), (Phi, H[:, :-1], good), (Phi[:, :0], H[:, :0], good),       # shapes
        (wide, np.zeros((N, 41 * 42 // 2)), good),                                                     # n beyond the limit
        (1.001 * Phi, H, good), (Phi + 1e-6, H, good),                                                 # Phi not orthonormal to 1e-8
        (Phi, H + 1e-6 * Phi[:, :1], good),                                                            # Phi^T H beyond 1e-8
        (Phi, np.where(np.arange(k) == 0, np.nan, H), good),                                           # not finite
        (Phi, H, samp([0, 8, 7, 300])), (Phi, H, samp([0, 7, 7, 300])),                                # not ascending, not distinct
        (Phi, H, samp([0, 7, 600])), (Phi, H, samp([-1, 7])), (Phi, H, samp([])),                      # outside the mesh, empty
        (Phi, H, samp([0, 7, 8], np.array([1.0, -0.5, 1.0]))),                                         # a negative weight
        (Phi, H, samp([0, 7, 8], np.array([1.0, np.nan, 1.0]))),                                       # a non-finite weight
        (Phi, H, samp([0, 7, 8], np.ones(2))),                                                         # one weight each
        (Phi, H, samp(np.arange(0, 2 * 257, 2))),                                                      # more rows than the loop takes
        (Phi, H, samp([0, 7, 8], proj="petrov")),                                                      # an unknown projection
    ]
    for c, (a, b, s) in enumerate(bad):
        with pytest.raises(ValueError):
            rom.HyperQuadPlan(a, b, s, X, None)
            pytest.fail(f"case {c} was accepted")
    with pytest.raises(ValueError, match="re-project"):
        rom.HyperQuadPlan(Phi, H + 1e-6 * Phi[:, :1], good, X, None)
    with pytest.raises(ValueError):
        rom.HyperQuadPlan(Phi, H, good, X[:-1], None)                                                  # another mesh length
    # 256 isolated rows bring 768 stencil nodes: both limits themselves (a table beyond 768 nodes cannot exist at m <= 256)
    X4, U4 = np.linspace(0.0, 100.0, 2049), np.linalg.qr(rng.standard_normal((2049, n + k)))[0]
    if not torch.cuda.is_available():                                     # a plan that passes goes on to the device
        with pytest.raises(RuntimeError):
            rom.HyperQuadPlan(Phi, H, good, X, None)
        with pytest.raises(RuntimeError):
            rom.HyperQuadPlan(U4[:, :n], U4[:, n:], samp(np.arange(1, 4 * 256, 4)), X4, None)          # both limits at once
