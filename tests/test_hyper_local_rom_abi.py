"""CPU-side checks of bg_hyper_local_rom_run (the hyper-reduced local POD loop on sampled mesh rows): the limits and sizes it
reports, the argument validation that happens before anything is launched and its order, the route's fields, what
rom.HyperLocalPlan refuses before it touches a device, and that nothing routes to the loop unless asked."""
import ctypes

import numpy as np
import pytest

from loop_cases import built_library, host_pointers


@pytest.fixture(scope="module")
def L():
    return built_library()


def test_limits_and_sizes(L):
    from burgers_hip import lib, pod
    out = [ctypes.c_int(-1) for _ in range(4)]
    assert L.bg_hyper_local_rom_limits(*[ctypes.byref(v) for v in out]) == 0
    assert tuple(v.value for v in out) == (40, 256, 64, 64)
    assert lib.limits("bg_hyper_local_rom_limits", 4) == pod.hyper_local_rom_limits() == (40, 256, 64, 64)
    assert L.bg_hyper_local_rom_limits(None, None, None, None) == 0
    for C, m, covered in ((1, 1, True), (11, 121, True), (64, 256, True), (0, 5, False), (65, 5, False), (3, 0, False), (3, 257, False),
                          (-1, 5, False)):
        want = C * ((m + 31) // 32 * 32) * 3 * 42 if covered else 0
        assert L.bg_hyper_local_rom_table_elems(C, m) == want, (C, m)
    # block c of the stack is bg_hyper_rom_run's table of cluster c's basis
    assert L.bg_hyper_local_rom_table_elems(1, 121) == L.bg_hyper_rom_table_elems(121, 40)
    assert L.bg_hyper_local_rom_table_elems(7, 33) == 7 * L.bg_hyper_rom_table_elems(33, 8)


def test_argument_validation_before_launch_and_its_order(L):
    from burgers_hip import lib
    null = None
    p, ip = host_pointers()
    buf = (ctypes.c_double * 8)()
    aligned = (ctypes.addressof(buf) + 15) & ~15
    dp = lambda addr: ctypes.cast(addr, ctypes.POINTER(ctypes.c_double))

    def run(N=2049, B=4, C=11, rmax=40, mg=12, m=120, nsteps=2, proj=lib.BG_PROJ_GALERKIN, dt=0.0125, max_it=20, idx=ip, ops=p,
            table=None, hist=p, outs=ip, clusters=ip):
        table = dp(aligned) if table is None else table
        return L.bg_hyper_local_rom_run(N, B, C, rmax, mg, m, nsteps, proj, idx, ops, ops, table, idx, ops, ops, ops, ops, ops, ops,
                                        ops, ops, dt, 0.0, 1e-6, max_it, lib.BG_OPT_SUPG, hist, outs, outs, outs, clusters, null, null)

    for bad in (dict(N=2), dict(C=0), dict(rmax=0), dict(mg=0), dict(m=0), dict(nsteps=-1), dict(max_it=0), dict(dt=0.0),
                dict(B=-1)):
        assert run(**bad) == lib.BG_ERR_BAD_ARG, bad
    assert run(proj=9) == lib.BG_ERR_PROJECTION
    assert run(N=L.bg_fom_max_n() + 1) == lib.BG_ERR_UNSUPPORTED_N
    assert run(N=L.bg_fom_max_n(), B=0) == lib.BG_OK               # the whole range of the FOM is covered
    assert run(N=3, m=3, B=0) == lib.BG_OK
    assert run(C=64, rmax=40, mg=64, m=256, B=0) == lib.BG_OK      # all four limits at once
    for beyond in (dict(rmax=41), dict(m=257), dict(mg=65), dict(C=65)):
        assert run(**beyond) == lib.BG_ERR_UNSUPPORTED_R, beyond
    assert run(N=100, m=101) == lib.BG_ERR_BAD_ARG                 # more rows than the mesh has
    # the order: bad arguments, projection, mesh, limits, m > N, the empty batch, the pointers
    assert run(N=2, proj=9) == lib.BG_ERR_BAD_ARG
    assert run(proj=9, N=L.bg_fom_max_n() + 1, rmax=41) == lib.BG_ERR_PROJECTION
    assert run(N=L.bg_fom_max_n() + 1, rmax=41, m=300) == lib.BG_ERR_UNSUPPORTED_N
    assert run(N=200, m=257) == lib.BG_ERR_UNSUPPORTED_R
    assert run(N=100, m=101, B=0) == lib.BG_ERR_BAD_ARG            # the sizes are checked for an empty batch too
    assert run(C=65, B=0) == lib.BG_ERR_UNSUPPORTED_R
    assert run(table=dp(aligned + 8)) == lib.BG_ERR_BAD_ARG        # PhiS not 16-byte aligned
    assert run(ops=null) == lib.BG_ERR_BAD_ARG                     # null operands, B > 0
    assert run(idx=null) == lib.BG_ERR_BAD_ARG
    assert run(table=dp(0)) == lib.BG_ERR_BAD_ARG
    assert run(hist=null) == lib.BG_ERR_BAD_ARG                    # null outputs, B > 0
    assert run(outs=null) == lib.BG_ERR_BAD_ARG
    assert run(nsteps=0, B=0, clusters=null) == lib.BG_OK
    assert run(B=0, idx=null, ops=null, table=dp(8), hist=null, outs=null, clusters=null) == lib.BG_OK     # empty batch: no pointer is looked at


def test_route_fields_and_existing_limits(L):
    from burgers_hip import lib, rom
    assert L.bg_abi_version() == 1
    r = rom._ROUTES["bg_hyper_local_rom_run"]
    assert r.min_n == 3 and rom._limit(r.max_n) == L.bg_fom_max_n() and rom._limit(r.wg_per_cu) == 2
    assert r.group == 1 and r.supg and not r.redo
    assert lib.limits("bg_hyper_rom_limits", 2) == (40, 256)
    assert lib.limits("bg_local_rom_run_long_limits", 4) == (1024, 40, 64, 64) and lib.limits("bg_local_rom_limits", 3) == (40, 64, 64)
    # local_prom_run without hyper= resolves to the routes it resolved to
    assert rom._local_route(512) == () and rom._local_route(512, fused=True) == ("bg_local_rom_run",)
    assert rom._local_route(1024, fused=True) == ("bg_local_rom_run",)
    assert rom._local_route(1024, fused=True, long_mesh=True) == ("bg_local_rom_run_long", "bg_local_rom_run")
    assert rom._local_route(512, fused=True, long_mesh=True) == ("bg_local_rom_run",)
    assert rom._local_route(2049, long_mesh=True) == ()


def test_local_prom_run_without_hyper_never_reaches_the_hyper_loop(L, monkeypatch):
    """``hyper=None`` (the default) goes on to the routes of _local_route; only a sampling or a plan reaches local_prom_run_hyper."""
    from burgers_hip import lib, rom
    seen = []
    monkeypatch.setattr(rom, "local_prom_run_hyper", lambda *a, **k: seen.append("hyper") or (_ for _ in ()).throw(KeyError("hyper")))
    monkeypatch.setattr(lib, "require_device", lambda d: (_ for _ in ()).throw(KeyError("routes")))
    X = np.linspace(0.0, 100.0, 64)
    cen, bases, Ug = np.zeros((2, 3)), {0: np.zeros((64, 2)), 1: np.zeros((64, 4))}, np.zeros((64, 3))
    for kw in (dict(), dict(fused=True), dict(fused=True, long_mesh=True)):
        with pytest.raises(KeyError, match="routes"):
            rom.local_prom_run(X, np.ones(64), 4.5, 0.02, 0.05, 2, cen, bases, Ug, 3, **kw)
    assert seen == []
    with pytest.raises(KeyError, match="hyper"):
        rom.local_prom_run(X, np.ones(64), 4.5, 0.02, 0.05, 2, cen, bases, Ug, 3, hyper=object())
    assert seen == ["hyper"]


def test_plan_refuses_before_the_device(L):
    """Without a device a plan that reached its device copy raises RuntimeError: ValueError means the checks came first."""
    import torch
    from burgers_hip import pod, rom
    N, mg = 600, 5
    X = np.linspace(0.0, 100.0, N)
    rng = np.random.default_rng(3)
    ortho = lambda w: np.linalg.qr(rng.standard_normal((N, w)))[0]
    cen, Ug = rng.standard_normal((3, mg)), ortho(8)
    bases = {0: ortho(4), 1: ortho(40), 2: ortho(9)}
    samp = lambda rows, xi=None, proj="lspg": pod.RowSampling(np.asarray(rows, dtype=np.int32),
                                                              np.ones(len(rows)) if xi is None else xi, proj, 0.0, 0, 0.0)
    good = samp([0, 7, 8, 300, 599])
    swap = lambda c, b: {**bases, c: b}
    plan = lambda cen=cen, bases=bases, Ug=Ug, mg=mg, s=good, X=X: rom.HyperLocalPlan(cen, bases, Ug, mg, s, X, None)
    bad = [
        dict(bases={0: bases[0], 2: bases[2]}),                                                   # a centre without a basis
        dict(bases=swap(1, np.zeros((N, 0)))), dict(bases=swap(1, ortho(41))),                    # width 0, width 41
        dict(bases=swap(2, 1.001 * bases[2])), dict(bases=swap(0, bases[0] + 1e-6)),              # not orthonormal to 1e-8
        dict(bases=swap(0, np.where(np.arange(4) == 0, np.nan, bases[0]))),                       # not finite
        dict(bases=swap(2, bases[2][:-1])), dict(bases=swap(2, bases[2][:, 0])),                  # shapes
        dict(s=samp([0, 8, 7, 300])), dict(s=samp([0, 7, 7, 300])),                               # not ascending, not distinct
        dict(s=samp([0, 7, 600])), dict(s=samp([-1, 7])), dict(s=samp([])),                       # outside the mesh, empty
        dict(s=samp([1, 7, 8])),                                                                  # row 0 is missing
        dict(s=samp([0, 7, 8], np.array([1.0, -0.5, 1.0]))),                                      # a negative weight
        dict(s=samp([0, 7, 8], np.array([1.0, np.nan, 1.0]))),                                    # a non-finite weight
        dict(s=samp([0, 7, 8], np.ones(2))),                                                      # one weight each
        dict(s=samp(np.arange(0, 2 * 257, 2))),                                                   # 257 rows
        dict(s=samp([0, 7, 8], proj="petrov")),                                                   # an unknown projection
        dict(cen=rng.standard_normal((3, 65)), Ug=ortho(70), mg=65),                              # 65 global modes
        dict(cen=cen[:, :4]), dict(Ug=Ug[:, :4]), dict(Ug=Ug[:-1]), dict(mg=0, cen=cen[:, :0]),   # shapes of the pick
        dict(cen=np.zeros((65, mg)), bases={c: bases[0] for c in range(65)}),                     # 65 centres
        dict(X=X[:-1]), dict(X=np.linspace(0.0, 100.0, N + 1)),                                   # another mesh length
    ]
    for c, kw in enumerate(bad):
        with pytest.raises(ValueError):
            plan(**kw)
            pytest.fail(f"case {c} was accepted")
    with pytest.raises(ValueError, match="re-project"):
        plan(bases=swap(2, 1.001 * bases[2]))
    with pytest.raises(ValueError, match="row 0"):
        plan(s=samp([1, 7, 8]))
    if not torch.cuda.is_available():                                     # a plan that passes goes on to the device
        with pytest.raises(RuntimeError):
            plan()
        with pytest.raises(RuntimeError):
            plan(s=samp(np.arange(0, 2 * 256, 2)), cen=np.zeros((64, 64)), Ug=ortho(64), mg=64,
                 bases={c: bases[1] for c in range(64)})                  # every limit at once
