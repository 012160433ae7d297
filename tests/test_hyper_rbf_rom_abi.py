"""CPU-side checks of bg_hyper_rbf_rom_run (the hyper-reduced POD-RBF loop on sampled mesh rows): the limits it reports, the
argument validation that happens before anything is launched, and what rom.HyperRbfPlan refuses before it touches a device."""
import ctypes

import numpy as np
import pytest

from loop_cases import built_library, host_pointers


@pytest.fixture(scope="module")
def L():
    return built_library()


def _limits(L):
    out = [ctypes.c_int(-1) for _ in range(5)]
    assert L.bg_hyper_rbf_rom_limits(*[ctypes.byref(v) for v in out]) == 0
    return tuple(v.value for v in out)


def test_limits_and_instantiations(L):
    from burgers_hip import lib, pod
    max_n, max_nbar, max_ns, max_m, max_nodes = _limits(L)
    assert (max_n, max_nbar, max_ns) == lib.limits("bg_rbf_rom_limits", 3) == (20, 128, 65536)     # the closure limits of bg_rbf_rom_run
    assert (max_m, max_nodes) == (256, 768) and max_nodes == 3 * max_m
    assert lib.limits("bg_hyper_rbf_rom_limits", 5) == pod.hyper_rbf_rom_limits() == (max_n, max_nbar, max_ns, max_m, max_nodes)
    assert L.bg_hyper_rbf_rom_limits(None, None, None, None, None) == 0
    table = {0: (0, 0), 1: (2, 512), 256: (2, 512), 257: (2, 512), 512: (2, 512), 513: (1, 1024), max_nodes: (1, 1024),
             max_nodes + 1: (0, 0), -1: (0, 0)}
    for nodes, (wg, ld) in table.items():
        assert (L.bg_hyper_rbf_rom_workgroups_per_cu(nodes), L.bg_hyper_rbf_rom_ut_ld(nodes)) == (wg, ld), nodes


def test_argument_validation_before_launch(L):
    from burgers_hip import lib
    max_n, max_nbar, max_ns, max_m, max_nodes = _limits(L)
    null = None
    p, ip = host_pointers()
    buf = (ctypes.c_double * 8)()                                   # 16-byte alignment is checked, the contents never read
    addr = (ctypes.addressof(buf) + 15) & ~15
    dp = lambda a: ctypes.cast(a, ctypes.POINTER(ctypes.c_double))

    def run(N=2049, B=4, n=17, nbar=79, Ns=300, m=200, nodes=241, nsteps=2, proj=lib.BG_PROJ_GALERKIN, kind=lib.BG_RBF_IMQ,
            dt=0.0125, max_it=30, idx=ip, ops=p, utn=dp(addr), wd=dp(addr), hist=p, outs=ip):
        return L.bg_hyper_rbf_rom_run(N, B, n, nbar, Ns, m, nodes, nsteps, proj, kind, idx, ops, idx, ops, utn, ops, wd, ops, ops,
                                      ops, 1.0, ops, ops, ops, ops, dt, 0.0, 1e-6, max_it, lib.BG_OPT_SUPG, hist, hist, outs, outs,
                                      outs, null, null)

    # (every call below is refused, or has B = 0: nothing is launched)
    for bad in (dict(N=2), dict(n=0), dict(nbar=0), dict(Ns=0), dict(m=0), dict(nodes=0), dict(nsteps=-1), dict(max_it=0),
                dict(dt=0.0), dict(B=-1)):
        assert run(B=bad.pop("B", 0), **bad) == lib.BG_ERR_BAD_ARG, bad
    assert run(kind=7, B=0) == lib.BG_ERR_BAD_ARG
    assert run(kind=7, proj=9, B=0) == lib.BG_ERR_BAD_ARG          # the kind is looked at before the projection
    assert run(proj=9, B=0) == lib.BG_ERR_PROJECTION
    assert run(proj=9, N=L.bg_fom_max_n() + 1, B=0) == lib.BG_ERR_PROJECTION      # ... the projection before the mesh
    assert run(N=L.bg_fom_max_n() + 1, B=0) == lib.BG_ERR_UNSUPPORTED_N
    assert run(N=L.bg_fom_max_n() + 1, n=max_n + 1, B=0) == lib.BG_ERR_UNSUPPORTED_N                # ... the mesh before the limits
    assert run(N=L.bg_fom_max_n(), B=0) == lib.BG_OK               # the whole range of the FOM is covered
    assert run(N=3, m=3, nodes=3, B=0) == lib.BG_OK
    assert run(m=max_m, nodes=max_nodes, B=0) == lib.BG_OK         # both limits at once
    assert run(n=max_n, nbar=max_nbar, Ns=max_ns, B=0) == lib.BG_OK
    assert run(m=max_m + 1, nodes=max_m + 1, B=0) == lib.BG_ERR_UNSUPPORTED_R
    assert run(m=max_m, nodes=max_nodes + 1, B=0) == lib.BG_ERR_UNSUPPORTED_R
    assert run(n=max_n + 1, B=0) == lib.BG_ERR_UNSUPPORTED_R
    assert run(nbar=max_nbar + 1, B=0) == lib.BG_ERR_UNSUPPORTED_R
    assert run(Ns=max_ns + 1, B=0) == lib.BG_ERR_UNSUPPORTED_R
    assert run(N=300, m=max_m + 1, nodes=301, B=0) == lib.BG_ERR_UNSUPPORTED_R                      # ... the limits before the table's shape
    assert run(N=100, m=101, nodes=101, B=0) == lib.BG_ERR_BAD_ARG  # more rows than the mesh has
    assert run(N=220, m=200, nodes=221, B=0) == lib.BG_ERR_BAD_ARG  # more table nodes than the mesh has
    assert run(m=200, nodes=199, B=0) == lib.BG_ERR_BAD_ARG        # every sampled row is a table node ...
    assert run(m=200, nodes=601, B=0) == lib.BG_ERR_BAD_ARG        # ... and brings at most two neighbours
    assert run(ops=null) == lib.BG_ERR_BAD_ARG                     # null operands, B > 0
    assert run(idx=null) == lib.BG_ERR_BAD_ARG
    assert run(utn=null) == lib.BG_ERR_BAD_ARG
    assert run(wd=null) == lib.BG_ERR_BAD_ARG
    assert run(hist=null) == lib.BG_ERR_BAD_ARG                    # null outputs, B > 0
    assert run(outs=null) == lib.BG_ERR_BAD_ARG
    assert run(utn=dp(addr + 8)) == lib.BG_ERR_BAD_ARG             # UTn not 16-byte aligned
    assert run(wd=dp(addr + 8)) == lib.BG_ERR_BAD_ARG              # Wd not 16-byte aligned
    assert run(B=0, idx=null, ops=null, utn=null, wd=null, hist=null, outs=null) == lib.BG_OK       # empty batch: nothing to do


def test_existing_limits_are_unchanged(L):
    from burgers_hip import lib
    assert L.bg_abi_version() == 1
    assert lib.limits("bg_rbf_rom_limits", 3) == (20, 128, 65536)
    assert lib.limits("bg_rbf_rom_run_long_limits", 4) == (1024, 20, 128, 65536)
    assert lib.limits("bg_hyper_ann_rom_limits", 6) == (8, 128, 256, 8, 256, 768)
    assert lib.limits("bg_hyper_rom_limits", 2) == (40, 256)
    assert L.bg_rom_max_n() == 512 and L.bg_fom_max_n() == 8192


def test_route_entry(L):
    from burgers_hip import rom
    r = rom._ROUTES["bg_hyper_rbf_rom_run"]
    assert r.min_n == 3 and rom._limit(r.max_n) == L.bg_fom_max_n() and r.supg and rom._limit(r.wg_per_cu) == 2
    assert rom._rbf_route(512) == () and rom._rbf_route(512, fused=True) == ("bg_rbf_rom_run",)       # the defaults stay
    assert rom._rbf_route(1024, fused=True, long_mesh=True) == ("bg_rbf_rom_run_long", "bg_rbf_rom_run")
    assert rom.HyperAnnRomResult is rom.HyperRbfRomResult          # one result implementation, both names


def test_plan_refuses_before_the_device(L):
    """Without a device a plan that reached its device copy raises RuntimeError: ValueError means the checks came first."""
    import torch
    from burgers_hip import pod, rom
    max_n, max_nbar, max_ns, max_m, _ = _limits(L)
    N, n, nbar, Ns = 600, 5, 20, 30
    rng = np.random.default_rng(3)
    X = np.linspace(0.0, 100.0, N)
    U = np.linalg.qr(rng.standard_normal((N, n + nbar)))[0]
    Up, Us = U[:, :n], U[:, n:]
    Xt, W = rng.uniform(-1.0, 1.0, (Ns, n)), rng.standard_normal((Ns, nbar))
    lo_x, hi_x, lo_y, hi_y = -np.ones(n), np.ones(n), -np.ones(nbar), np.ones(nbar)
    samp = lambda rows, xi=None, proj="lspg": pod.RowSampling(np.asarray(rows, dtype=np.int32),
                                                              np.ones(len(rows)) if xi is None else xi, proj, 0.0, 0, 0.0)
    good = samp([0, 7, 8, 300, 599])
    base = dict(U_p=Up, U_s=Us, X_train=Xt, W=W, epsilon=1.5, x_min=lo_x, x_max=hi_x, y_min=lo_y, y_max=hi_y, kernel="imq",
                sampling=good, X=X, device=None)
    wide = np.linalg.qr(rng.standard_normal((N, max_n + 1 + nbar)))[0]
    bad = [
        dict(U_p=Up[:, 0]), dict(U_s=Us[:-1]), dict(U_p=Up[:, :0]),                                        # shapes of the bases
        dict(X_train=Xt[:, :-1]), dict(W=W[:-1]), dict(W=W[:, :-1]), dict(X_train=Xt[:0], W=W[:0]),        # ... of the closure
        dict(x_min=lo_x[:-1]), dict(x_max=np.ones(n + 1)), dict(y_min=lo_y[:-1]), dict(y_max=np.ones((nbar, 1))),
        dict(U_p=wide[:, :max_n + 1], U_s=wide[:, max_n + 1:], X_train=np.zeros((Ns, max_n + 1)), x_min=-np.ones(max_n + 1),
             x_max=np.ones(max_n + 1)),                                                                  # n beyond the limit
        dict(sampling=samp([0, 8, 7, 300])), dict(sampling=samp([0, 7, 7, 300])),                          # not ascending, not distinct
        dict(sampling=samp([0, 7, 600])), dict(sampling=samp([-1, 7])), dict(sampling=samp([])),           # outside the mesh, empty
        dict(sampling=samp([0, 7, 8], np.array([1.0, -0.5, 1.0]))),                                        # a negative weight
        dict(sampling=samp([0, 7, 8], np.array([1.0, np.nan, 1.0]))),                                      # a non-finite weight
        dict(sampling=samp([0, 7, 8], np.ones(2))),                                                        # one weight each
        dict(sampling=samp(np.arange(0, 2 * (max_m + 1), 2))),                                             # more rows than the loop takes
        dict(sampling=samp([0, 7, 8], proj="petrov")),                                                     # an unknown projection
        dict(kernel="cubic"),                                                                              # an unknown kernel
        dict(U_s=1.001 * Us), dict(U_s=Us + 1e-6),                                                         # not orthonormal to 1e-8
        dict(X=X[:-1]),                                                                                    # another mesh length
    ]
    for k, change in enumerate(bad):
        with pytest.raises(ValueError):
            rom.HyperRbfPlan(**{**base, **change})
            pytest.fail(f"case {k} was accepted")
    many = max_ns + 1                                                        # more centres than the loop takes
    with pytest.raises(ValueError):
        rom.HyperRbfPlan(**{**base, "X_train": np.zeros((many, n)), "W": np.zeros((many, nbar))})
    if not torch.cuda.is_available():                                     # a plan that passes goes on to the device
        with pytest.raises(RuntimeError):
            rom.HyperRbfPlan(**base)
        with pytest.raises(RuntimeError):
            rom.HyperRbfPlan(**{**base, "sampling": samp(np.arange(0, 2 * max_m, 2))})                     # the row limit itself
        import hyper_rbf_ref as hrr
        Xc, _, cl = hrr.committed("imq")                                  # the committed bases are orthonormal to 1e-8
        with pytest.raises(RuntimeError):
            rom.HyperRbfPlan(*cl, "imq", samp([0, 100, 511]), Xc, None)
