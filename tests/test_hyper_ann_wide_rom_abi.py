"""CPU-side checks of bg_hyper_ann_rom_run_wide (the hyper-reduced POD-ANN loop for up to 20 primary modes): the limits and
table properties it reports, the argument validation that happens before anything is launched, the route entry, and what
rom.HyperAnnWidePlan refuses before it touches a device."""
import ctypes

import numpy as np
import pytest

import ann_wide_cases as aw
import hyper_ann_wide_cases as hw
from loop_cases import built_library, host_pointers


@pytest.fixture(scope="module")
def L():
    return built_library()


def _limits(L):
    out = [ctypes.c_int(-1) for _ in range(6)]
    assert L.bg_hyper_ann_rom_wide_limits(*[ctypes.byref(v) for v in out]) == 0
    return tuple(v.value for v in out)


def test_limits_and_table_properties(L):
    from burgers_hip import lib, pod
    assert _limits(L) == hw.LIMITS
    assert _limits(L)[:4] == lib.limits("bg_ann_rom_run_wide_limits", 4)          # the closure limits of bg_ann_rom_run_wide
    assert lib.limits("bg_hyper_ann_rom_wide_limits", 6) == hw.LIMITS and pod.hyper_ann_wide_rom_limits() == hw.LIMITS
    assert L.bg_hyper_ann_rom_wide_limits(None, None, None, None, None, None) == 0
    max_nodes = hw.LIMITS[5]
    assert max_nodes >= 3 * hw.LIMITS[4]                                          # every sampling of max_m rows runs
    for nodes in (1, 2, 255, 256, 257, 511, 512, 513, max_nodes - 1, max_nodes):
        assert L.bg_hyper_ann_rom_wide_workgroups_per_cu(nodes) in (1, 2)
        ld = L.bg_hyper_ann_rom_wide_ut_ld(nodes)
        assert ld >= nodes and ld % 2 == 0                                        # a row holds the table; 16-byte rows
    for nodes in (-1, 0, max_nodes + 1, 1 << 20):
        assert L.bg_hyper_ann_rom_wide_workgroups_per_cu(nodes) == 0 and L.bg_hyper_ann_rom_wide_ut_ld(nodes) == 0


def test_argument_validation_before_launch(L):
    """Every row of test_hyper_ann_rom_abi.py's table, with n = 17."""
    from burgers_hip import lib
    max_n, max_nbar, max_w, max_l, max_m, max_nodes = _limits(L)
    null = None
    p, ip = host_pointers()
    fbuf = (ctypes.c_float * 64)()                                  # 16-byte alignment is checked, the contents never read
    faddr = (ctypes.addressof(fbuf) + 15) & ~15

    def run(N=2049, B=4, n=17, nbar=79, m=120, nodes=181, nsteps=2, proj=lib.BG_PROJ_GALERKIN, dt=0.0125, max_it=50, idx=ip, ops=p,
            hist=p, outs=ip, widths=None, layers=2, wt=faddr, acts=(lib.BG_ACT_ELU, lib.BG_ACT_NONE), model=True,
            options=lib.BG_OPT_SUPG):
        widths = (n, 32, nbar) if widths is None else widths
        mlp = (layers, (ctypes.c_int * len(widths))(*widths), (ctypes.c_void_p * layers)(*[wt] * layers),
               (ctypes.c_void_p * layers)(*[None] * layers), (ctypes.c_int * layers)(*acts[:layers]),
               (ctypes.c_float * layers)(*[1.0] * layers)) if model else (layers, None, None, None, None, None)
        return L.bg_hyper_ann_rom_run_wide(N, B, n, nbar, m, nodes, nsteps, proj, idx, ops, idx, ops, ops, ops, ops, ops, ops, *mlp,
                                           dt, 0.0, 1e-6, max_it, options, hist, hist, outs, outs, outs, null, null)

    for bad in (dict(N=2), dict(n=0), dict(nbar=0), dict(m=0), dict(nodes=0), dict(nsteps=-1), dict(max_it=0), dict(dt=0.0),
                dict(B=-1), dict(layers=0)):
        assert run(**bad) == lib.BG_ERR_BAD_ARG, bad
    assert run(proj=9) == lib.BG_ERR_PROJECTION
    assert run(N=L.bg_fom_max_n() + 1) == lib.BG_ERR_UNSUPPORTED_N
    assert run(N=L.bg_fom_max_n(), B=0) == lib.BG_OK               # the whole range of the FOM is covered
    assert run(N=3, m=3, nodes=3, B=0) == lib.BG_OK
    assert run(m=max_m, nodes=max_nodes, B=0) == lib.BG_OK         # both limits at once
    assert run(n=max_n, B=0) == lib.BG_OK and run(n=1, B=0) == lib.BG_OK and run(n=8, B=0) == lib.BG_OK
    assert run(m=max_m + 1, nodes=max_m + 1) == lib.BG_ERR_UNSUPPORTED_R
    assert run(m=max_m, nodes=max_nodes + 1) == lib.BG_ERR_UNSUPPORTED_R
    assert run(n=max_n + 1) == lib.BG_ERR_UNSUPPORTED_R
    assert run(nbar=max_nbar + 1) == lib.BG_ERR_UNSUPPORTED_R
    assert run(widths=(17, max_w + 1, 79)) == lib.BG_ERR_UNSUPPORTED_R
    assert run(layers=max_l + 1, model=False) == lib.BG_ERR_UNSUPPORTED_R
    assert run(N=100, m=101, nodes=101) == lib.BG_ERR_BAD_ARG      # more rows than the mesh has
    assert run(N=150, m=120, nodes=151) == lib.BG_ERR_BAD_ARG      # more table nodes than the mesh has
    assert run(m=120, nodes=119) == lib.BG_ERR_BAD_ARG             # every sampled row is a table node ...
    assert run(m=120, nodes=361) == lib.BG_ERR_BAD_ARG             # ... and brings at most two neighbours
    assert run(widths=(16, 32, 79)) == lib.BG_ERR_BAD_ARG          # the model does not fit n
    assert run(wt=faddr + 4) == lib.BG_ERR_BAD_ARG                 # weights not 16-byte aligned
    assert run(model=False) == lib.BG_ERR_BAD_ARG                  # null model arrays
    assert run(ops=null) == lib.BG_ERR_BAD_ARG                     # null operands, B > 0
    assert run(idx=null) == lib.BG_ERR_BAD_ARG
    assert run(hist=null) == lib.BG_ERR_BAD_ARG                    # null outputs, B > 0
    assert run(outs=null) == lib.BG_ERR_BAD_ARG
    assert run(B=0, idx=null, ops=null, hist=null, outs=null) == lib.BG_OK     # empty batch: nothing to do
    assert run(B=0, options=lib.BG_OPT_SUPG | lib.BG_OPT_NO_TANGENT_REUSE) == lib.BG_OK      # accepted


def test_existing_limits_are_unchanged(L):
    from burgers_hip import lib
    assert L.bg_abi_version() == 1
    assert lib.limits("bg_ann_rom_limits", 4) == (8, 128, 256, 8)
    assert lib.limits("bg_ann_rom_run_wide_limits", 4) == (20, 128, 256, 8)
    assert lib.limits("bg_hyper_ann_rom_limits", 6) == (8, 128, 256, 8, 256, 768)
    assert lib.limits("bg_hyper_rbf_rom_limits", 5)[0] == 20 and lib.limits("bg_hyper_rom_limits", 2) == (40, 256)
    assert L.bg_rom_max_n() == 512 and L.bg_fom_max_n() == 8192


def test_route_entry(L):
    from burgers_hip import rom
    r = rom._ROUTES[hw.ENTRY]
    assert r.min_n == 3 and rom._limit(r.max_n) == L.bg_fom_max_n() and r.supg and not r.redo and r.group == 1
    assert rom._limit(r.wg_per_cu) == 2
    # the defaults stay: nothing routes to a hyper loop unless asked
    assert rom._ann_route(5) == ("bg_ann_rom_run",) and rom._ann_route(5, fused=False) == ()
    assert rom._ann_route(17) == ("bg_ann_rom_run",) and rom._ann_route(17, wide=True) == ("bg_ann_rom_run_wide", "bg_ann_rom_run")
    import inspect
    assert inspect.signature(rom.pod_ann_run).parameters["hyper"].default is None


def test_plan_refuses_before_the_device(L):
    """Without a device a plan that reached its device copy raises RuntimeError: ValueError means the checks came first."""
    import torch
    import torch.nn as nn
    from burgers_hip import pod, rom
    max_n, max_nbar, max_w, max_l, max_m, _ = _limits(L)
    N, n, nbar = 600, 17, 20
    X = np.linspace(0.0, 100.0, N)
    U = np.linalg.qr(np.random.default_rng(3).standard_normal((N, n + nbar)))[0]
    Up, Us = U[:, :n], U[:, n:]
    model = aw.mlp([n, 16, nbar], "ELU", True, 1)
    samp = lambda rows, xi=None, proj="lspg": pod.RowSampling(np.asarray(rows, dtype=np.int32),
                                                              np.ones(len(rows)) if xi is None else xi, proj, 0.0, 0, 0.0)
    good = samp([0, 7, 8, 300, 599])
    wide_U = np.linalg.qr(np.random.default_rng(4).standard_normal((N, max_n + 1 + nbar)))[0]
    assert max_n + 1 == 21
    bad = [
        (Up[:, 0], Us, model, good), (Up, Us[:-1], model, good), (Up[:, :0], Us, model, good),         # shapes
        (wide_U[:, :max_n + 1], wide_U[:, max_n + 1:], aw.mlp([max_n + 1, 16, nbar], "ELU", True, 1), good),   # n = 21
        (Up, Us, model, samp([0, 8, 7, 300])), (Up, Us, model, samp([0, 7, 7, 300])),                  # not ascending, not distinct
        (Up, Us, model, samp([0, 7, 600])), (Up, Us, model, samp([])),                                 # outside the mesh, empty
        (Up, Us, model, samp([0, 7, 8], np.array([1.0, -0.5, 1.0]))),                                  # a negative weight
        (Up, Us, model, samp([0, 7, 8], np.array([1.0, np.nan, 1.0]))),                                # a non-finite weight
        (Up, Us, model, samp([0, 7, 8], np.ones(2))),                                                  # one weight each
        (Up, Us, model, samp(np.arange(0, 2 * (max_m + 1), 2))),                                       # more rows than the loop takes
        (Up, Us, aw.mlp([n, max_w + 1, nbar], "ELU", True, 1), good),                                  # a layer too wide
        (Up, Us, aw.mlp([n] + [8] * max_l + [nbar], "ELU", True, 1), good),                            # too many layers
        (Up, Us, aw.mlp([n, 16, nbar + 1], "ELU", True, 1), good),                                     # not (n) -> (nbar)
        (Up, Us, aw.mlp([n, 16, nbar], "ELU", True, 1).double(), good),                                # not float32
        (Up, Us, nn.Sequential(nn.Linear(n, 16), nn.Sigmoid(), nn.Linear(16, nbar)), good),            # not a recognised MLP
        (Up, Us, lambda q: q, good),                                                                   # not a module
        (Up, Us, model, samp([0, 7, 8, 300, 599], proj="petrov")),                                     # an unknown projection
        (Up, 1.001 * Us, model, good), (Up, Us + 1e-6, model, good),                                   # not orthonormal to 1e-8
    ]
    for k, (a, b, mdl, s) in enumerate(bad):
        with pytest.raises(ValueError):
            rom.HyperAnnWidePlan(a, b, mdl, s, X, None)
            pytest.fail(f"case {k} was accepted")
    with pytest.raises(ValueError):
        rom.HyperAnnWidePlan(Up, Us, model, good, X[:-1], None)                                        # another mesh length
    # the narrow plan keeps refusing more than 8 primary modes
    U9 = np.linalg.qr(np.random.default_rng(5).standard_normal((N, 9 + nbar)))[0]
    with pytest.raises(ValueError):
        rom.HyperAnnPlan(U9[:, :9], U9[:, 9:], aw.mlp([9, 16, nbar], "ELU", True, 1), good, X, None)
    if not torch.cuda.is_available():                                     # a plan that passes goes on to the device
        with pytest.raises(RuntimeError):
            rom.HyperAnnWidePlan(Up, Us, model, good, X, None)
        with pytest.raises(RuntimeError):
            rom.HyperAnnWidePlan(Up, Us, model, samp(np.arange(0, 2 * max_m, 2)), X, None)             # the row limit itself
        with pytest.raises(RuntimeError):                                 # n <= 8 is inside the wide limits
            rom.HyperAnnWidePlan(U[:, :5], U[:, 5:], aw.mlp([5, 16, n + nbar - 5], "ELU", True, 1), good, X, None)


def test_row_sampling_builder_takes_the_limit_of_the_loop_that_takes_n(L, monkeypatch):
    """build_ann_row_sampling's max_rows default: hyper_ann_rom_limits up to its n, hyper_ann_wide_rom_limits beyond."""
    from burgers_hip import pod
    seen = {}

    def fit(G, pairs, projection, tau, min_rows, max_rows):
        seen["max_rows"] = max_rows
        return None
    monkeypatch.setattr(pod, "ann_row_sampling_system", lambda *a, **k: (None, 0))
    monkeypatch.setattr(pod, "_fit_row_sampling", fit)
    X = np.linspace(0.0, 100.0, 64)
    runs = [(np.ones((64, 3)), 4.5, 0.02)]
    monkeypatch.setattr(pod, "hyper_ann_rom_limits", lambda: (8, 128, 256, 8, 111, 333))
    monkeypatch.setattr(pod, "hyper_ann_wide_rom_limits", lambda: (20, 128, 256, 8, 222, 666))
    for n, want in ((8, 111), (9, 222), (20, 222)):
        pod.build_ann_row_sampling(X, np.zeros((64, n)), np.zeros((64, 4)), None, runs, 0.05, "lspg")
        assert seen["max_rows"] == want, n
    pod.build_ann_row_sampling(X, np.zeros((64, 17)), np.zeros((64, 4)), None, runs, 0.05, "lspg", max_rows=50)
    assert seen["max_rows"] == 50
