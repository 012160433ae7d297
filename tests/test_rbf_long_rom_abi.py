"""CPU-side checks of bg_rbf_rom_run_long_limits / bg_rbf_rom_run_long (the device-side POD-RBF time loop for meshes of
513 .. 1024 nodes): the limits, the argument validation that happens before anything is launched, the route table of
rom.pod_rbf_run, what the long plan refuses before it touches a device -- and the conditioning of the cases the GPU test
(tests/test_rom_rbf_long_gpu.py) holds the loop to."""
import ctypes

import numpy as np
import pytest

import rbf_long_cases as rc
from conftest import rel_l2
from loop_cases import built_library, host_pointers


@pytest.fixture(scope="module")
def L():
    return built_library()


def test_limits(L):
    v = [ctypes.c_int(-1) for _ in range(4)]
    assert L.bg_rbf_rom_run_long_limits(*[ctypes.byref(x) for x in v]) == 0
    assert tuple(x.value for x in v) == (1024, 20, 128, 65536)
    one = ctypes.c_int(-1)                                   # every output is optional
    assert L.bg_rbf_rom_run_long_limits(None, None, ctypes.byref(one), None) == 0 and one.value == 128
    assert L.bg_rbf_rom_run_long_limits(None, None, None, None) == 0


def test_existing_limits_are_unchanged(L):
    v = [ctypes.c_int(-1) for _ in range(3)]
    assert L.bg_rbf_rom_limits(*[ctypes.byref(x) for x in v]) == 0
    assert tuple(x.value for x in v) == (20, 128, 65536)
    assert L.bg_rom_max_n() == 512
    assert L.bg_abi_version() == 1


def _caller(L):
    from burgers_hip import lib
    p, ip = host_pointers()

    def run(N=1024, B=4, n=17, nbar=79, Ns=300, nsteps=2, proj=lib.BG_PROJ_LSPG, kind=lib.BG_RBF_GAUSSIAN, ops=p, outs=ip,
            UT=None, dt=0.05, max_it=30):
        return L.bg_rbf_rom_run_long(N, B, n, nbar, Ns, nsteps, proj, kind, ops, ops if UT is None else UT, ops, ops, ops,
                                     ops, ops, 1.0, ops, ops, ops, dt, 0.0, 1e-6, max_it, lib.BG_OPT_SUPG, ops, outs, outs,
                                     outs, None, None)
    return run


def test_argument_validation_before_launch(L):
    from burgers_hip import lib
    run, null = _caller(L), None
    assert run(n=0) == lib.BG_ERR_BAD_ARG
    assert run(nbar=0) == lib.BG_ERR_BAD_ARG
    assert run(Ns=0) == lib.BG_ERR_BAD_ARG
    assert run(B=-1) == lib.BG_ERR_BAD_ARG
    assert run(nsteps=-1) == lib.BG_ERR_BAD_ARG
    assert run(max_it=0) == lib.BG_ERR_BAD_ARG
    assert run(dt=0.0) == lib.BG_ERR_BAD_ARG
    assert run(kind=7) == lib.BG_ERR_BAD_ARG
    assert run(proj=9) == lib.BG_ERR_PROJECTION
    assert run(N=512) == lib.BG_ERR_UNSUPPORTED_N          # bg_rbf_rom_run covers the short meshes
    assert run(N=2) == lib.BG_ERR_UNSUPPORTED_N
    assert run(N=1025) == lib.BG_ERR_UNSUPPORTED_N
    assert run(n=21) == lib.BG_ERR_UNSUPPORTED_R
    assert run(nbar=129) == lib.BG_ERR_UNSUPPORTED_R
    assert run(Ns=65537) == lib.BG_ERR_UNSUPPORTED_R
    assert run(ops=null) == lib.BG_ERR_BAD_ARG              # null operands, B > 0
    assert run(outs=null) == lib.BG_ERR_BAD_ARG
    assert run(B=0, ops=null, outs=null) == lib.BG_OK        # empty batch: nothing to do, no pointer is looked at
    assert run(N=513, B=0, ops=null, outs=null) == lib.BG_OK


def test_misaligned_ut_is_refused(L):
    from burgers_hip import lib
    buf = (ctypes.c_double * 8)()
    base = ctypes.addressof(buf)
    at = lambda rem: ctypes.cast(base + (rem - base) % 16, ctypes.POINTER(ctypes.c_double))
    assert _caller(L)(UT=at(8)) == lib.BG_ERR_BAD_ARG       # 8 bytes past a 16-byte boundary


def test_rbf_route_table(L):
    """pod_rbf_run tries these loops in this order and takes the first whose RbfFusedPlan is ``ok``; nothing left: host."""
    from burgers_hip.rom import _rbf_route as route
    F, FL = "bg_rbf_rom_run", "bg_rbf_rom_run_long"
    for N in (17, 512, 513, 1024, 1025):
        assert route(N) == () and route(N, long_mesh=True) == ()              # the default is the host-driven iteration
        assert route(N, fused=True) == (F,)                                  # (its plan declines N > 512)
    for N in (17, 512):
        assert route(N, fused=True, long_mesh=True) == (F,)                  # long_mesh starts above 512 nodes
    for N in (513, 1024, 1025):
        assert route(N, fused=True, long_mesh=True) == (FL, F)               # (the long plan declines N > 1024)


def test_long_plan_refuses_before_the_device(L):
    """Without a device a plan that reached its device copy raises RuntimeError: ValueError means the shape checks came first."""
    import torch
    from burgers_hip import rom
    Up, Us, Xt, W, eps, x_min, x_max, y_min, y_max = rc.closure(600, "gaussian")
    plan = lambda *a: rom.RbfFusedPlan(*a, "gaussian", None, long_mesh=True)
    for bad in ((Up[:, 0], Us, Xt, W, eps, x_min, x_max, y_min, y_max),            # U_p without columns
                (Up[:599], Us, Xt, W, eps, x_min, x_max, y_min, y_max),            # rows of U_p and U_s differ
                (Up, Us[:, :50], Xt, W, eps, x_min, x_max, y_min, y_max),          # W has the columns of another U_s
                (Up[:, :16], Us, Xt, W, eps, x_min[:16], x_max[:16], y_min, y_max),  # centres of another n
                (Up, Us, Xt, W[:299], eps, x_min, x_max, y_min, y_max),            # one weight row short
                (Up, Us, Xt, W, eps, x_min[:16], x_max, y_min, y_max),
                (Up, Us, Xt, W, eps, x_min, x_max, y_min, y_max[:78])):
        with pytest.raises(ValueError):
            plan(*bad)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            plan(Up, Us, Xt, W, eps, x_min, x_max, y_min, y_max)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_cases_are_well_conditioned(name):
    """Every case of the GPU test, by the oracle, clean and with U_p, U_s, W carrying 4e-16 relative noise: the same
    iteration counts and rel-L2 < 1e-12, three orders below the GPU gate of 1e-9 -- a loop that rounds differently from the
    oracle cannot miss the gate for that reason.  Also pins the counts the table lists."""
    clean, noisy = rc.oracle_run(name), rc.oracle_run_perturbed(name)
    want = rc.CASES[name][-1]
    if want is not None:
        assert clean[0][1].tolist() == want
    for (U, it), (Un, itn) in zip(clean, noisy):
        err = rel_l2(Un, U)
        print(f"{name}: iterations {it.tolist()}, rel-L2 under operand noise {err:.1e}")
        assert np.array_equal(it, itn)
        assert err < 1e-12
