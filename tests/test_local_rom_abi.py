"""CPU-side checks of bg_local_rom_limits / bg_local_rom_run (the device-side local POD time loop): the limits it reports
and the argument validation that happens before anything is launched."""
import ctypes

import pytest

from loop_cases import built_library, host_pointers


@pytest.fixture(scope="module")
def L():
    return built_library()


def test_limits_cover_the_issue_sizes(L):
    v = [ctypes.c_int() for _ in range(3)]
    assert L.bg_local_rom_limits(*[ctypes.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [40, 64, 64]


def test_argument_validation_before_launch(L):
    from burgers_hip import lib
    null = None
    p, ip = host_pointers()

    def run(N=512, B=4, C=4, rmax=30, m=12, nsteps=2, proj=lib.BG_PROJ_GALERKIN, ops=p, widths=ip, outs=ip, dt=0.05,
            max_it=20):
        return L.bg_local_rom_run(N, B, C, rmax, m, nsteps, proj, ops, ops, widths, ops, ops, ops, ops, ops, dt, 0.0, 1e-6,
                                  max_it, lib.BG_OPT_SUPG, ops, outs, outs, outs, null, null, null)

    assert run(N=1) == lib.BG_ERR_BAD_ARG
    assert run(B=-1) == lib.BG_ERR_BAD_ARG
    assert run(C=0) == lib.BG_ERR_BAD_ARG
    assert run(rmax=0) == lib.BG_ERR_BAD_ARG
    assert run(m=0) == lib.BG_ERR_BAD_ARG
    assert run(nsteps=-1) == lib.BG_ERR_BAD_ARG
    assert run(max_it=0) == lib.BG_ERR_BAD_ARG
    assert run(dt=0.0) == lib.BG_ERR_BAD_ARG
    assert run(proj=9) == lib.BG_ERR_PROJECTION
    assert run(N=513) == lib.BG_ERR_UNSUPPORTED_N
    assert run(rmax=41) == lib.BG_ERR_UNSUPPORTED_R
    assert run(m=65) == lib.BG_ERR_UNSUPPORTED_R
    assert run(C=65) == lib.BG_ERR_UNSUPPORTED_R
    assert run(ops=null) == lib.BG_ERR_BAD_ARG          # null operands, B > 0
    assert run(widths=null) == lib.BG_ERR_BAD_ARG
    assert run(outs=null) == lib.BG_ERR_BAD_ARG
    assert run(B=0, ops=null, widths=null, outs=null) == lib.BG_OK    # empty batch: nothing to do
