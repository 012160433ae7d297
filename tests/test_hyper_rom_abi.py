"""CPU-side checks of bg_hyper_rom_run (the hyper-reduced POD-PROM loop on sampled mesh rows): the limits and table size
it reports and the argument validation that happens before anything is launched."""
import ctypes

import pytest

from loop_cases import built_library, host_pointers


@pytest.fixture(scope="module")
def L():
    return built_library()


def _limits(L):
    max_r, max_m = ctypes.c_int(), ctypes.c_int()
    assert L.bg_hyper_rom_limits(ctypes.byref(max_r), ctypes.byref(max_m)) == 0
    return max_r.value, max_m.value


def test_limits_cover_the_headline_case(L):
    max_r, max_m = _limits(L)
    assert max_r >= 40 and max_m >= 256
    assert L.bg_hyper_rom_limits(None, None) != 0


def test_table_elems_are_positive_monotone_and_hold_the_stencil(L):
    max_r, max_m = _limits(L)
    ms, rs = (1, 17, 31, 32, 33, 122, 255, max_m), (1, 17, max_r)
    for r in rs:
        t = [L.bg_hyper_rom_table_elems(m, r) for m in ms]
        assert all(v > 0 for v in t) and t == sorted(t)
        for m, v in zip(ms, t):
            assert v >= 3 * m * r
    for m in ms:
        t = [L.bg_hyper_rom_table_elems(m, r) for r in rs]
        assert t == sorted(t)
    for m, r in ((0, 17), (max_m + 1, 17), (17, 0), (17, max_r + 1)):
        assert L.bg_hyper_rom_table_elems(m, r) == 0               # not covered


def test_argument_validation_before_launch(L):
    """In the style of loop_cases.check_pod_loop_argument_validation, for this entry's own argument list."""
    from burgers_hip import lib
    max_r, max_m = _limits(L)
    null = None
    p, ip = host_pointers()

    def run(N=2049, B=4, r=40, m=122, nsteps=2, proj=lib.BG_PROJ_GALERKIN, dt=0.0125, max_it=20, rows=ip, ops=p, hist=p, outs=ip):
        return L.bg_hyper_rom_run(N, B, r, m, nsteps, proj, rows, ops, ops, ops, ops, ops, ops, ops, dt, 0.0, 1e-6, max_it,
                                  lib.BG_OPT_SUPG, hist, outs, outs, outs, null, null)

    assert run(N=2) == lib.BG_ERR_BAD_ARG
    assert run(r=0) == lib.BG_ERR_BAD_ARG
    assert run(m=0) == lib.BG_ERR_BAD_ARG
    assert run(nsteps=-1) == lib.BG_ERR_BAD_ARG
    assert run(max_it=0) == lib.BG_ERR_BAD_ARG
    assert run(dt=0.0) == lib.BG_ERR_BAD_ARG
    assert run(B=-1) == lib.BG_ERR_BAD_ARG
    assert run(proj=9) == lib.BG_ERR_PROJECTION
    assert run(N=L.bg_fom_max_n() + 1) == lib.BG_ERR_UNSUPPORTED_N
    assert run(N=L.bg_fom_max_n(), B=0) == lib.BG_OK               # the whole range of the FOM is covered
    assert run(r=max_r + 1) == lib.BG_ERR_UNSUPPORTED_R
    assert run(m=max_m + 1) == lib.BG_ERR_UNSUPPORTED_R            # the documented code for too many rows
    assert run(N=100, m=101) == lib.BG_ERR_BAD_ARG                 # more rows than the mesh has
    assert run(ops=null) == lib.BG_ERR_BAD_ARG                     # null operands, B > 0
    assert run(rows=null) == lib.BG_ERR_BAD_ARG
    assert run(hist=null) == lib.BG_ERR_BAD_ARG                    # null outputs, B > 0
    assert run(outs=null) == lib.BG_ERR_BAD_ARG
    assert run(B=0, rows=null, ops=null, hist=null, outs=null) == lib.BG_OK     # empty batch: nothing to do


def test_existing_limits_are_unchanged(L):
    assert L.bg_abi_version() == 1
    assert L.bg_rom_max_n() == 512 and L.bg_rom_run_max_r() == 40
    assert L.bg_rom_run_long_max_n() == 1024 and L.bg_rom_run_long_max_r() == 40
    assert L.bg_fom_max_n() == 8192
