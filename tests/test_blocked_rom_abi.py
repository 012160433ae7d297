"""CPU-side checks of bg_rom_run_blocked (the device-side POD-PROM loop for bases of up to 256 modes): the limits and
sizes it reports and the argument validation that happens before anything is launched."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    from burgers_hip import build, lib
    build.build_library()
    return lib.load()


def test_limits_cover_the_thesis_bases(L):
    assert L.bg_rom_run_blocked_max_r() >= 227
    assert L.bg_rom_run_blocked_max_r() > L.bg_rom_run_wide_max_r()


def test_element_counts_are_positive_and_grow_with_r(L):
    for N in (3, 200, 300, 512):
        phi = [L.bg_rom_run_blocked_phi_elems(N, r) for r in (1, 97, 160, 227, 256)]
        work = [L.bg_rom_run_blocked_work_elems(N, r) for r in (1, 97, 160, 227, 256)]
        assert all(v > 0 for v in phi + work)
        assert phi == sorted(phi) and len(set(phi)) == len(phi)
        assert work == sorted(work) and len(set(work)) == len(work)
        assert phi[-1] >= (N + 2) * 256                       # at least the padded basis
        assert work[3] >= 227 * 228                           # at least Ar | br at r = 227


def test_argument_validation_before_launch(L):
    from burgers_hip import lib
    null = None
    buf = (ctypes.c_double * 8)()
    ibuf = (ctypes.c_int32 * 8)()
    p = ctypes.cast(buf, ctypes.POINTER(ctypes.c_double))
    ip = ctypes.cast(ibuf, ctypes.POINTER(ctypes.c_int32))

    def run(N=512, B=4, r=160, nsteps=2, proj=lib.BG_PROJ_GALERKIN, dt=0.05, max_it=20, ops=p, work=p, slots=4, outs=ip):
        return L.bg_rom_run_blocked(N, B, r, nsteps, proj, ops, ops, ops, ops, ops, dt, 0.0, 1e-6, max_it,
                                    lib.BG_OPT_SUPG, work, slots, ops, outs, outs, outs, null, null)

    assert run(N=2) == lib.BG_ERR_BAD_ARG
    assert run(r=0) == lib.BG_ERR_BAD_ARG
    assert run(nsteps=-1) == lib.BG_ERR_BAD_ARG
    assert run(max_it=0) == lib.BG_ERR_BAD_ARG
    assert run(dt=0.0) == lib.BG_ERR_BAD_ARG
    assert run(B=-1) == lib.BG_ERR_BAD_ARG
    assert run(proj=9) == lib.BG_ERR_PROJECTION
    assert run(N=513) == lib.BG_ERR_UNSUPPORTED_N
    assert run(r=257) == lib.BG_ERR_UNSUPPORTED_R
    assert run(ops=null) == lib.BG_ERR_BAD_ARG             # null operands, B > 0
    assert run(outs=null) == lib.BG_ERR_BAD_ARG
    assert run(work=null) == lib.BG_ERR_WORKSPACE
    assert run(slots=0) == lib.BG_ERR_WORKSPACE
    assert run(B=0, ops=null, work=null, slots=0, outs=null) == lib.BG_OK     # empty batch: nothing to do
