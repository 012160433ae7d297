"""CPU-side checks of bg_rom_run_long (the device-side POD-PROM loop for meshes of 513 .. 1024 nodes): the limits and
sizes it reports and the argument validation that happens before anything is launched."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    from burgers_hip import build, lib
    build.build_library()
    return lib.load()


def test_limits_cover_the_headline_mesh(L):
    assert L.bg_rom_run_long_max_n() >= 1024
    assert L.bg_rom_run_long_max_r() >= 40
    assert L.bg_rom_run_long_workgroups_per_cu() >= 1


def test_element_counts_are_positive_and_do_not_shrink(L):
    Ns, rs = (513, 600, 1024), (1, 17, 40)
    for N in Ns:
        phi = [L.bg_rom_run_long_phi_elems(N, r) for r in rs]
        assert all(v > 0 for v in phi) and phi == sorted(phi)
        for r, v in zip(rs, phi):
            assert v >= (N + 2) * r                                  # at least the padded basis
    for r in rs:
        phi = [L.bg_rom_run_long_phi_elems(N, r) for N in Ns]
        assert phi == sorted(phi)


def test_argument_validation_before_launch(L):
    from burgers_hip import lib
    null = None
    buf = (ctypes.c_double * 8)()
    ibuf = (ctypes.c_int32 * 8)()
    p = ctypes.cast(buf, ctypes.POINTER(ctypes.c_double))
    ip = ctypes.cast(ibuf, ctypes.POINTER(ctypes.c_int32))

    def run(N=1024, B=4, r=40, nsteps=2, proj=lib.BG_PROJ_GALERKIN, dt=0.025, max_it=20, ops=p, hist=p, outs=ip):
        return L.bg_rom_run_long(N, B, r, nsteps, proj, ops, ops, ops, ops, ops, dt, 0.0, 1e-6, max_it,
                                 lib.BG_OPT_SUPG, hist, outs, outs, outs, null, null)

    assert run(N=2) == lib.BG_ERR_BAD_ARG
    assert run(r=0) == lib.BG_ERR_BAD_ARG
    assert run(nsteps=-1) == lib.BG_ERR_BAD_ARG
    assert run(max_it=0) == lib.BG_ERR_BAD_ARG
    assert run(dt=0.0) == lib.BG_ERR_BAD_ARG
    assert run(B=-1) == lib.BG_ERR_BAD_ARG
    assert run(proj=9) == lib.BG_ERR_PROJECTION
    assert run(N=L.bg_rom_run_long_max_n() + 1) == lib.BG_ERR_UNSUPPORTED_N
    assert run(r=L.bg_rom_run_long_max_r() + 1) == lib.BG_ERR_UNSUPPORTED_R
    assert run(ops=null) == lib.BG_ERR_BAD_ARG             # null operands, B > 0
    assert run(hist=null) == lib.BG_ERR_BAD_ARG            # null outputs, B > 0
    assert run(outs=null) == lib.BG_ERR_BAD_ARG
    assert run(B=0, ops=null, hist=null, outs=null) == lib.BG_OK     # empty batch: nothing to do


def test_existing_limits_are_unchanged(L):
    assert L.bg_rom_max_n() == 512 and L.bg_rom_run_max_r() == 40
    assert L.bg_abi_version() == 1
