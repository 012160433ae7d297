"""CPU-side checks of bg_local_rom_run_long (the device-side local POD loop for meshes of 513 .. 1024 nodes): the limits
and sizes it reports and the argument validation that happens before anything is launched."""
import ctypes

import pytest

from loop_cases import built_library


@pytest.fixture(scope="module")
def L():
    return built_library()


def _limits(L, name, n):
    v = [ctypes.c_int() for _ in range(n)]
    assert getattr(L, name)(*[ctypes.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


def test_limits_cover_the_headline_mesh(L):
    max_n, max_r, max_m, max_c = _limits(L, "bg_local_rom_run_long_limits", 4)
    assert max_n >= 1024 and max_r >= 40 and max_m >= 12 and max_c >= 64
    assert L.bg_local_rom_run_long_limits(None, None, None, None) == 0          # every output is optional


def test_element_counts_are_positive_and_do_not_shrink(L):
    Ns, Cs = (513, 600, 1024), (1, 11, 64)
    for N in Ns:
        v = [L.bg_local_rom_run_long_bases_elems(N, C) for C in Cs]
        assert all(e > 0 for e in v) and v == sorted(v)
        for C, e in zip(Cs, v):
            assert e >= C * (N + 2) * 40                                      # at least the padded bases
    for C in Cs:
        v = [L.bg_local_rom_run_long_bases_elems(N, C) for N in Ns]
        assert v == sorted(v)
    assert L.bg_local_rom_run_long_bases_elems(1025, 4) == 0 and L.bg_local_rom_run_long_bases_elems(1024, 65) == 0


def test_argument_validation_before_launch(L):
    from burgers_hip import lib
    null = None
    buf = (ctypes.c_double * 10)()
    ibuf = (ctypes.c_int32 * 8)()
    aligned = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    p = ctypes.cast(aligned, ctypes.POINTER(ctypes.c_double))
    ip = ctypes.cast(ibuf, ctypes.POINTER(ctypes.c_int32))
    max_n, max_r, max_m, max_c = _limits(L, "bg_local_rom_run_long_limits", 4)

    def run(N=1024, B=4, C=11, rmax=40, m=12, nsteps=2, proj=lib.BG_PROJ_GALERKIN, dt=0.025, max_it=20, ops=p, wid=ip,
            bases=p, hist=p, outs=ip):
        return L.bg_local_rom_run_long(N, B, C, rmax, m, nsteps, proj, ops, bases, wid, ops, ops, ops, ops, ops, dt, 0.0,
                                       1e-6, max_it, lib.BG_OPT_SUPG, hist, outs, outs, outs, null, null, null)

    assert run(N=2) == lib.BG_ERR_BAD_ARG
    assert run(B=-1) == lib.BG_ERR_BAD_ARG
    assert run(C=0) == lib.BG_ERR_BAD_ARG
    assert run(rmax=0) == lib.BG_ERR_BAD_ARG
    assert run(m=0) == lib.BG_ERR_BAD_ARG
    assert run(nsteps=-1) == lib.BG_ERR_BAD_ARG
    assert run(max_it=0) == lib.BG_ERR_BAD_ARG
    assert run(dt=0.0) == lib.BG_ERR_BAD_ARG
    assert run(proj=9) == lib.BG_ERR_PROJECTION
    assert run(N=max_n + 1) == lib.BG_ERR_UNSUPPORTED_N
    assert run(rmax=max_r + 1) == lib.BG_ERR_UNSUPPORTED_R
    assert run(m=max_m + 1) == lib.BG_ERR_UNSUPPORTED_R
    assert run(C=max_c + 1) == lib.BG_ERR_UNSUPPORTED_R
    assert run(ops=null) == lib.BG_ERR_BAD_ARG             # null operands, B > 0
    assert run(bases=null) == lib.BG_ERR_BAD_ARG
    assert run(wid=null) == lib.BG_ERR_BAD_ARG
    assert run(hist=null) == lib.BG_ERR_BAD_ARG            # null outputs, B > 0
    assert run(outs=null) == lib.BG_ERR_BAD_ARG
    odd = ctypes.cast(aligned + 8, ctypes.POINTER(ctypes.c_double))
    assert run(bases=odd) == lib.BG_ERR_BAD_ARG            # bases not 16-byte aligned
    assert run(B=0, ops=null, wid=null, bases=null, hist=null, outs=null) == lib.BG_OK   # empty batch: nothing to do


def test_existing_limits_are_unchanged(L):
    assert _limits(L, "bg_local_rom_limits", 3) == (40, 64, 64)
    assert L.bg_rom_run_long_max_n() == 1024 and L.bg_rom_run_long_max_r() == 40
    assert L.bg_rom_max_n() == 512 and L.bg_rom_run_max_r() == 40
    assert L.bg_abi_version() == 1
