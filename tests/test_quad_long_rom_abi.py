"""bg_quad_rom_run_long (csrc/quad_long.hip), the part that needs no GPU: the limits, the element-count queries and the
argument validation, which returns before any pointer is touched or any kernel is launched; and the limits of the
entry points beside it, which must not move."""
import ctypes

import pytest


def _call(L, N=1024, B=1, n=40, nsteps=1, proj=1, dt=0.05, max_it=25, ptrs=None):
    p = [None] * 12 if ptrs is None else ptrs
    # x, PhiT, Phif, H3f, u0, mu1, mu2 | hist, iters, flags, info, order
    return L.bg_quad_rom_run_long(N, B, n, nsteps, proj, *p[:7], dt, 0.0, 1e-6, max_it, 0, *p[7:], None)


def test_limits_and_element_counts():
    from burgers_hip import lib
    L = lib.load()
    assert L.bg_quad_rom_run_long_max_n() >= 1024 and L.bg_quad_rom_run_long_max_r() >= 40
    assert L.bg_quad_rom_run_long_workgroups_per_cu() >= 1
    for q in (L.bg_quad_rom_run_long_phit_elems, L.bg_quad_rom_run_long_phif_elems, L.bg_quad_rom_run_long_h3f_elems):
        counts = [q(N) for N in (513, 600, 1024)]
        assert all(c > 0 for c in counts) and counts == sorted(counts), counts
    # the documented layouts: PhiT [40][NPAD], Phif [NG][10][16], H3f [NG][28][64][2]
    assert L.bg_quad_rom_run_long_phit_elems(1000) == 40 * 1024
    assert L.bg_quad_rom_run_long_phif_elems(1000) == 250 * 160
    assert L.bg_quad_rom_run_long_h3f_elems(1000) == 250 * 28 * 128
    # N <= 512 is refused (bg_quad_rom_run covers it), and so is N > 1024: no operand to size
    for N in (2, 512, 1025):
        assert L.bg_quad_rom_run_long_h3f_elems(N) == 0 and L.bg_quad_rom_run_long_phit_elems(N) == 0


@pytest.mark.parametrize("kw", [dict(N=2), dict(n=0), dict(nsteps=-1), dict(max_it=0), dict(dt=0.0), dict(dt=-0.05), dict(B=-1)])
def test_bad_sizes_are_bad_arguments(kw):
    from burgers_hip import lib
    assert _call(lib.load(), **kw) == lib.BG_ERR_BAD_ARG


def test_codes_in_the_documented_order():
    from burgers_hip import lib
    L = lib.load()
    assert _call(L, proj=7) == lib.BG_ERR_PROJECTION
    assert _call(L, N=1025) == lib.BG_ERR_UNSUPPORTED_N
    assert _call(L, N=4096) == lib.BG_ERR_UNSUPPORTED_N
    assert _call(L, N=512) == lib.BG_ERR_UNSUPPORTED_N          # refused by design: bg_quad_rom_run's range
    assert _call(L, N=64) == lib.BG_ERR_UNSUPPORTED_N
    assert _call(L, n=41) == lib.BG_ERR_UNSUPPORTED_R
    assert _call(L, N=1025, proj=7) == lib.BG_ERR_PROJECTION     # the projection is looked at first, as in bg_rom_run_long
    assert _call(L, N=2, proj=7) == lib.BG_ERR_BAD_ARG


def test_empty_batch_and_null_pointers():
    from burgers_hip import lib
    L = lib.load()
    for N in (513, 600, 1024):
        for proj in (0, 1):
            assert _call(L, N=N, B=0, proj=proj) == lib.BG_OK          # nothing to do, nothing dereferenced
    assert _call(L, N=1024, B=1) == lib.BG_ERR_BAD_ARG                 # null operands and outputs with B > 0
    # every single null operand or output is caught (the others point at host memory that is never read: no launch)
    buf = (ctypes.c_double * 8)()
    addr = ctypes.cast(buf, ctypes.c_void_p)
    for hole in range(11):                                             # order (index 11) may be null
        ptrs = [addr] * 11 + [None]
        ptrs[hole] = None
        assert _call(L, N=1024, B=1, ptrs=ptrs) == lib.BG_ERR_BAD_ARG, hole


def test_existing_limits_are_unchanged():
    from burgers_hip import lib
    L = lib.load()
    assert L.bg_abi_version() == 1
    assert L.bg_quad_rom_max_n() == 40
    assert L.bg_quad_rom_run(600, 1, 5, 1, 1, None, None, None, None, None, None, None, 0.05, 0.0, 1e-6, 25, 0, None, None, None, None,
                             None, None) == lib.BG_ERR_UNSUPPORTED_N
    assert L.bg_rom_run_long_max_n() == 1024 and L.bg_rom_run_long_max_r() == 40


def test_plan_refusals_that_need_no_device():
    """QuadLongPlan checks the shapes before it asks for a device."""
    import numpy as np
    from burgers_hip import rom
    with pytest.raises(ValueError):
        rom.QuadLongPlan(np.zeros((1024, 41)), np.zeros((1024, 41 * 42 // 2)), None)      # n = 41
    with pytest.raises(ValueError):
        rom.QuadLongPlan(np.zeros((1025, 8)), np.zeros((1025, 36)), None)                 # N = 1025
    with pytest.raises(ValueError):
        rom.QuadLongPlan(np.zeros((512, 8)), np.zeros((512, 36)), None)                   # bg_quad_rom_run's range
    with pytest.raises(ValueError):
        rom.QuadLongPlan(np.zeros((1024, 8)), np.zeros((1024, 35)), None)                 # H one column short
    with pytest.raises(ValueError):
        rom.QuadLongPlan(np.zeros(1024), np.zeros((1024, 1)), None)
