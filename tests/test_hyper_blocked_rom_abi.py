"""CPU-side checks of bg_hyper_rom_run_blocked (the hyper-reduced POD-PROM loop for 97 to 256 modes on sampled mesh rows): the
limits, table and workspace sizes it reports, the argument validation that happens before anything is launched, the host-side
route, and the row limit build_row_sampling hands to the fit for a basis beyond the wide loop's."""
import ctypes

import numpy as np
import pytest

from loop_cases import built_library, host_pointers


@pytest.fixture(scope="module")
def L():
    return built_library()


def _limits(L, name="bg_hyper_rom_blocked_limits"):
    max_r, max_m = ctypes.c_int(), ctypes.c_int()
    assert getattr(L, name)(ctypes.byref(max_r), ctypes.byref(max_m)) == 0
    return max_r.value, max_m.value


def test_limits_and_the_workspace_slot(L):
    from burgers_hip import pod
    max_r, max_m = _limits(L)
    assert max_r == 256 and max_m >= 768 and max_m % 8 == 0
    assert L.bg_hyper_rom_blocked_limits(None, None) != 0
    assert tuple(pod.hyper_blocked_rom_limits()) == (max_r, max_m)
    assert _limits(L, "bg_hyper_rom_wide_limits") == (96, 512)     # the wide loop keeps its own
    for r in (1, 16, 17, 97, 160, 227, 256):
        RP = (r + 15) // 16 * 16
        assert L.bg_hyper_rom_blocked_work_elems(r) == RP * (RP + 16)
        assert L.bg_hyper_rom_blocked_work_elems(r) == L.bg_rom_run_blocked_work_elems(512, r)      # bg_rom_run_blocked's slot
    assert L.bg_hyper_rom_blocked_work_elems(0) == 0 and L.bg_hyper_rom_blocked_work_elems(257) == 0


def test_table_elems_are_three_padded_rows_per_sampled_row(L):
    max_r, max_m = _limits(L)
    for m in (1, 7, 8, 9, 261, 300, 513, 768, max_m - 1, max_m):
        for r in (1, 97, 113, 160, 227, max_r):
            MPAD, RP = (m + 7) // 8 * 8, (r + 15) // 16 * 16
            assert L.bg_hyper_rom_blocked_table_elems(m, r) == 3 * MPAD * RP
    for m, r in ((0, 160), (max_m + 1, 160), (300, 0), (300, max_r + 1)):
        assert L.bg_hyper_rom_blocked_table_elems(m, r) == 0       # not covered


def test_argument_validation_before_launch(L):
    """test_hyper_wide_rom_abi.py's list for this entry, with the workspace and the option it refuses."""
    from burgers_hip import lib
    max_r, max_m = _limits(L)
    null = None
    p, ip = host_pointers()

    def run(N=2049, B=4, r=160, m=480, nsteps=2, proj=lib.BG_PROJ_GALERKIN, dt=0.0125, max_it=20, rows=ip, ops=p, hist=p, outs=ip,
            table=None, opts=lib.BG_OPT_SUPG, work=p, slots=4):
        return L.bg_hyper_rom_run_blocked(N, B, r, m, nsteps, proj, rows, ops, ops, ops if table is None else table, ops, ops, ops, ops,
                                          dt, 0.0, 1e-6, max_it, opts, work, slots, hist, outs, outs, outs, null, null)

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
    base = ctypes.addressof(p.contents)
    unaligned = ctypes.cast(base + (8 if base % 16 == 0 else 0), ctypes.POINTER(ctypes.c_double))
    assert run(table=unaligned) == lib.BG_ERR_BAD_ARG              # as the other tables: 16-byte aligned
    assert run(work=null) == lib.BG_ERR_WORKSPACE
    assert run(slots=0) == lib.BG_ERR_WORKSPACE
    assert run(opts=lib.BG_OPT_SUPG | lib.BG_OPT_PIVOT_ON_DEVICE) == lib.BG_ERR_BAD_ARG      # this loop has no repair kernel
    assert run(B=0, rows=null, ops=null, hist=null, outs=null, work=null, slots=0) == lib.BG_OK     # empty batch: nothing to do


def test_route_and_plan_type(L):
    from burgers_hip import rom
    route = rom._ROUTES["bg_hyper_rom_run_blocked"]
    assert route.redo and route.wg_per_cu == 1 and route.min_n == 3 and rom._limit(route.max_n) == L.bg_fom_max_n()
    assert issubclass(rom.HyperBlockedPodPlan, rom.HyperPodPlan) and not issubclass(rom.HyperBlockedPodPlan, rom.HyperWidePodPlan)
    assert rom.HyperBlockedPodPlan.entry == "bg_hyper_rom_run_blocked"


def test_build_row_sampling_hands_the_fit_the_blocked_limit_beyond_the_wide_basis(L, monkeypatch):
    from burgers_hip import pod
    seen = {}

    def fit(G, pairs, projection, tau, min_rows, max_rows):
        seen["limits"] = (min_rows, max_rows)
        return "fitted"
    monkeypatch.setattr(pod, "_fit_row_sampling", fit)
    monkeypatch.setattr(pod, "row_sampling_system", lambda *a, **k: (np.zeros((97, 600)), 1))
    X = np.linspace(0.0, 100.0, 600)
    runs = [(np.ones((600, 3)), 4.5, 0.02)]
    assert pod.build_row_sampling(X, np.zeros((600, 97)), runs, 0.05, "Galerkin") == "fitted"
    assert seen["limits"] == (291, _limits(L)[1])
    assert pod.build_row_sampling(X, np.zeros((600, 97)), runs, 0.05, "LSPG", min_rows=7, max_rows=300) == "fitted"
    assert seen["limits"] == (7, 300)
