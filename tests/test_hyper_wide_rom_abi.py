"""CPU-side checks of bg_hyper_rom_run_wide (the hyper-reduced POD-PROM loop for 41 to 96 modes on sampled mesh rows): the
limits and table size it reports, the argument validation that happens before anything is launched, the host-side route,
and the row limit build_row_sampling hands to the fit for each width."""
import ctypes

import numpy as np
import pytest

from loop_cases import built_library, host_pointers


@pytest.fixture(scope="module")
def L():
    return built_library()


def _limits(L, name="bg_hyper_rom_wide_limits"):
    max_r, max_m = ctypes.c_int(), ctypes.c_int()
    assert getattr(L, name)(ctypes.byref(max_r), ctypes.byref(max_m)) == 0
    return max_r.value, max_m.value


def test_limits_are_the_wide_basis_and_512_rows(L):
    from burgers_hip import pod
    assert _limits(L) == (96, 512)
    assert L.bg_hyper_rom_wide_limits(None, None) != 0
    assert _limits(L, "bg_hyper_rom_limits") == (40, 256)          # the narrow loop keeps its own
    assert tuple(pod.hyper_wide_rom_limits()) == (96, 512) and tuple(pod.hyper_rom_limits()) == (40, 256)


def test_table_elems_are_positive_monotone_and_hold_the_stencil(L):
    max_r, max_m = _limits(L)
    ms, rs = (1, 15, 16, 17, 122, 256, 257, 507, max_m), (1, 41, 77, max_r)
    for r in rs:
        t = [L.bg_hyper_rom_wide_table_elems(m, r) for m in ms]
        assert all(v > 0 for v in t) and t == sorted(t)
        for m, v in zip(ms, t):
            assert v >= 3 * m * r
    for m in ms:
        t = [L.bg_hyper_rom_wide_table_elems(m, r) for r in rs]
        assert t == sorted(t)
    for m, r in ((0, 17), (max_m + 1, 17), (17, 0), (17, max_r + 1)):
        assert L.bg_hyper_rom_wide_table_elems(m, r) == 0          # not covered


def test_argument_validation_before_launch(L):
    """test_hyper_rom_abi.py's list, for the wide entry."""
    from burgers_hip import lib
    max_r, max_m = _limits(L)
    null = None
    p, ip = host_pointers()

    def run(N=2049, B=4, r=96, m=200, nsteps=2, proj=lib.BG_PROJ_GALERKIN, dt=0.0125, max_it=20, rows=ip, ops=p, hist=p, outs=ip,
            table=None):
        return L.bg_hyper_rom_run_wide(N, B, r, m, nsteps, proj, rows, ops, ops, ops if table is None else table, ops, ops, ops, ops,
                                       dt, 0.0, 1e-6, max_it, lib.BG_OPT_SUPG, hist, outs, outs, outs, null, null)

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
    assert (max_r + 1, max_m + 1) == (97, 513)
    assert run(r=97) == lib.BG_ERR_UNSUPPORTED_R
    assert run(m=513) == lib.BG_ERR_UNSUPPORTED_R                  # the documented code for too many rows
    assert run(N=100, m=101) == lib.BG_ERR_BAD_ARG                 # more rows than the mesh has
    assert run(ops=null) == lib.BG_ERR_BAD_ARG                     # null operands, B > 0
    assert run(rows=null) == lib.BG_ERR_BAD_ARG
    assert run(hist=null) == lib.BG_ERR_BAD_ARG                    # null outputs, B > 0
    assert run(outs=null) == lib.BG_ERR_BAD_ARG
    base = ctypes.addressof(p.contents)
    unaligned = ctypes.cast(base + (8 if base % 16 == 0 else 0), ctypes.POINTER(ctypes.c_double))
    assert run(table=unaligned) == lib.BG_ERR_BAD_ARG              # the table is read by 16-byte LDS DMA
    assert run(B=0, rows=null, ops=null, hist=null, outs=null) == lib.BG_OK     # empty batch: nothing to do


def test_abi_version_and_route(L):
    from burgers_hip import rom
    assert L.bg_abi_version() == 1
    route = rom._ROUTES["bg_hyper_rom_run_wide"]
    assert route.redo and route.wg_per_cu == 1 and route.min_n == 3 and rom._limit(route.max_n) == L.bg_fom_max_n()
    assert not rom._ROUTES["bg_hyper_rom_run"].redo
    assert issubclass(rom.HyperWidePodPlan, rom.HyperPodPlan) and rom.HyperWidePodPlan.entry == "bg_hyper_rom_run_wide"


@pytest.mark.parametrize("r,want", [(96, (288, 512)), (41, (123, 512)), (40, (120, 256))])
def test_build_row_sampling_hands_the_fit_the_limit_of_the_loop_that_takes_r(L, monkeypatch, r, want):
    from burgers_hip import pod
    seen = {}

    def fit(G, pairs, projection, tau, min_rows, max_rows):
        seen["limits"] = (min_rows, max_rows)
        return "fitted"
    monkeypatch.setattr(pod, "_fit_row_sampling", fit)
    monkeypatch.setattr(pod, "row_sampling_system", lambda *a, **k: (np.zeros((r, 600)), 1))
    X = np.linspace(0.0, 100.0, 600)
    runs = [(np.ones((600, 3)), 4.5, 0.02)]
    assert pod.build_row_sampling(X, np.zeros((600, r)), runs, 0.05, "Galerkin") == "fitted"
    assert seen["limits"] == want
    assert pod.build_row_sampling(X, np.zeros((600, r)), runs, 0.05, "LSPG", min_rows=7, max_rows=300) == "fitted"
    assert seen["limits"] == (7, 300)
