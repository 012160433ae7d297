"""CPU-side checks of the device-side pivoting of bg_hyper_rom_run_wide and of bg_wide_solve_pivoted: the symbol and its
binding, the return codes that come back before anything is launched, the option constant, and the ``pivot`` keyword's
refusals."""
import re

import numpy as np
import pytest

from conftest import REPO, mesh
from loop_cases import built_library, host_pointers


@pytest.fixture(scope="module")
def L():
    return built_library()


def test_symbol_is_exported_bound_and_declared(L):
    from burgers_hip import lib
    assert hasattr(L, "bg_wide_solve_pivoted") and "bg_wide_solve_pivoted" in lib.declared_symbols()
    header = open(f"{REPO}/include/burgers_hip.h").read()
    assert re.search(r"\bint bg_wide_solve_pivoted\(int B, int n, const double \*A, const double \*b, double \*x, int32_t \*piv, "
                     r"int32_t \*info, void \*stream\);", header)
    assert len(L.bg_wide_solve_pivoted.argtypes) == 8


def test_return_codes_without_a_launch(L):
    from burgers_hip import lib
    p, ip = host_pointers()
    null = None
    for n in (0, -1, 97, 1000):
        assert L.bg_wide_solve_pivoted(4, n, p, p, p, ip, ip, null) == lib.BG_ERR_UNSUPPORTED_R
    assert L.bg_wide_solve_pivoted(0, 97, null, null, null, null, null, null) == lib.BG_ERR_UNSUPPORTED_R
    for n in (1, 41, 96):
        assert L.bg_wide_solve_pivoted(0, n, null, null, null, null, null, null) == lib.BG_OK      # empty batch: nothing to do
        assert L.bg_wide_solve_pivoted(-1, n, p, p, p, ip, ip, null) == lib.BG_ERR_BAD_ARG
        assert L.bg_wide_solve_pivoted(4, n, null, p, p, ip, ip, null) == lib.BG_ERR_BAD_ARG
        assert L.bg_wide_solve_pivoted(4, n, p, null, p, ip, ip, null) == lib.BG_ERR_BAD_ARG
        assert L.bg_wide_solve_pivoted(4, n, p, p, null, ip, ip, null) == lib.BG_ERR_BAD_ARG
        assert L.bg_wide_solve_pivoted(4, n, p, p, p, ip, null, null) == lib.BG_ERR_BAD_ARG


def test_option_constant_and_abi_version(L):
    from burgers_hip import lib
    assert lib.BG_OPT_PIVOT_ON_DEVICE == 256 and L.bg_abi_version() == 1
    header = open(f"{REPO}/include/burgers_hip.h").read()
    assert re.search(r"\bBG_OPT_PIVOT_ON_DEVICE = 256\b", header) and re.search(r"#define BG_ABI_VERSION 1\b", header)
    others = (lib.BG_OPT_SUPG, lib.BG_OPT_NONUNIFORM, lib.BG_OPT_W_COLMAJOR, lib.BG_OPT_MFMA_16X16, lib.BG_OPT_FORCE_PIVOTED,
              lib.BG_OPT_NO_TANGENT_REUSE, lib.BG_OPT_FOM_WIDE, lib.BG_OPT_FOM_WAVE)
    assert all(lib.BG_OPT_PIVOT_ON_DEVICE & o == 0 for o in others)


def test_pivot_keyword_is_refused_before_a_launch(L, monkeypatch):
    from burgers_hip import lib, pod, rom
    from fem_burgers import FEMBurgers

    def no_launch(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(rom, "_device_loop", no_launch)
    monkeypatch.setattr(lib, "require_device", no_launch)
    N = 64
    X, T = mesh(N)
    s = pod.RowSampling(np.arange(N, dtype=np.int32), np.ones(N), "galerkin", 0.0, 0, 0.0)
    args = (X, np.ones(N), [4.5], [0.02], 0.05, 2)
    for bad in ("both", "Device", "", None, True):
        for Phi in (np.zeros((N, 48)), np.zeros((N, 8))):           # the wide loop's width and the narrow loop's
            with pytest.raises(ValueError, match="pivot"):
                rom.pod_prom_run_hyper(*args, Phi, s, rom.PROJ["galerkin"], pivot=bad)
            with pytest.raises(ValueError, match="pivot"):
                rom.pod_prom_run(*args, Phi, hyper=s, pivot=bad)
            with pytest.raises(ValueError, match="pivot"):
                FEMBurgers(X, T).pod_prom_burgers(0.05, 2, np.ones(N), 4.5, 0.0, 0.02, Phi, hyper=s, pivot=bad)
        with pytest.raises(ValueError, match="pivot"):
            rom.pod_prom_run_hyper_wide(*args, np.zeros((N, 48)), s, rom.PROJ["galerkin"], pivot=bad)
