"""CPU-side checks of bg_rom_run_long_wide (the device-side POD-PROM loop for 41 .. 96 modes on meshes of 513 .. 1024 nodes):
the limits and sizes it reports, the argument validation that happens before anything is launched, its row of the route
table and the refusals of its plan."""
import numpy as np
import pytest

from loop_cases import built_library, check_pod_loop_argument_validation

ENTRY = "bg_rom_run_long_wide"


@pytest.fixture(scope="module")
def L():
    return built_library()


def test_limits(L):
    assert L.bg_rom_run_long_wide_max_n() >= 1024
    assert L.bg_rom_run_long_wide_max_r() == L.bg_rom_run_wide_max_r()


def test_element_counts(L):
    for N in (513, 600, 1024):
        assert L.bg_rom_run_long_wide_phi_elems(N) == ((N + 63) // 64 * 64 + 2) * 96
    counts = [L.bg_rom_run_long_wide_phi_elems(N) for N in range(513, L.bg_rom_run_long_wide_max_n() + 1)]
    assert counts == sorted(counts)


def test_argument_validation_before_launch(L):
    check_pod_loop_argument_validation(L, ENTRY, 1024, 96, L.bg_rom_run_long_wide_max_n(), L.bg_rom_run_long_wide_max_r())


def test_existing_limits_are_unchanged(L):
    assert L.bg_rom_max_n() == 512
    assert L.bg_rom_run_wide_max_r() == 96 and L.bg_rom_run_long_max_r() == 40
    assert L.bg_abi_version() == 1


def test_route_table(L):
    from burgers_hip import rom
    route = rom._pod_route
    max_n = L.bg_rom_run_long_wide_max_n()
    for N in (513, max_n):
        assert route(N, 41, long_wide=True) == ENTRY
        assert route(N, 96, long_wide=True) == ENTRY
        assert route(N, 97, long_wide=True) == "library"
        assert route(N, 40, long_wide=True) == "library"                 # bg_rom_run_long is the loop for these
        assert route(N, 40, long_wide=True, long_mesh=True) == "bg_rom_run_long"
        assert route(N, 96, long_wide=True, fused=False) == "library"
    assert route(512, 96, long_wide=True) == "bg_rom_run_wide"
    assert route(max_n + 1, 96, long_wide=True) == "library"
    assert ENTRY in rom._ROUTES and rom._ROUTES[ENTRY].redo


def test_plan_refuses_before_the_device(L):
    """Without a device a plan that reached its device copy raises RuntimeError: ValueError means the shape checks came
    first."""
    import torch
    from burgers_hip import rom
    max_n = L.bg_rom_run_long_wide_max_n()
    for Phi in (np.zeros(600), np.zeros((600, 0)), np.zeros((600, 97)), np.zeros((max_n + 1, 3))):
        with pytest.raises(ValueError):
            rom.LongWidePodPlan(Phi, None)
    if not torch.cuda.is_available():                                  # a basis that passes goes on to the device
        with pytest.raises(RuntimeError):
            rom.LongWidePodPlan(np.zeros((600, 96)), None)
