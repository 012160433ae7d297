"""CPU-side checks of bg_rom_run_blocked (the device-side POD-PROM loop for bases of up to 256 modes): the limits and
sizes it reports and the argument validation that happens before anything is launched."""
import pytest

from loop_cases import built_library, check_pod_loop_argument_validation, host_pointers


@pytest.fixture(scope="module")
def L():
    return built_library()


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
    p, _ = host_pointers()
    run = check_pod_loop_argument_validation(L, "bg_rom_run_blocked", 512, 160, 512, 256, extra=(p, 4))      # work, slots
    assert run(extra=(None, 4)) == lib.BG_ERR_WORKSPACE
    assert run(extra=(p, 0)) == lib.BG_ERR_WORKSPACE
    assert run(B=0, ops=None, hist=None, outs=None, extra=(None, 0)) == lib.BG_OK     # empty batch: nothing to do
