"""CPU-side checks of bg_rom_run_long (the device-side POD-PROM loop for meshes of 513 .. 1024 nodes): the limits and
sizes it reports and the argument validation that happens before anything is launched."""
import pytest

from loop_cases import built_library, check_pod_loop_argument_validation


@pytest.fixture(scope="module")
def L():
    return built_library()


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
    check_pod_loop_argument_validation(L, "bg_rom_run_long", 1024, 40, L.bg_rom_run_long_max_n(), L.bg_rom_run_long_max_r())


def test_existing_limits_are_unchanged(L):
    assert L.bg_rom_max_n() == 512 and L.bg_rom_run_max_r() == 40
    assert L.bg_abi_version() == 1
