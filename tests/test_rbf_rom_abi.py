"""CPU-side checks of bg_rbf_rom_limits / bg_rbf_rom_run (the device-side POD-RBF time loop): the limits it reports and
the argument validation that happens before anything is launched."""
import ctypes

import pytest

from loop_cases import built_library, host_pointers


@pytest.fixture(scope="module")
def L():
    return built_library()


def test_limits_cover_the_issue_sizes(L):
    v = [ctypes.c_int() for _ in range(3)]
    assert L.bg_rbf_rom_limits(*[ctypes.byref(x) for x in v]) == 0
    max_n, max_nbar, max_ns = (x.value for x in v)
    assert max_n >= 20 and max_nbar >= 128 and max_ns >= 4096


def test_argument_validation_before_launch(L):
    from burgers_hip import lib
    null = None
    p, ip = host_pointers()

    def run(N=512, B=4, n=17, nbar=79, Ns=300, nsteps=2, proj=lib.BG_PROJ_LSPG, kind=lib.BG_RBF_GAUSSIAN, ops=p, outs=ip):
        return L.bg_rbf_rom_run(N, B, n, nbar, Ns, nsteps, proj, kind, ops, ops, ops, ops, ops, ops, ops, 1.0, ops, ops, ops,
                                0.05, 0.0, 1e-6, 30, lib.BG_OPT_SUPG, ops, outs, outs, outs, null, null)

    assert run(N=2) == lib.BG_ERR_BAD_ARG
    assert run(n=0) == lib.BG_ERR_BAD_ARG
    assert run(nbar=0) == lib.BG_ERR_BAD_ARG
    assert run(Ns=0) == lib.BG_ERR_BAD_ARG
    assert run(B=-1) == lib.BG_ERR_BAD_ARG
    assert run(kind=7) == lib.BG_ERR_BAD_ARG
    assert run(proj=9) == lib.BG_ERR_PROJECTION
    assert run(N=513) == lib.BG_ERR_UNSUPPORTED_N
    assert run(n=21) == lib.BG_ERR_UNSUPPORTED_R
    assert run(nbar=129) == lib.BG_ERR_UNSUPPORTED_R
    assert run(ops=null) == lib.BG_ERR_BAD_ARG          # null operands, B > 0
    assert run(outs=null) == lib.BG_ERR_BAD_ARG
    assert run(B=0, ops=null, outs=null) == lib.BG_OK    # empty batch: nothing to do
