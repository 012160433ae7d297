"""CPU-side checks of bg_ann_rom_run_wide_limits / bg_ann_rom_run_wide (the device-side POD-ANN time loop for up to 20
primary modes): the limits, the argument validation that happens before anything is launched, the routes of
rom.pod_ann_run -- and the conditioning of the cases the GPU test (tests/test_rom_ann_wide_gpu.py) holds the loop to."""
import ctypes

import numpy as np
import pytest

import ann_wide_cases as aw
from conftest import rel_l2
from loop_cases import built_library, host_pointers


@pytest.fixture(scope="module")
def L():
    return built_library()


def test_limits(L):
    v = [ctypes.c_int(-1) for _ in range(4)]
    assert L.bg_ann_rom_run_wide_limits(*[ctypes.byref(x) for x in v]) == 0
    assert tuple(x.value for x in v) == (20, 128, 256, 8)
    for k, want in enumerate((20, 128, 256, 8)):             # every output is optional
        one = ctypes.c_int(-1)
        assert L.bg_ann_rom_run_wide_limits(*[ctypes.byref(one) if j == k else None for j in range(4)]) == 0
        assert one.value == want
    assert L.bg_ann_rom_run_wide_limits(None, None, None, None) == 0


def test_existing_limits_are_unchanged(L):
    v = [ctypes.c_int(-1) for _ in range(4)]
    assert L.bg_ann_rom_limits(*[ctypes.byref(x) for x in v]) == 0
    assert tuple(x.value for x in v) == (8, 128, 256, 8)
    assert L.bg_abi_version() == 1


def _aligned_floats(count, offset=0):
    """A float32 host pointer ``offset`` bytes past a 16-byte boundary (and the buffer that keeps it alive)."""
    buf = (ctypes.c_float * (count + 8))()
    base = ctypes.addressof(buf)
    return ctypes.c_void_p(base + (-base) % 16 + offset), buf


def _caller(L):
    from burgers_hip import lib
    p, ip = host_pointers()
    good, keep = _aligned_floats(16)

    def run(N=512, B=4, n=17, nbar=79, nsteps=2, proj=lib.BG_PROJ_LSPG, ops=p, outs=ip, UT=None, dt=0.05, max_it=50,
            widths=None, wt=good, arrays=True, nl=None, act=lib.BG_ACT_ELU, _keep=keep):
        widths = [n, 32, nbar] if widths is None else widths
        nl = len(widths) - 1 if nl is None else nl
        m = max(nl, 1)
        wa = (ctypes.c_int * (m + 1))(*(list(widths) + [1] * (m + 1))[:m + 1])
        wts = (ctypes.c_void_p * m)(*[wt] * m)
        bs = (ctypes.c_void_p * m)(*[None] * m)
        acts = (ctypes.c_int * m)(*[act] * m)
        al = (ctypes.c_float * m)(*[1.0] * m)
        mlp = (nl, wa, wts, bs, acts, al) if arrays else (nl, None, None, None, None, None)
        return L.bg_ann_rom_run_wide(N, B, n, nbar, nsteps, proj, ops, ops if UT is None else UT, ops, ops, ops, *mlp, dt,
                                     0.0, 1e-6, max_it, lib.BG_OPT_SUPG, ops, outs, outs, outs, None, None)
    return run


def test_argument_validation_before_launch(L):
    """The codes and their order are bg_ann_rom_run's: BAD_ARG, PROJECTION, UNSUPPORTED_N, UNSUPPORTED_R, then the pointers
    and the consistency of the widths; an empty batch is BG_OK before any batch pointer is looked at."""
    from burgers_hip import lib
    run, null = _caller(L), None
    for bad in (dict(N=1), dict(B=-1), dict(n=0), dict(nbar=0), dict(nsteps=-1), dict(max_it=0), dict(dt=0.0), dict(nl=0)):
        assert run(**bad) == lib.BG_ERR_BAD_ARG, bad
    assert run(proj=9) == lib.BG_ERR_PROJECTION
    assert run(proj=9, N=513, n=21) == lib.BG_ERR_PROJECTION      # the order: projection first,
    assert run(N=513) == lib.BG_ERR_UNSUPPORTED_N
    assert run(N=513, n=21) == lib.BG_ERR_UNSUPPORTED_N           # then the mesh,
    assert run(n=21) == lib.BG_ERR_UNSUPPORTED_R                  # then the model
    assert run(nbar=129) == lib.BG_ERR_UNSUPPORTED_R
    assert run(widths=[17] + [16] * 8 + [79]) == lib.BG_ERR_UNSUPPORTED_R       # nine layers
    assert run(n=21, arrays=False) == lib.BG_ERR_UNSUPPORTED_R    # ... before the pointers
    assert run(widths=[17, 257, 79]) == lib.BG_ERR_UNSUPPORTED_R
    assert run(arrays=False) == lib.BG_ERR_BAD_ARG
    assert run(widths=[16, 32, 79]) == lib.BG_ERR_BAD_ARG         # widths[0] != n
    assert run(widths=[17, 32, 78]) == lib.BG_ERR_BAD_ARG         # widths[-1] != nbar
    assert run(widths=[17, 0, 79]) == lib.BG_ERR_UNSUPPORTED_R
    assert run(wt=null) == lib.BG_ERR_BAD_ARG
    assert run(wt=_aligned_floats(16, 4)[0]) == lib.BG_ERR_BAD_ARG                # misaligned wt[l]
    assert run(act=7) == lib.BG_ERR_BAD_ARG
    assert run(ops=null) == lib.BG_ERR_BAD_ARG                    # null operands, B > 0
    assert run(outs=null) == lib.BG_ERR_BAD_ARG
    buf = (ctypes.c_double * 8)()
    base = ctypes.addressof(buf)
    assert run(UT=ctypes.cast(base + (8 - base) % 16, ctypes.POINTER(ctypes.c_double))) == lib.BG_ERR_BAD_ARG
    assert run(B=0, ops=null, outs=null) == lib.BG_OK             # empty batch: nothing to do, no batch pointer is looked at
    for n in (1, 5, 8, 9, 20):
        assert run(B=0, n=n, ops=null, outs=null) == lib.BG_OK


class _Reached(Exception):
    pass


def test_routes(L, monkeypatch):
    """pod_ann_run(wide=True) takes bg_ann_rom_run_wide only for a model with more primary modes than bg_ann_rom_run
    covers that is inside the wide limits; everything else routes as without the flag."""
    import torch
    import torch.nn as nn
    from burgers_hip import rom
    assert rom._ROUTES[aw.WIDE].wg_per_cu == 2 and rom._ROUTES[aw.WIDE].max_n == 512
    route = rom._ann_route
    for n in (1, 5, 8, 9, 17, 20, 21):
        assert route(n, fused=False) == () and route(n, fused=False, wide=True) == ()
        assert route(n) == ("bg_ann_rom_run",)
        assert route(n, wide=True) == ((aw.WIDE, "bg_ann_rom_run") if n > 8 else ("bg_ann_rom_run",))

    # the plan builder, on CPU tensors: which models each entry point's limits let through
    cpu = torch.device("cpu")
    plan = lambda model, n, nbar, N=512, **kw: rom._ann_fused_plan(model, n, nbar, N, torch.float32, cpu, **kw)
    wide = dict(limits="bg_ann_rom_run_wide_limits")
    a17, a5 = aw.case_model(aw.CASE_A), aw.mlp([5, 32, 91], "ELU", True, 0)
    assert plan(a17, 17, 79) is None and plan(a5, 5, 91) is not None
    p = plan(a17, 17, 79, **wide)
    assert p is not None and p.args[0] == 6 and list(p.args[1]) == [17, 32, 64, 128, 256, 256, 79]
    assert [tuple(w.shape) for w in p.keep[0]] == [(20, 32), (32, 64), (64, 128), (128, 256), (256, 256), (256, 80)]
    assert plan(a5, 5, 91, **wide) is not None
    assert plan(aw.mlp([17, 300, 79], "ELU", True, 0), 17, 79, **wide) is None          # a 300-wide layer
    assert plan(aw.mlp([21, 32, 75], "ELU", True, 0), 21, 75, **wide) is None
    assert plan(aw.mlp([17, 32, 129], "ELU", True, 0), 17, 129, **wide) is None
    assert plan(aw.mlp([17] + [16] * 8 + [79], "ELU", True, 0), 17, 79, **wide) is None  # nine layers
    assert plan(a17, 17, 79, N=513, **wide) is None

    class Odd(nn.Module):
        def __init__(self):
            super().__init__()
            self.l = nn.Linear(17, 79)

        def forward(self, x):
            return 0.01 * torch.sin(self.l(x))
    assert plan(Odd(), 17, 79, **wide) is None

    # pod_ann_run: which runner it calls, and that the host path is what is left
    calls = []

    def runner(entry, takes):
        def run(X, u0, mu1, mu2, dt, nsteps, U_p, U_s, model, proj, *a, **k):
            calls.append(entry)
            n, nbar = np.shape(U_p)[1], np.shape(U_s)[1]
            lim = {"limits": "bg_ann_rom_run_wide_limits"} if entry == aw.WIDE else {}
            if plan(model, n, nbar, len(X), **lim) is None:
                return None
            raise _Reached(entry)
        return run

    def host(*a, **k):
        raise _Reached("host")
    monkeypatch.setattr(rom, "pod_ann_run_wide", runner(aw.WIDE, None))
    monkeypatch.setattr(rom, "pod_ann_run_fused", runner("bg_ann_rom_run", None))
    monkeypatch.setattr(rom, "_setup", host)

    def taken(model, n, nbar, **kw):
        calls.clear()
        X, Up, Us = aw.bases(512, n, nbar)
        with pytest.raises(_Reached) as e:
            rom.pod_ann_run(X, np.ones(512), [4.5], [0.02], 0.05, 2, Up, Us, model, **kw)
        return str(e.value), list(calls)
    assert taken(a17, 17, 79) == ("host", ["bg_ann_rom_run"])                          # wide=False: as before
    assert taken(a17, 17, 79, wide=True) == (aw.WIDE, [aw.WIDE])
    assert taken(a17, 17, 79, wide=True, fused=False) == ("host", [])
    assert taken(a17, 17, 79, wide=True, ann_dtype=torch.float64) == ("host", [])
    assert taken(a5, 5, 91, wide=True) == ("bg_ann_rom_run", ["bg_ann_rom_run"])       # n <= 8 keeps bg_ann_rom_run
    assert taken(aw.mlp([17, 300, 79], "ELU", True, 0), 17, 79, wide=True) == ("host", [aw.WIDE, "bg_ann_rom_run"])
    assert taken(Odd(), 17, 79, wide=True) == ("host", [aw.WIDE, "bg_ann_rom_run"])


def test_wide_runner_reaches_the_device_loop(L, monkeypatch):
    """pod_ann_run_wide hands the model of case A to _device_loop with the bg_ann_rom_run_wide route, the UT layout the
    header documents ([n + nbar][512], zero columns from N) and the plan's closure arguments."""
    import torch
    from burgers_hip import lib, rom
    seen = {}

    def device_loop(route, Xh, u0, mu1, mu2, nsteps, device, options, balance, launch, keep=(), slots=None):
        seen.update(route=route.entry, keep=keep, N=len(Xh))
        raise _Reached(route.entry)
    monkeypatch.setattr(rom, "_device_loop", device_loop)
    monkeypatch.setattr(lib, "require_device", lambda device=None: torch.device("cpu"))
    monkeypatch.setattr(rom, "_as_dev", lambda a, device: torch.as_tensor(np.array(a, dtype=np.float64)))
    X, Up, Us = aw.bases(301, 13, 40)
    model = aw.case_model(aw.SHAPE_CASES[3])
    with pytest.raises(_Reached):
        rom.pod_ann_run_wide(X, np.ones(301), [4.5], [0.02], 0.05, 2, Up, Us, model, rom.PROJ["lspg"])
    plan, UT = seen["keep"]
    assert seen["route"] == aw.WIDE and tuple(UT.shape) == (53, 512)
    assert np.array_equal(UT[:13, :301].numpy(), Up.T) and np.array_equal(UT[13:, :301].numpy(), Us.T)
    assert float(UT[:, 301:].abs().max()) == 0.0 and list(plan.args[1]) == [13, 130, 50, 40]
    # outside the limits: None, and nothing is launched
    assert rom.pod_ann_run_wide(X, np.ones(301), [4.5], [0.02], 0.05, 2, Up, Us, aw.mlp([13, 300, 40], "ELU", True, 0),
                                rom.PROJ["lspg"]) is None


_MUS = ((4.3, 0.016), (5.4, 0.029))      # two corners of the thesis box


@pytest.mark.parametrize("case", aw.ALL_CASES, ids=[c[0] for c in aw.ALL_CASES])
@pytest.mark.parametrize("proj", ["LSPG", "Galerkin"])
def test_cases_are_well_conditioned(case, proj):
    """Every case of the GPU test by the oracle alone: finite, and every step far from the 50-iteration cap, so that 'no
    flags, no info' is a condition the reference meets.  The oracle restates the ELU network only: a case with another
    activation runs with ELU in its place, which keeps its basis, shape, seed and scale."""
    elu = case[:5] + ("ELU",) + case[6:]
    for mu1, mu2 in _MUS:
        U, it = aw.oracle(elu, mu1, mu2, 5, proj)
        print(f"{case[0]} {proj} mu=({mu1}, {mu2}): iterations {it.tolist()}")
        assert np.isfinite(U).all() and it.max() <= 25


@pytest.mark.parametrize("proj", ["LSPG", "Galerkin"])
def test_case_a_is_tangent_sensitive(proj):
    """Case A at scale 3.0 with columns 0 and 16 of the closure Jacobian exchanged moves the 5-step history by at least ten
    times the float32 gate (at scale 0.02 by less than the gate itself): a loop with a wrong tangent row cannot pass."""
    shifts = []
    for mu1, mu2 in _MUS:
        U, _ = aw.oracle(aw.CASE_A, mu1, mu2, 5, proj)
        Us, _ = aw.oracle(aw.CASE_A, mu1, mu2, 5, proj, swap=(0, 16))
        shifts.append(rel_l2(Us, U))
    print(f"case A, scale 3.0, {proj}: history shift under the Jacobian swap {shifts}")
    assert max(shifts) >= 10 * aw.TOL32
