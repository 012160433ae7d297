"""CPU-side checks of the host side of the device-side time loops (burgers_hip/rom.py): which route an (N, r, flags) takes
(the table in DESIGN.md, "Host side of the device-side loops"; the expected names below are written out from the ladders
the route functions replaced), what the plans refuse before they touch a device, and lib.limits."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from burgers_hip import build, lib
    build.build_library()
    return lib.load()


RUN, WIDE, BLOCKED, LONG = "bg_rom_run", "bg_rom_run_wide", "bg_rom_run_blocked", "bg_rom_run_long"


def test_pod_route_table(L):
    from burgers_hip.rom import _pod_route as route
    r_run, r_wide, r_blk, r_red = L.bg_rom_run_max_r(), L.bg_rom_run_wide_max_r(), L.bg_rom_run_blocked_max_r(), L.bg_rom_max_r()
    n_long, r_long = L.bg_rom_run_long_max_n(), L.bg_rom_run_long_max_r()
    assert r_run < r_red < r_wide < r_blk and r_long <= r_red and n_long > 513       # what the rows below presuppose
    for N in (17, 512):
        assert route(N, 1) == RUN and route(N, r_run) == RUN
        assert route(N, r_run + 1) == WIDE and route(N, r_wide) == WIDE
        for blocked in (False, True):                        # up to the wide limit ``blocked`` changes nothing
            assert route(N, r_run, blocked=blocked) == RUN
            assert route(N, r_wide, blocked=blocked) == WIDE
        assert route(N, r_wide + 1) == "library" and route(N, r_wide + 1, blocked=True) == BLOCKED
        assert route(N, r_blk) == "library" and route(N, r_blk, blocked=True) == BLOCKED
        assert route(N, r_blk + 1) == "library" and route(N, r_blk + 1, blocked=True) == "library"
        # fused=False: the host-driven iteration up to the reduce kernels' r, the library path beyond; no device loop
        assert route(N, r_run, fused=False) == "host" and route(N, r_red, fused=False) == "host"
        assert route(N, r_red + 1, fused=False) == "library"
        assert route(N, r_wide, fused=False, blocked=True, long_mesh=True) == "library"
        assert route(N, r_red) == WIDE and route(N, r_red + 1) == WIDE       # fused: the wide loop wins over both
        assert route(N, r_run, long_mesh=True) == RUN                       # long_mesh starts above 512 nodes
    for N in (513, n_long):
        assert route(N, 3) == "library" and route(N, r_long) == "library"
        assert route(N, 3, long_mesh=True) == LONG and route(N, r_long, long_mesh=True) == LONG
        assert route(N, r_long + 1, long_mesh=True) == "library"
        assert route(N, 3, fused=False, long_mesh=True) == "library"
        assert route(N, r_wide, blocked=True) == "library" and route(N, r_blk, blocked=True) == "library"
    assert route(n_long + 1, 3) == "library" and route(n_long + 1, 3, long_mesh=True) == "library"


def test_quad_route_table(L):
    from burgers_hip.rom import _quad_route as route
    n_max, N_long, n_long = L.bg_quad_rom_max_n(), L.bg_quad_rom_run_long_max_n(), L.bg_quad_rom_run_long_max_r()
    Q, QL = "bg_quad_rom_run", "bg_quad_rom_run_long"
    for N in (17, 512):
        for long_mesh in (False, True):
            assert route(N, 1, long_mesh=long_mesh) == Q and route(N, n_max, long_mesh=long_mesh) == Q
            assert route(N, n_max + 1, long_mesh=long_mesh) == "host"
            assert route(N, n_max, fused=False, long_mesh=long_mesh) == "host"
    for N in (513, N_long):
        assert route(N, 1) == "host" and route(N, n_long) == "host"
        assert route(N, 1, long_mesh=True) == QL and route(N, n_long, long_mesh=True) == QL
        assert route(N, n_long + 1, long_mesh=True) == "host"
        assert route(N, n_long, fused=False, long_mesh=True) == "host"
    assert route(N_long + 1, 1, long_mesh=True) == "host"


def test_local_route_table(L):
    """local_prom_run tries these loops in this order and takes the first whose LocalPodPlan is ``ok``; nothing left: host."""
    from burgers_hip import lib
    from burgers_hip.rom import _local_route as route
    F, FL = "bg_local_rom_run", "bg_local_rom_run_long"
    n_long = lib.limits("bg_local_rom_run_long_limits", 4)[0]
    for N in (17, 512, 513, n_long, n_long + 1):
        assert route(N) == () and route(N, long_mesh=True) == ()              # the default is the host-driven iteration
        assert route(N, fused=True) == (F,)                                  # (its plan declines N > 512)
    for N in (17, 512):
        assert route(N, fused=True, long_mesh=True) == (F,)                  # long_mesh starts above 512 nodes
    for N in (513, n_long, n_long + 1):
        assert route(N, fused=True, long_mesh=True) == (FL, F)               # (the long plan declines N > its max_n)


def _pod_plan_cases(L):
    from burgers_hip import rom
    return [(rom.WidePodPlan, L.bg_rom_run_wide_max_r(), 200, (1, 513)),
            (rom.BlockedPodPlan, L.bg_rom_run_blocked_max_r(), 200, (2, 513)),
            (rom.LongPodPlan, L.bg_rom_run_long_max_r(), 600, (2, L.bg_rom_run_long_max_n() + 1))]


def test_pod_plans_refuse_before_the_device(L):
    """Without a device a plan that reached its device copy raises RuntimeError: ValueError means the shape checks came
    first.  (With a device the same refusals hold; a basis that passes them is then simply built.)"""
    import torch
    for plan, max_r, N, bad_n in _pod_plan_cases(L):
        for Phi in (np.zeros(N), np.zeros((N, 0)), np.zeros((N, max_r + 1))) + tuple(np.zeros((n, 3)) for n in bad_n):
            with pytest.raises(ValueError):
                plan(Phi, None)
        if not torch.cuda.is_available():                                  # a basis that passes goes on to the device
            with pytest.raises(RuntimeError):
                plan(np.zeros((N, max_r)), None)


def test_quad_long_plan_refuses_before_the_device(L):
    import torch
    from burgers_hip import rom
    n_max, N_max = L.bg_quad_rom_run_long_max_r(), L.bg_quad_rom_run_long_max_n()
    pair = lambda N, n: (np.zeros((N, n)), np.zeros((N, n * (n + 1) // 2)))
    for Phi, H in ((np.zeros(600), np.zeros((600, 1))), pair(600, 0), pair(600, n_max + 1), pair(512, 8), pair(N_max + 1, 8)):
        with pytest.raises(ValueError):
            rom.QuadLongPlan(Phi, H, None)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            rom.QuadLongPlan(*pair(600, n_max), None)


@pytest.mark.parametrize("name,count", [("bg_ann_rom_limits", 4), ("bg_rbf_rom_limits", 3), ("bg_local_rom_limits", 3),
                                        ("bg_local_rom_run_long_limits", 4)])
def test_limits_match_a_direct_call(L, name, count):
    from burgers_hip import lib
    out = [ctypes.c_int(-1) for _ in range(count)]
    assert getattr(L, name)(*[ctypes.byref(v) for v in out]) == lib.BG_OK
    got = lib.limits(name, count)
    assert isinstance(got, tuple) and got == tuple(v.value for v in out) and all(v > 0 for v in got)
