"""bg_lu_solve and bg_lu_solve_update (csrc/rom.hip, lu_pivoted_wave in csrc/rom_device.hpp): the solve and the convergence
bookkeeping of the host-driven iteration, which every device-side loop is tested against.  Every NMAX rung of dispatch_lu
from both sides, the value of `info`, pivot ties in the 32-bit pivot search, and the update rules, flags and counters of
include/burgers_hip.h ("mode 1 / 2 / 3") at the cap, at zero denominators, with singular systems and with inactive
samples.  Accuracy bound: rel-L2 < 1e-13 max(10, cond(A)) per system against np.linalg.solve (tests/test_rom_gpu.py).
References: float64 numpy written here, and rom._IterState._solve_update_library, the project's second implementation of
the same rules."""
import types

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
Q_SENTINEL, I_SENTINEL = -7.0, -99


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _bound(A):
    return 1e-13 * np.maximum(10.0, np.linalg.cond(A))


def _needs_pivoting(rng, B, n):
    """The matrices of test_lu_solve_vs_numpy: randn + 0.1 I, one sample row-reversed (tiny leading pivots)."""
    A = rng.standard_normal((B, n, n)) + 0.1 * np.eye(n)
    A[3] = A[3][::-1].copy()
    return A


def _scaled_permutation(rng, n, zero_col=None):
    """diag(2^e) P: the elimination is exact (every multiplier is 0).  ``zero_col``: that column zeroed, so that the
    first zero pivot is the one of step ``zero_col`` (LAPACK's dgetrf: info = zero_col + 1)."""
    A = np.zeros((n, n))
    A[np.arange(n), rng.permutation(n)] = 2.0 ** rng.integers(-3, 4, n)
    if zero_col is not None:
        A[:, zero_col] = 0.0
    return A


# ------------------------------------------------------------------------------------ bg_lu_solve
@pytest.mark.parametrize("n", [9, 16, 17, 32, 33, 48, 49])
def test_lu_solve_rungs(hip, n):
    """The NMAX rungs 16 and 32 and both sides of every rung (with test_lu_solve_vs_numpy: 8 | 9, 16 | 17, ... 48 | 49).
    A rung whose identity padding, right-hand-side column or back substitution is off by one row fails here."""
    from burgers_hip import rom
    rng = np.random.default_rng(100 + n)
    B = 37
    A = _needs_pivoting(rng, B, n)
    b = rng.standard_normal((B, n))
    x, info = rom.lu_solve(_dev(A), _dev(b), -1.0)
    torch.cuda.synchronize()
    ref = np.linalg.solve(A, -b[..., None])[..., 0]
    assert (info.cpu().numpy() == 0).all()
    rel = np.linalg.norm(x.cpu().numpy() - ref, axis=1) / np.linalg.norm(ref, axis=1)
    assert (rel < _bound(A)).all(), float((rel / _bound(A)).max())


@pytest.mark.parametrize("n", [12, 40, 64])
def test_info_is_first_zero_pivot_plus_one(hip, n):
    """info == k + 1 for a zero pivot at step k = 0, n // 2, n - 1 (an off-by-one, or the LAST zero pivot, fails); the
    healthy system of the same workgroup keeps info == 0 and gets its solution.  And the contract rom._IterState relies
    on across iterations: info is only ever written with a non-zero value, so a sentinel survives a healthy system."""
    from burgers_hip import rom
    rng = np.random.default_rng(n)
    ks = [0, n // 2, n - 1]
    A = np.stack([_scaled_permutation(rng, n)] + [_scaled_permutation(rng, n, k) for k in ks])
    b = rng.integers(1, 9, (4, n)).astype(np.float64)
    x, info = rom.lu_solve(_dev(A), _dev(b), 1.0)
    torch.cuda.synchronize()
    assert info.cpu().numpy().tolist() == [0] + [k + 1 for k in ks]
    assert rel_l2(x[0].cpu().numpy(), np.linalg.solve(A[0], b[0])) < 1e-12          # 1e-13 max(10, cond), cond <= 64
    info = torch.full((4,), I_SENTINEL, dtype=torch.int32, device="cuda")
    rom.lu_solve(_dev(A), _dev(b), 1.0, info=info)
    torch.cuda.synchronize()
    assert info.cpu().numpy().tolist() == [I_SENTINEL] + [k + 1 for k in ks]


@pytest.mark.parametrize("n,col", [(24, 0), (24, 12), (40, 17)])
def test_pivot_ties_in_the_top_32_bits(hip, n, col):
    """The pivot search compares the high dword of |a[k]| only.  Two candidates of column ``col`` agree there and differ
    below, the larger in the higher row, so the search takes the other one than LAPACK: the solution must stay within the
    bound.  The block below-left of (col, col) is zero, so the rows from ``col`` on reach step ``col`` untouched and the
    tie is the one written here."""
    from burgers_hip import rom
    rng = np.random.default_rng(n + col)
    B = 6
    A = np.clip(rng.standard_normal((B, n, n)), -2.5, 2.5) + 0.1 * np.eye(n)
    A[:, col:, :col] = 0.0
    lo_row, hi_row = col + 1, min(n - 1, col + 5)
    A[:, lo_row, col] = 3.0
    A[:, hi_row, col] = 3.0 + 2.0 ** -24                                      # same high dword, larger
    A[1, lo_row, col], A[1, hi_row, col] = -3.0, 3.0 + 2.0 ** -30              # and with opposite signs
    hi = A[:, [lo_row, hi_row], col].copy().view(np.uint64) >> 32
    assert ((hi[:, 0] & 0x7fffffff) == (hi[:, 1] & 0x7fffffff)).all()
    b = rng.standard_normal((B, n))
    x, info = rom.lu_solve(_dev(A), _dev(b), 1.0)
    torch.cuda.synchronize()
    ref = np.linalg.solve(A, b[..., None])[..., 0]
    assert (info.cpu().numpy() == 0).all()
    rel = np.linalg.norm(x.cpu().numpy() - ref, axis=1) / np.linalg.norm(ref, axis=1)
    assert (rel < _bound(A)).all(), float((rel / _bound(A)).max())


# ------------------------------------------------------------------------------------ bg_lu_solve_update
def _rules(mode, dq, base, k0, tol, max_it):
    """Header lines "mode 1 / 2 / 3" in float64 numpy: (q, err, go on, flags, iters) of one update."""
    from burgers_hip import lib
    q = base + dq
    nd, nq = np.linalg.norm(dq, axis=1), np.linalg.norm(q, axis=1)
    k = k0 + 1
    with np.errstate(all="ignore"):
        if mode == 1:
            err = nd / nq; more = (err > tol) & (k < max_it)
        elif mode == 2:
            err = nd / np.where(nq > 1e-14, nq, 1e-14); more = ~(err < tol) & (k < max_it)
        else:
            err = nd / (nq + 1e-14); more = (err > tol) & (k < max_it)
    capped = (k >= max_it) & (~(err < tol) if mode == 2 else True)
    flags = np.where(np.isfinite(err), 0, lib.BG_FLAG_NONFINITE) | np.where(capped, lib.BG_FLAG_HIT_CAP, 0)
    return q, err, more, flags.astype(np.int32), k.astype(np.int32)


class _Call:
    """One bg_lu_solve_update launch.  Every output starts from what a caller would hold (``iters``, ``flags``) or from a
    sentinel (``dq``, ``info``, mode 1's ``q``), so that what the kernel did not write shows."""

    def __init__(self, hip, A, b, mode, base, active, iters, flags, tol, max_it):
        B, n = b.shape
        i32 = dict(dtype=torch.int32, device="cuda")
        self.mode, self.base, self.act0, self.k0, self.fl0 = mode, base, np.asarray(active), np.asarray(iters), np.asarray(flags)
        self.q0 = np.full((B, n), Q_SENTINEL) if mode == 1 else base.copy()
        self.Ad, self.bd = _dev(A), _dev(b)
        self.wtu = _dev(base) if mode == 1 else None
        self.q, self.dq = _dev(self.q0), torch.full((B, n), Q_SENTINEL, dtype=torch.float64, device="cuda")
        self.act, self.k, self.fl = (torch.as_tensor(np.asarray(v), **i32) for v in (active, iters, flags))
        self.info = torch.full((B,), I_SENTINEL, **i32)
        self.counter = torch.zeros((2, hip.BG_COUNTER_SLOTS, hip.BG_COUNTER_STRIDE), **i32)
        hip.check(hip.load().bg_lu_solve_update(n, B, hip.ptr(self.Ad), hip.ptr(self.bd), mode, hip.ptr(self.wtu),
                                                hip.ptr(self.q), hip.ptr(self.dq), tol, max_it, hip.ptr(self.act),
                                                hip.ptr(self.k), hip.ptr(self.fl), hip.ptr(self.counter), hip.ptr(self.info),
                                                hip.stream_ptr(torch.device("cuda", 0))), "bg_lu_solve_update")
        torch.cuda.synchronize()
        self.out = {k: getattr(self, k).cpu().numpy() for k in ("q", "dq", "act", "k", "fl", "info", "counter")}

    def check_inactive_untouched(self):
        off = self.act0 == 0
        o = self.out
        assert np.array_equal(o["q"][off], self.q0[off]) and (o["dq"][off] == Q_SENTINEL).all()
        assert np.array_equal(o["k"][off], self.k0[off]) and np.array_equal(o["fl"][off], self.fl0[off])
        assert (o["info"][off] == I_SENTINEL).all() and (o["act"][off] == 0).all()

    def check_counter(self, hip, singular):
        """Sample b adds to element [row][b % BG_COUNTER_SLOTS][0]: row 0 if it goes on, row 1 if it was active and
        singular; every other element of the two rows stays 0."""
        B = len(self.act0)
        want = np.zeros((2, hip.BG_COUNTER_SLOTS, hip.BG_COUNTER_STRIDE), dtype=np.int32)
        np.add.at(want[0, :, 0], np.arange(B) % hip.BG_COUNTER_SLOTS, self.out["act"])
        np.add.at(want[1, :, 0], np.arange(B) % hip.BG_COUNTER_SLOTS, ((self.act0 == 1) & singular).astype(np.int32))
        assert np.array_equal(self.out["counter"], want)


def _library(mode, A, b, base, active, iters, flags, tol, max_it):
    """The same update through rom._IterState._solve_update_library (rocSOLVER LU + torch)."""
    from burgers_hip import rom
    B, n = b.shape
    st = rom._IterState(types.SimpleNamespace(B=B, device=torch.device("cuda", 0)), n)
    st.active.copy_(_dev(np.asarray(active, dtype=np.int32))); st.k.copy_(_dev(np.asarray(iters, dtype=np.int32)))
    st.flags.copy_(_dev(np.asarray(flags, dtype=np.int32)))
    q = _dev(base.copy())
    left = st._solve_update_library(mode, _dev(A), _dev(b), _dev(base) if mode == 1 else None, q, tol, max_it)
    return q.cpu().numpy(), st.active.cpu().numpy(), st.k.cpu().numpy(), st.flags.cpu().numpy(), left


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 8, 9, 24, 33, 48, 64])
def test_lu_update_rungs(hip, n, mode):
    """Every NMAX rung of the fused update from both sides (with the n = 40 of test_lu_solve_update_large_batch), on
    matrices that need pivoting, B = 13 (three full workgroups of four systems and one with a single live wave), with
    inactive samples, non-zero starting counts and flags.  Catches a rung that drops a row of q, reads wtu where it
    should read q, or counts / flags from the wrong sample."""
    rng = np.random.default_rng(1000 * mode + n)
    B, tol, max_it = 13, 0.5, 20
    A = _needs_pivoting(rng, B, n)
    b, base = rng.standard_normal((B, n)), rng.standard_normal((B, n))
    active = np.ones(B, dtype=np.int32); active[[2, 7, 12]] = 0
    iters = rng.integers(0, 5, B).astype(np.int32)
    flags = np.zeros(B, dtype=np.int32); flags[[1, 2]] = 4                  # a bit of the caller's own: or-ed, not overwritten
    c = _Call(hip, A, b, mode, base, active, iters, flags, tol, max_it)
    o, on = c.out, active == 1
    dq_ref = np.linalg.solve(A, -b[..., None])[..., 0]
    bound = _bound(A)
    rel = np.linalg.norm(o["dq"] - dq_ref, axis=1) / np.linalg.norm(dq_ref, axis=1)
    assert (rel[on] < bound[on]).all(), float((rel[on] / bound[on]).max())
    q_ref, err, more, fl_ref, k_ref = _rules(mode, dq_ref, base, iters, tol, max_it)
    relq = np.linalg.norm(o["q"] - q_ref, axis=1) / np.linalg.norm(q_ref, axis=1)
    assert (relq[on] < 10 * bound[on]).all()
    assert np.array_equal(o["q"][on], (base + o["dq"])[on])                  # the update itself is one exact addition
    clear = np.abs(err - tol) > 1e-6                                         # away from the threshold the decision is exact
    assert clear.sum() >= B - 2
    assert np.array_equal(o["act"][on & clear], more[on & clear].astype(np.int32))
    assert np.array_equal(o["k"][on], k_ref[on]) and np.array_equal(o["fl"][on], (flags | fl_ref)[on])
    assert (o["info"] == I_SENTINEL).all()
    c.check_inactive_untouched()
    c.check_counter(hip, np.zeros(B, dtype=bool))
    ql, actl, kl, fll, left = _library(mode, A, b, base, active, iters, flags, tol, max_it)
    assert np.array_equal(actl[clear], o["act"][clear]) and np.array_equal(kl, o["k"]) and np.array_equal(fll, o["fl"])
    assert left == int(o["act"].sum()) or not clear.all()
    assert (np.linalg.norm(ql - np.where(on[:, None], o["q"], base), axis=1) <= 10 * bound * np.linalg.norm(q_ref, axis=1)).all()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_counter_slots_wrap(hip, mode):
    """B = 37 > BG_COUNTER_SLOTS: samples b, b + 16, b + 32 share a slot; the existing tests check only the rows' sums."""
    rng = np.random.default_rng(mode)
    B, n = 37, 5
    A = rng.standard_normal((B, n, n)) + 6.0 * np.eye(n)
    b, base = rng.standard_normal((B, n)), rng.standard_normal((B, n))
    active = (rng.random(B) < 0.8).astype(np.int32)
    zero = np.zeros(B, dtype=np.int32)
    err = np.sort(_rules(mode, np.linalg.solve(A, -b[..., None])[..., 0], base, zero, 0.0, 20)[1][active == 1])
    tol = 0.5 * (err[len(err) // 2 - 1] + err[len(err) // 2])               # half of the active samples go on
    assert err[len(err) // 2] - err[len(err) // 2 - 1] > 1e-6
    c = _Call(hip, A, b, mode, base, active, zero, zero, tol, 20)
    assert c.out["act"].sum() == len(err) - len(err) // 2
    c.check_counter(hip, np.zeros(B, dtype=bool))
    c.check_inactive_untouched()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_cap(hip, mode):
    """iters = max_it - 1 with an error well above tol (samples 0, 1) and well below it (2, 3); sample 4 has an
    iteration to spare.  active == 0 and iters == max_it; HIT_CAP in modes 1 and 3 in both cases (their loop condition
    is `k < max_it`), in mode 2 only when the error is not below tol (its loop breaks on err < tol first)."""
    from burgers_hip import lib
    n, tol, max_it = 12, 1e-3, 9
    rng = np.random.default_rng(5)
    A = np.tile(np.eye(n), (5, 1, 1))
    base = 1.0 + rng.random((5, n))
    b = rng.standard_normal((5, n)); b[2:4] *= 1e-7
    iters = np.array([8, 8, 8, 8, 7], dtype=np.int32)
    c = _Call(hip, A, b, mode, base, np.ones(5, dtype=np.int32), iters, np.zeros(5, dtype=np.int32), tol, max_it)
    _, err, more, fl_ref, k_ref = _rules(mode, -b, base, iters, tol, max_it)
    assert (err[[0, 1, 4]] > 10 * tol).all() and (err[2:4] < 0.1 * tol).all()
    o = c.out
    assert o["act"].tolist() == [0, 0, 0, 0, 1] and o["k"].tolist() == [9, 9, 9, 9, 8]
    small = 0 if mode == 2 else lib.BG_FLAG_HIT_CAP
    assert o["fl"].tolist() == [lib.BG_FLAG_HIT_CAP] * 2 + [small] * 2 + [0]
    assert np.array_equal(o["fl"], fl_ref) and np.array_equal(o["act"], more.astype(np.int32)) and np.array_equal(o["k"], k_ref)
    c.check_counter(hip, np.zeros(5, dtype=bool))
    _, actl, kl, fll, left = _library(mode, A, b, base, np.ones(5, dtype=np.int32), iters, np.zeros(5, dtype=np.int32), tol, max_it)
    assert np.array_equal(actl, o["act"]) and np.array_equal(kl, o["k"]) and np.array_equal(fll, o["fl"]) and left == 1


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_zero_denominators(hip, mode):
    """A = I, so dq = -b exactly.  Sample 0: b = base, the new q is exactly 0.  Sample 1: b = base = 0, dq and q are 0.
    Sample 2: ordinary.  Mode 1 divides by |q|: inf (flagged, goes on while k < max_it) and NaN (flagged, stopped: NaN > tol
    is false).  Modes 2 and 3 guard the denominator with 1e-14: |dq| / 1e-14 is finite (goes on, no flag), 0 / 1e-14 = 0
    (stops, no flag)."""
    from burgers_hip import lib
    n, tol, max_it = 9, 1e-6, 20
    rng = np.random.default_rng(8)
    A = np.tile(np.eye(n), (3, 1, 1))
    base = 1.0 + rng.random((3, n)); base[1] = 0.0
    b = base.copy(); b[2] = 0.25 * rng.standard_normal(n)
    zero = np.zeros(3, dtype=np.int32)
    c = _Call(hip, A, b, mode, base, np.ones(3, dtype=np.int32), zero, zero, tol, max_it)
    o = c.out
    assert np.array_equal(o["dq"], -b) and (o["q"][:2] == 0.0).all() and np.array_equal(o["q"][2], base[2] - b[2])
    _, err, more, fl_ref, k_ref = _rules(mode, -b, base, zero, tol, max_it)
    if mode == 1:
        assert np.isposinf(err[0]) and np.isnan(err[1])
        assert o["act"].tolist() == [1, 0, 1] and o["fl"].tolist() == [lib.BG_FLAG_NONFINITE, lib.BG_FLAG_NONFINITE, 0]
    else:
        assert np.isfinite(err).all() and err[0] > 1e13 and err[1] == 0.0
        assert o["act"].tolist() == [1, 0, 1] and o["fl"].tolist() == [0, 0, 0]
    assert np.array_equal(o["fl"], fl_ref) and np.array_equal(o["act"], more.astype(np.int32)) and o["k"].tolist() == [1, 1, 1]
    c.check_counter(hip, np.zeros(3, dtype=bool))
    _, actl, kl, fll, _ = _library(mode, A, b, base, np.ones(3, dtype=np.int32), zero, zero, tol, max_it)
    assert np.array_equal(actl, o["act"]) and np.array_equal(kl, o["k"]) and np.array_equal(fll, o["fl"])
    # mode 1 at the last iteration: the inf error no longer goes on, and is capped as well as flagged
    if mode == 1:
        last = np.full(3, max_it - 1, dtype=np.int32)
        o = _Call(hip, A, b, mode, base, np.ones(3, dtype=np.int32), last, zero, tol, max_it).out
        assert o["act"].tolist() == [0, 0, 0] and o["fl"][0] == lib.BG_FLAG_NONFINITE | lib.BG_FLAG_HIT_CAP


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("n", [12, 40])
def test_singular_systems_inside_an_update(hip, n, mode):
    """Singular systems (zero pivot at step k) among healthy ones, B = 21: info == k + 1, counter row 1 counts exactly
    the singular ACTIVE systems in their own slots, a singular system with active == 0 is neither counted nor touched,
    and the healthy systems beside them are solved and updated as if alone."""
    rng = np.random.default_rng(10 * n + mode)
    B, tol, max_it = 21, 0.5, 20
    A = rng.standard_normal((B, n, n)) + 6.0 * np.eye(n)
    sing = {1: 0, 6: n // 2, 11: n - 1, 17: 3, 18: n // 2, 20: 0}             # sample: step of its first zero pivot
    for s, k in sing.items():
        A[s] = _scaled_permutation(rng, n, k)
    active = np.ones(B, dtype=np.int32); active[[3, 11, 18]] = 0              # two of the singular ones are inactive
    b, base = rng.standard_normal((B, n)), rng.standard_normal((B, n))
    iters = np.full(B, 2, dtype=np.int32)
    c = _Call(hip, A, b, mode, base, active, iters, np.zeros(B, dtype=np.int32), tol, max_it)
    o = c.out
    singular = np.zeros(B, dtype=bool); singular[list(sing)] = True
    want_info = np.full(B, I_SENTINEL); want_info[[s for s in sing if active[s]]] = [sing[s] + 1 for s in sing if active[s]]
    assert np.array_equal(o["info"], want_info)
    assert int(o["counter"][1].sum()) == 4
    c.check_counter(hip, singular)
    c.check_inactive_untouched()
    ok = (active == 1) & ~singular
    dq_ref = np.linalg.solve(A[ok], -b[ok][..., None])[..., 0]
    rel = np.linalg.norm(o["dq"][ok] - dq_ref, axis=1) / np.linalg.norm(dq_ref, axis=1)
    assert (rel < _bound(A[ok])).all()
    _, err, more, fl_ref, k_ref = _rules(mode, dq_ref, base[ok], iters[ok], tol, max_it)
    clear = np.abs(err - tol) > 1e-6
    assert np.array_equal(o["act"][ok][clear], more[clear].astype(np.int32))
    assert np.array_equal(o["k"][ok], k_ref) and np.array_equal(o["fl"][ok], fl_ref)
