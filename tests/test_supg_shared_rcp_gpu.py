"""The SUPG element terms with one reciprocal per four elements (csrc/fom_device.hpp, supg_terms).

se[j] = t[j] / mx[j], mx[j] = max(|w_j|, 2e-10).  The kernel used to form each quotient as t * rcp1(mx); every full group of
four now shares one rcp1 through a product tree (r = rcp1(m0 m1 m2 m3), r01 = r (m2 m3), r23 = r (m0 m1), 1/m0 = r01 m1, ...),
and the R % 4 elements left over keep the per-element form.  The first tests restate both forms on the CPU (an exactly
rounded seed plus one Newton step, exact fused multiply-adds through rationals) and bound their difference; the GPU tests
run the assembly of every rows-per-thread class against the oracle, the time loops against the C oracle, and the range limit
of the product (a group past 1.8e308 ends non-finite and flagged, never silently wrong).

Gates: 8 ulp between the two forms on the CPU; the gates of test_fom_gpu.test_assembly_matches_oracle for the assembly;
rel-L2 <= 1e-10 and identical iteration counts against the C oracle for the time loops."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import mesh, rel_l2
from oracle import burgers_ref as br
from oracle import burgers_ref_c as bc

RUN_TOL = 1e-10
ULP = 2.0 ** -52
CLAMP = 2.0e-10
BG_FLAG_NONFINITE = 2                                           # include/burgers_hip.h


# ---- CPU: the two forms of the quotients ---------------------------------------------------------------------------------
def _fma(a, b, c):
    """Elementwise fma with one rounding: exact in rationals, then rounded to nearest even by float(); IEEE rules through
    plain float arithmetic where an operand is not finite (inf * 0 = NaN is all that the range test needs)."""
    def f(x, y, z):
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
            return x * y + z
        return float(Fraction(x) * Fraction(y) + Fraction(z))
    return np.vectorize(f, otypes=[np.float64])(a, b, c)


def _rcp1(d):
    """rcp1 with an exactly rounded seed: one Newton step on top of it (as test_pcr_short_exit_trim_gpu._stride8_last_step)."""
    r = 1.0 / d
    return _fma(r, _fma(-d, r, np.ones_like(d)), r)


def _per_element(mx, t):
    return t * _rcp1(mx)


def _tree(mx, t):
    """Groups of four along the last axis, the kernel's order of operations."""
    m0, m1, m2, m3 = (mx[..., k] for k in range(4))
    p01, p23 = m0 * m1, m2 * m3
    r = _rcp1(p01 * p23)
    r01, r23 = r * p23, r * p01
    return t * np.stack([r01 * m1, r01 * m0, r23 * m3, r23 * m2], axis=-1)


@functools.lru_cache(maxsize=None)
def _groups():
    """(name, mx (G, 4), t (G, 4)): mx uniform and log-uniform over [2e-10, 20], the clamp value mixed with O(1) values in
    every pattern of a group, and groups at 1e76 (the product, 1e304, is still finite)."""
    rng = np.random.default_rng(3118)
    t = lambda g: rng.standard_normal((g, 4)) * 10.0 ** rng.integers(-3, 3, (g, 4))
    out = [("uniform", rng.uniform(CLAMP, 20.0, (160, 4)), t(160)),
           ("log-uniform", np.exp(rng.uniform(np.log(CLAMP), np.log(20.0), (160, 4))), t(160))]
    mixed = rng.uniform(0.5, 10.0, (15 * 4, 4))
    for g in range(mixed.shape[0]):
        for k in range(4):
            if ((g % 15) + 1) >> k & 1:                        # every non-empty subset of the four slots
                mixed[g, k] = CLAMP
    out.append(("clamp mixed with O(1)", mixed, t(mixed.shape[0])))
    big = 1e76 * rng.uniform(0.5, 1.0, (24, 4)); big[0] = 1e76
    out.append(("1e76", big, t(24)))
    return out


def test_the_tree_matches_the_per_element_quotients_to_8_ulp():
    for name, mx, t in _groups():
        assert mx.min() >= CLAMP
        a, b = _tree(mx, t), _per_element(mx, t)
        assert np.isfinite(a).all() and np.isfinite(b).all(), name
        d = float((np.abs(a - b) / np.abs(b)).max())
        print(f"{name}: max relative difference {d / ULP:.2f} ulp")
        assert d <= 8 * ULP, f"{name}: {d / ULP:.2f} ulp"


def test_a_group_past_the_range_is_non_finite_in_all_four_slots():
    mx = np.full((1, 4), 1e80); t = np.array([[1.0, -2.0, 0.5, 3.0]])
    with np.errstate(all="ignore"):
        se = _tree(mx, t)
        assert np.isfinite(_per_element(mx, t)).all()          # not vacuous: the per-element form is fine there
    assert not np.isfinite(se).any(), se


# ---- GPU: one assembly against the oracle ---------------------------------------------------------------------------------
def _graded(N, rng):
    w = rng.uniform(0.7, 1.3, N - 1)
    return np.concatenate([[0.0], np.cumsum(w)]) * (100.0 / w.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("N,graded", [(256, False), (320, False), (192, False), (65, False), (2049, False), (300, True)])
def test_assembly_against_the_oracle(hip, N, graded):
    """Rows per thread R = 4 (one group), 5 (a group and a remainder), 3 (remainder only), 2 with padded rows (w = 0 there, so
    clamp values sit inside the lane), 12 in the workgroup form, 5 on the general path; sample 1 carries +-1e-13 pairs
    (the clamp branch).  The gates of test_fom_gpu.test_assembly_matches_oracle."""
    from burgers_hip import fom
    rng = np.random.default_rng(9100 + N)
    X = _graded(N, rng) if graded else mesh(N)[0]
    B = 3
    uk = 1.0 + 4.0 * rng.random((B, N)); un = 1.0 + 4.0 * rng.random((B, N))
    uk[1, ::5] = 1e-13; uk[1, 1::5] = -1e-13
    mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
    dt, E = 0.03, 0.02
    lo, di, up, rhs = [t.cpu().numpy() for t in fom.fom_assemble(X, uk, un, mu1, mu2, dt, E=E)]
    M3, K3 = br.mass_tridiag(X), br.diffusion_tridiag(X)
    for b in range(B):
        l, d, u = br.system_tridiag(M3, K3, br.convection_tridiag(X, uk[b]), dt, E)
        bb = br.tridiag_matvec(*M3, un[b]) + dt * br.forcing_vector(X, mu2[b]) - dt * br.supg_term(X, uk[b], mu2[b])
        bb[0] = mu1[b]
        r = bb - br.tridiag_matvec(l, d, u, uk[b])
        scale = np.abs(d).max()
        errs = [np.abs(lo[b] - l).max() / scale, np.abs(di[b] - d).max() / scale, np.abs(up[b] - u).max() / scale,
                np.abs(rhs[b] - r).max() / max(1.0, np.abs(r).max())]
        print(f"N={N} graded={graded} sample {b}: lo {errs[0]:.2e} di {errs[1]:.2e} up {errs[2]:.2e} rhs {errs[3]:.2e}")
        assert errs[0] < 1e-13 and errs[1] < 1e-13 and errs[2] < 1e-13
        assert errs[3] < 1e-12


# ---- GPU: time loops against the C oracle ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _run_case(N):
    rng = np.random.default_rng(9200 + N)
    B, nsteps, dt = 4, 8, 0.025
    X, _ = mesh(N)
    mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
    ho, ito = bc.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps)
    return X, mu1, mu2, dt, nsteps, ho, ito


@pytest.mark.gpu
@pytest.mark.parametrize("N,form", [(256, None), (320, None), (1024, None), (320, "wide")])
def test_fom_run_against_the_oracle(hip, N, form):
    from burgers_hip import fom
    X, mu1, mu2, dt, nsteps, ho, ito = _run_case(N)
    res = fom.fom_run(X, np.ones(N), mu1, mu2, dt, nsteps, form=form)
    torch.cuda.synchronize()
    e = rel_l2(res.hist.cpu().numpy(), ho)
    print(f"fom_run N={N} form={form}: rel-L2 {e:.2e}, iterations {int(ito.sum())}")
    assert e <= RUN_TOL
    assert np.array_equal(res.iters.cpu().numpy(), ito)
    assert not (res.flags.cpu().numpy() & BG_FLAG_NONFINITE).any()


# ---- GPU: the range of the shared reciprocal ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_state_past_the_range_is_flagged_not_silently_wrong(hip):
    """u0 = 1e80 in sample 1, past the documented range (every mx <= 1e77): the sample must end with BG_FLAG_NONFINITE and
    its neighbour in the same workgroup must be untouched.  Sample 1's counts are not compared with the oracle's.

    What this pins is the contract, not the tree: N = 128 is two rows per lane, which has no group of four, and a state
    of 1e80 also overflows elsewhere in the iteration.  Measured on one MI355X, parent library and this one alike:
    flags [0, 2], iterations [[6, 5], [2, 1]] (oracle [[6, 5], [5, 1]], its sample 1 non-finite too); at N = 256 (one
    group per lane) both give [[7, 6], [1, 1]].  That a group past the range is non-finite in all four slots while the
    per-element form is not is what test_a_group_past_the_range_is_non_finite_in_all_four_slots shows."""
    from burgers_hip import fom
    N, B, nsteps, dt = 128, 2, 2, 0.025
    X, _ = mesh(N)
    u0 = np.ones((B, N)); u0[1] = 1e80
    mu1 = np.array([4.7, 5.1]); mu2 = np.array([0.02, 0.025])
    res = fom.fom_run(X, u0, mu1, mu2, dt, nsteps)
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        ho, ito = bc.fom_run(X, u0, mu1, mu2, dt, nsteps)
    flags, iters = res.flags.cpu().numpy(), res.iters.cpu().numpy()
    hist = res.hist.cpu().numpy()
    print("flags", flags.tolist(), "iters", iters.tolist(), "oracle iters", ito.tolist(),
          "sample 1 finite:", bool(np.isfinite(hist[1]).all()))
    e = rel_l2(hist[0], ho[0])
    print(f"sample 0: rel-L2 {e:.2e}")
    assert e <= RUN_TOL and np.array_equal(iters[0], ito[0]) and not flags[0] & BG_FLAG_NONFINITE
    assert flags[1] & BG_FLAG_NONFINITE
