"""The FOM Picard loop (csrc/fom.hip, fom_sample) and its assembly away from the one operating point every other FOM test
sits on (tol = 1e-6, max_it = 20 or 1, SUPG on, u > 0): the stopping controls tol and max_it over every instantiation family
of the loop, the ends of tol, the traced run at max_it != 20, SUPG off, and states of either sign.

Gates, the project's own.  A time loop against oracle.burgers_ref_c.fom_run called with the same tol, max_it, supg and E:
iteration counts identical, rel-L2 of the whole history and of every sample <= 1e-10, flags BG_FLAG_HIT_CAP exactly on the
samples with a step at the cap and 0 elsewhere; where both forms exist (64 < N <= 1536, uniform mesh) form="wide" and
form="wave" as in test_fom_gpu._run: equal counts and flags, histories within 1e-12 max(1, max|u|).  A single assembly
against a long-double restatement of the oracle's formulas, row by row (section 5a below).

0. Conditions on the reference (test_reference_conditions and test_assembly_reference_conditions, CPU, unmarked), asserted for
   every time-loop case of the table CASES on the C oracle alone:
     1. the oracle's history is finite;
     2. the counts at tol * 1.001 and tol / 1.001 are those at tol (finite positive tol): no stopping decision on the edge;
     3. a 1e-13 relative Gaussian perturbation of u0 moves the oracle's history by at most 100 x 1e-13 rel-L2 and changes no
        count.  The kernel differs from the oracle by about 1e-14 per solve, so this leaves two decades under the gate.
        Sign-changing time loops (u0 = 0.3 + 1.2 sin(3 pi x / 100), mu1 x 0.1) amplify such a perturbation by 9e10 to 1e13
        at N = 128 ... 8192 and change counts: they can be compared with nothing, and states of mixed sign are pinned by
        single assemblies (5a), by the one well-conditioned run of 5c and by three runs without SUPG, which amplify by
        less than 1;
     4. the structure the case exists for (``needs``), read from the per-iteration errors of oracle.burgers_ref.fom_burgers:
          two    a step of two iterations, the first lean and the second for the increment: tol < err_1 <= 16 tol
          lean   the cap falls inside the lean loop: err_{max_it - 1} > 16 tol in a step that runs to the cap
          incr   the cap falls inside the increment loop: err_{max_it - 1} <= 16 tol and err_{max_it} > tol
          long   an uncapped step of more than 20 iterations (max_it = 40)
          cap / nocap / count7 / count0   every step at the cap / below it / of 7 / of 0 iterations
          below  (tol < 0) at |tol| every step ends below the cap
          negative   every element sum u_e + u_{e+1} of the whole history is negative
        each with a margin of 1.001 on its comparisons.
   Moved to meet condition 2 (MOVED, INCR_CAP): dt of (1e-4, 20) at N = 300 graded, 1024 and 1537 graded and of (1e-9, 40) at
   N = 6145; to meet ``negative``: dt of four reversed-flow cases (SECTION5C).  Extremes: see MEASURED below.

1. tol x max_it, CONTROLS, over the families of fom_sample: the wave kernels full (N = 64, one row per lane; 128; 1024) and
   masked (65, 1000), graded with the lean loop (300) and without (1300, 24 rows per lane), the workgroup kernels uniform
   (2049), parked without the lean loop (6145), graded with (1537) and without (4097) the lean loop, and the opt-in workgroup
   form at N = 128 and 1024 through form="wide".  u0 = ones, B = 5, six steps, dt = min(0.2, 0.05 * 512 / N).
2. The ends of tol at N = 128 and 2049, max_it = 7: tol = 0 and tol = -1e-6 run every step to the cap, as the oracle does
   (fom_args squares tol for the kernels' test nd > tol^2 nu; the square of a negative tol stopped where |tol| stops:
   counts [5 4 4 4] for the oracle's [7 7 7 7] at N = 2049).  dt is a tenth of section 1's, so that |tol| stops below the
   cap.  tol = inf and tol = NaN: no comparison holds; the oracle's while loop then runs no iteration at all, the kernel's
   first iteration always runs, so every count is 1, no flag, and the history is gated against the oracle's at max_it = 1,
   which is the same one solve per step.
3. bg_fom_run_traced with max_it = 7, 40, 20: history, counts and flags bitwise those of the untraced run, errs of shape
   (B, nsteps, max_it), NaN exactly where the reference ran no iteration, values within rtol 1e-6.
4. SUPG off: one assembly (reference: the oracle's pieces without the supg_term line, gates of
   test_fom_gpu.py::test_assembly_matches_oracle, and the switch moves the right-hand side by more than 1e-3 max|b|) and the
   time loop against the C oracle with supg=False.
5. States of either sign.  5a: one assembly of six states (positive, negative, sign-changing, and three of mixed sign whose
   element sums at a thread's first and last row, inside a group of four of supg_terms and in its ragged last group are set
   exactly to 0, +-1e-10, +-2e-10, +-3e-10, +-1e-3 on the grid 2^-50, and in the last state to the doubles 1e-10, 2e-10, 3e-10
   themselves), un of mixed sign too.  Diagonals within 1e-13 max|di|; right-hand side row by row,
   |rhs_i - ref_i| <= 1e-13 T_i, T_i the sum of the absolute values of the terms of row i in the long-double reference
   (|g_i|, dt |S| of both elements, |lo u|, |di u|, |up u|): 40 times the 2.6e-15 the header of supg_terms derives for one
   quotient, where a wrong sign is of order T_i.  The float64 oracle itself meets 1e-14 T_i (section 0).
   5c: reversed flow, u0 = -ones and mu1 = -MU1, through the time loop (the interface couplings mirrored, so that the
   ballots of pcr64 go the other way), the one sign-changing run that is well conditioned (N = 65, E = 0.2), and
   sign-changing runs with SUPG off at N = 128, 1024 and 2049.

MEASURED (the C oracle on the CPU, and one MI355X):
  section 0: most iterations 40 (the cap of (1e-9, 40), N = 128); largest amplification of condition 3: 3.2
  (s5c_n1024_reversed_E0), 1.1 among the other reversed-flow cases, 0.91 for the sign-changing run, below 1 everywhere
  else.  The float64 oracle against the long-double assembly: at most 1.0e-15 T_i (n2049).
  worst rel-L2 against the oracle, whole history / worst sample: section 1: 1.3e-14 / 1.3e-14 (n64, (1e-6, 3));
  section 2: 6.9e-15 / 7.0e-15 (n128, tol = inf); section 3: 5.8e-15 / 5.9e-15 (traced errors within 3.1e-7 relative, at
  errors of 8e-10, n128 (1e-9, 40); 1.2e-8 on the graded mesh); section 4: 5.6e-16 / 5.9e-16; section 5c: 2.3e-15 / 4.2e-15.
  5a, worst |rhs_i - ref_i| / T_i per family: see ASSEMBLY_SHAPES (at most 1.2e-14, gate 1e-13).
  No case missed its gate.  On the library before fom_args cased the sign of tol the two tol = -1e-6 cases alone fail, with
  counts [5 5 4 4] ... [5 5 5 5] (N = 128) and [5 4 4 4] (N = 2049) for the oracle's [7 7 7 7]."""
import functools
from dataclasses import dataclass

import numpy as np
import pytest

from conftest import mesh, rel_l2
from oracle import burgers_ref as br
from oracle import burgers_ref_c as bc

TOL = 1e-10
MU1 = np.array([4.3, 4.7, 5.0, 5.3, 5.5])          # the values of test_picard_rotate_gpu.py
MU2 = np.array([0.016, 0.02, 0.024, 0.027, 0.03])
LEAN = 16.0                                        # BG_PICARD_LEAN_FACTOR
EDGE = 1.001
LD = np.longdouble


def _graded(N):
    w = np.random.default_rng(300).uniform(0.7, 1.3, N - 1)
    return np.concatenate([[0.0], np.cumsum(w)]) * (100.0 / w.sum())


# ---- the time-loop cases -----------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    N: int
    graded: bool = False
    E: float = 0.0
    dt: float = 0.0            # 0: min(0.2, 0.05 * 512 / N)
    nsteps: int = 6
    B: int = 5
    tol: float = 1e-6
    max_it: int = 20
    supg: bool = True
    start: str = "ones"        # ones | neg (u0 = -ones, mu1 = -MU1) | sin (u0 = 0.3 + 1.2 sin(3 pi x / 100), mu1 = 0.1 MU1)
    needs: tuple = ()          # the structural conditions of section 0.4
    ref_max_it: int = 0        # tol = inf, NaN: the oracle is run with this cap instead (see the docstring, section 2)

    @property
    def X(self):
        return _graded(self.N) if self.graded else mesh(self.N)[0]

    @property
    def step(self):
        return self.dt or min(0.2, 0.05 * 512 / self.N)

    @property
    def mu(self):
        f = {"ones": 1.0, "neg": -1.0, "sin": 0.1}[self.start]
        return f * MU1[:self.B], MU2[:self.B]

    @property
    def u0(self):
        if self.start == "sin":
            return 0.3 + 1.2 * np.sin(3 * np.pi * self.X / 100)
        return np.ones(self.N) if self.start == "ones" else -np.ones(self.N)


FAMILIES = [("n64", 64, False), ("n128", 128, False), ("n1024", 1024, False), ("n65", 65, False), ("n1000", 1000, False),
            ("n300g", 300, True), ("n1300g", 1300, True), ("n2049", 2049, False), ("n6145", 6145, False),
            ("n1537g", 1537, True), ("n4097g", 4097, True)]
HAS_LEAN = {"n64", "n128", "n1024", "n65", "n1000", "n300g", "n2049", "n1537g"}
CONTROLS = [(1e-2, 20), (1e-4, 20), (1e-9, 40), (1e-6, 3), (1e-6, 7), (1e-9, 12)]
# (family, tol, max_it) -> what the case must show (section 0.4) and what was moved to meet condition 2
NEEDS = {
    ("n64", 1e-2, 20): ("two", "nocap"), ("n1024", 1e-2, 20): ("two", "nocap"), ("n2049", 1e-2, 20): ("two", "nocap"),
    ("n300g", 1e-2, 20): ("two", "nocap"), ("n1537g", 1e-2, 20): ("two", "nocap"),
    ("n128", 1e-4, 20): ("nocap",), ("n1000", 1e-4, 20): ("nocap",),
    ("n128", 1e-9, 40): ("long",), ("n1024", 1e-9, 40): ("long",), ("n2049", 1e-9, 40): ("long", "nocap"),
    ("n1537g", 1e-9, 40): ("long",), ("n6145", 1e-9, 40): ("long", "nocap"),
    ("n128", 1e-6, 3): ("lean", "cap"), ("n1024", 1e-6, 3): ("lean", "cap"), ("n2049", 1e-6, 3): ("lean", "cap"),
    ("n300g", 1e-6, 3): ("lean", "cap"), ("n1537g", 1e-6, 3): ("lean", "cap"),
    ("n128", 1e-6, 7): ("lean", "cap"), ("n1024", 1e-6, 7): ("lean", "incr", "cap"), ("n2049", 1e-6, 7): ("lean", "incr", "cap"),
    ("n128", 1e-9, 12): ("lean", "cap"), ("n1024", 1e-9, 12): ("lean", "cap"), ("n6145", 1e-9, 12): ("cap",),
}
# condition 2 is missed at the table's dt (a count sits within 1.001 of the edge): dt moved, by 4 % at the most
MOVED = {
    ("n300g", 1e-4, 20): dict(dt=0.08),          # table: 0.0853
    ("n1024", 1e-4, 20): dict(dt=0.024),         # 0.025
    ("n1537g", 1e-4, 20): dict(dt=0.016),        # 0.01666
    ("n6145", 1e-9, 40): dict(dt=0.004),         # 0.004166
}


def _section1():
    out = []
    for fam, N, graded in FAMILIES:
        for tol, cap in CONTROLS:
            out.append(Case(f"s1_{fam}_tol{tol:g}_cap{cap}", N, graded, tol=tol, max_it=cap, needs=NEEDS.get((fam, tol, cap), ()),
                            **MOVED.get((fam, tol, cap), {})))
    # (c): the cap inside the increment loop; max_it read from the oracle's errors at tol = 1e-6
    out.append(Case("s1_n128_cap_in_increment", 128, tol=1e-6, max_it=INCR_CAP[128], needs=("incr",)))
    out.append(Case("s1_n1024_cap_in_increment", 1024, tol=1e-6, max_it=INCR_CAP[1024], needs=("incr",)))
    return out


INCR_CAP = {128: 13, 1024: 11}        # at 13, N = 1024 misses condition 2

# dt is a tenth of the table's: at the table's the steps take 7 iterations and more at tol = 1e-6 as well, and a negative tol
# that stopped where its square stops would show nothing.  Here tol = 1e-6 takes 4 to 6 (``below``, asserted in section 0).
SECTION2 = [Case(f"s2_n{N}_tol_{name}", N, dt=dt, nsteps=4, tol=tol, max_it=7, needs=needs, ref_max_it=ref)
            for N, dt in ((128, 0.02), (2049, 0.001))
            for name, tol, needs, ref in (("zero", 0.0, ("count7",), 0), ("negative", -1e-6, ("count7", "below"), 0),
                                          ("inf", float("inf"), ("count0",), 1), ("nan", float("nan"), ("count0",), 1))]
SECTION3 = [Case(f"s3_{fam}_tol{tol:g}_cap{cap}", N, graded, nsteps=5, B=3, tol=tol, max_it=cap)
            for fam, N, graded in (("n128", 128, False), ("n300g", 300, True))
            for tol, cap in ((1e-6, 7), (1e-9, 40), (1e-2, 20))]
SECTION4 = [Case(f"s4_n{N}_E{E:g}_supg_off", N, E=E, nsteps=8, supg=False) for N in (128, 1000, 2049) for E in (0.0, 0.05)] + \
           [Case("s4_n300g_E0.004_supg_off", 300, True, E=0.004, nsteps=8, supg=False)]
# dt of the four marked cases is below the one first measured (0.02, 0.0125, 0.0125, 0.01): there the outflow layer at the
# Dirichlet node overshoots within six steps and the sum of element 1 turns positive
SECTION5C = [
    Case("s5c_n65_reversed", 65, E=0.2, dt=0.05, start="neg", needs=("negative", "nocap")),
    Case("s5c_n128_reversed", 128, E=0.0, dt=0.02, start="neg", needs=("negative", "nocap")),
    Case("s5c_n300g_reversed", 300, True, E=0.05, dt=0.012, start="neg", needs=("negative", "nocap")),      # moved
    Case("s5c_n1000_reversed", 1000, E=0.05, dt=0.006, start="neg", needs=("negative", "nocap")),           # moved
    Case("s5c_n1024_reversed", 1024, E=0.05, dt=0.006, start="neg", needs=("negative", "nocap")),           # moved
    Case("s5c_n1300g_reversed", 1300, True, E=0.05, dt=0.005, start="neg", needs=("negative", "nocap")),    # moved
    Case("s5c_n2049_reversed", 2049, E=0.05, dt=0.0125, start="neg", needs=("negative", "nocap")),
    Case("s5c_n6145_reversed", 6145, E=0.05, dt=0.004, start="neg", needs=("negative", "nocap")),
    # no diffusion: some steps run into the cap and the layer oscillates through 0 (sums of elements 0, 1 and 4 turn positive)
    Case("s5c_n1024_reversed_E0", 1024, E=0.0, dt=0.0125, start="neg"),
    Case("s5c_n65_sign_changing", 65, E=0.2, dt=0.05, start="sin", needs=("nocap",)),
    # without SUPG, whose 1 / |u_e| is what makes such a run ill conditioned, a sign-changing start is as tame as any other
    Case("s5c_n128_sign_changing_supg_off", 128, E=0.05, start="sin", supg=False),
    Case("s5c_n1024_sign_changing_supg_off", 1024, E=0.05, start="sin", supg=False),
    Case("s5c_n2049_sign_changing_supg_off", 2049, E=0.05, start="sin", supg=False),
]
SECTION1 = _section1()
CASES = SECTION1 + SECTION2 + SECTION3 + SECTION4 + SECTION5C
assert len({c.id for c in CASES}) == len(CASES)


def _ids(cases):
    return [c.id for c in cases]


def _oracle_run(c, u0=None, tol=None):
    mu1, mu2 = c.mu
    if c.ref_max_it:                            # one iteration per step whatever the tolerance, which the oracle needs finite
        tol = 1e-6
    return bc.fom_run(c.X, c.u0 if u0 is None else u0, mu1, mu2, c.step, c.nsteps, E=c.E, tol=c.tol if tol is None else tol,
                      max_it=c.ref_max_it or c.max_it, supg=c.supg)


@functools.lru_cache(maxsize=None)
def oracle(c):
    """The C oracle on the case, computed once and read-only."""
    ho, ito = _oracle_run(c)
    ho.setflags(write=False); ito.setflags(write=False)
    return ho, ito


@functools.lru_cache(maxsize=None)
def oracle_errs(c):
    """Per-iteration errors (B, nsteps, max_it) and counts of the NumPy oracle (SUPG on only)."""
    assert c.supg
    mu1, mu2 = c.mu
    errs, its = [], []
    for b in range(c.B):
        _, it, e = br.fom_burgers(c.X, c.step, c.nsteps, c.u0, mu1[b], c.E, mu2[b], tol=c.tol, max_it=c.max_it,
                                  return_iters=True, return_errs=True)
        errs.append(e); its.append(it)
    return np.array(errs), np.array(its)


def structure(c):
    """Which of the structural conditions of section 0.4 hold on the oracle (those that need the errors only when asked)."""
    ho, ito = oracle(c)
    out = {"cap": bool((ito == c.max_it).all()), "nocap": bool((ito < c.max_it).all()),
           "long": bool(((ito > 20) & (ito < c.max_it)).any()), "count7": bool((ito == 7).all()),
           "negative": bool((ho[:, :, :-1] + ho[:, :, 1:] < 0).all())}
    if c.tol < 0:
        out["below"] = bool((_oracle_run(c, tol=-c.tol)[1] < c.max_it).all())
    if c.ref_max_it:
        out["count0"] = bool((bc.fom_run(c.X, c.u0, *c.mu, c.step, c.nsteps, E=c.E, tol=c.tol, max_it=c.max_it)[1] == 0).all())
    if set(c.needs) & {"two", "lean", "incr"}:
        e, it = oracle_errs(c)
        assert np.array_equal(it, ito)
        m = c.max_it
        two = (it == 2) & (e[..., 0] > c.tol * EDGE) & (e[..., 0] < LEAN * c.tol / EDGE)
        capped = it == m
        before = e[..., m - 2] if m >= 2 else np.full(it.shape, np.inf)      # decides the form of iteration m
        out["two"] = bool(two.any())
        out["lean"] = bool((capped & (before > LEAN * c.tol * EDGE)).any())
        out["incr"] = bool((capped & (before < LEAN * c.tol / EDGE) & (e[..., m - 1] > c.tol * EDGE)).any())
    return out


def amplification(c):
    """Condition 3: rel-L2 move of the oracle's history under a 1e-13 relative perturbation of u0, over 1e-13."""
    ho, ito = oracle(c)
    u0 = np.broadcast_to(c.u0, (c.B, c.N)) * (1.0 + 1e-13 * np.random.default_rng(13).standard_normal((c.B, c.N)))
    hp, itp = _oracle_run(c, u0=u0)
    return rel_l2(hp, ho) / 1e-13, np.array_equal(itp, ito)


@pytest.mark.parametrize("c", CASES, ids=_ids(CASES))
def test_reference_conditions(c):
    ho, ito = oracle(c)
    assert np.isfinite(ho).all()                                                          # 1
    if np.isfinite(c.tol) and c.tol > 0:                                                  # 2
        for f in (EDGE, 1.0 / EDGE):
            assert np.array_equal(_oracle_run(c, tol=c.tol * f)[1], ito), f"a stopping decision within {EDGE} of tol"
    amp, same = amplification(c)                                                          # 3
    print(f"{c.id}: iterations {ito.min()}..{ito.max()}, amplification {amp:.2g}")
    assert same and amp <= 100.0
    s = structure(c)                                                                      # 4
    for need in c.needs:
        assert s[need], (need, s)
    if c.needs and set(c.needs) & {"two", "lean", "incr"}:
        assert any(c.id.startswith(f"s1_{fam}_") for fam in HAS_LEAN)


def test_every_structure_is_met_somewhere():
    met = {n for c in CASES for n in c.needs}
    assert {"two", "lean", "incr", "long", "cap", "nocap", "count7", "count0", "below", "negative"} <= met


# ---- the time loop on the GPU ------------------------------------------------------------------------------------------------
def _gpu_loop(hip, c, forms=True):
    import torch
    from burgers_hip import fom
    ho, ito = oracle(c)
    mu1, mu2 = c.mu
    kw = dict(E=c.E, tol=c.tol, max_it=c.max_it, supg=c.supg)
    res = fom.fom_run(c.X, c.u0, mu1, mu2, c.step, c.nsteps, **kw)
    torch.cuda.synchronize()
    h, it, fl = res.hist.cpu().numpy(), res.iters.cpu().numpy(), res.flags.cpu().numpy()
    e = rel_l2(h, ho)
    worst = max(rel_l2(h[b], ho[b]) for b in range(c.B))
    print(f"{c.id}: rel-L2 {e:.2e}, worst sample {worst:.2e}, iterations {it.min()}..{it.max()}, oracle {ito.min()}..{ito.max()}")
    assert np.array_equal(it, ito), (it, ito)
    assert np.array_equal(fl, np.where((it >= c.max_it).any(axis=1), hip.BG_FLAG_HIT_CAP, 0))
    assert e <= TOL and worst <= TOL
    if forms and 64 < c.N <= 1536 and not c.graded:
        for form in ("wide", "wave"):
            r2 = fom.fom_run(c.X, c.u0, mu1, mu2, c.step, c.nsteps, form=form, **kw)
            torch.cuda.synchronize()
            assert np.array_equal(r2.iters.cpu().numpy(), it) and np.array_equal(r2.flags.cpu().numpy(), fl), form
            assert np.abs(r2.hist.cpu().numpy() - h).max() <= 1e-12 * max(1.0, np.abs(h).max()), form
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("c", SECTION1, ids=_ids(SECTION1))
def test_tol_and_cap_over_the_families(hip, c):
    _gpu_loop(hip, c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", SECTION2, ids=_ids(SECTION2))
def test_the_ends_of_tol(hip, c):
    ito = oracle(c)[1]
    assert (ito == (1 if c.ref_max_it else 7)).all()
    res = _gpu_loop(hip, c)
    assert (res.iters.cpu().numpy() == (1 if c.ref_max_it else 7)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("c", SECTION3, ids=_ids(SECTION3))
def test_traced_run_off_the_default_cap(hip, c):
    import torch
    from burgers_hip import fom
    a = _gpu_loop(hip, c, forms=False)
    mu1, mu2 = c.mu
    t = fom.fom_run(c.X, c.u0, mu1, mu2, c.step, c.nsteps, E=c.E, tol=c.tol, max_it=c.max_it, trace=True)
    torch.cuda.synchronize()
    assert torch.equal(a.hist, t.hist) and torch.equal(a.iters, t.iters) and torch.equal(a.flags, t.flags)
    errs = t.errs.cpu().numpy()
    eo, it = oracle_errs(c)
    assert errs.shape == (c.B, c.nsteps, c.max_it) == eo.shape
    assert np.array_equal(it, oracle(c)[1])
    ran = ~np.isnan(eo)
    assert np.array_equal(ran, np.arange(c.max_it)[None, None, :] < it[..., None])
    assert np.array_equal(np.isnan(errs), ~ran)                       # entries k >= iters keep the prefill
    print(f"{c.id}: worst relative deviation of a traced error {np.abs(errs[ran] / eo[ran] - 1.0).max():.2e}, "
          f"smallest error {eo[ran].min():.2e}")
    assert np.allclose(errs[ran], eo[ran], rtol=1e-6, atol=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("c", SECTION4, ids=_ids(SECTION4))
def test_time_loop_without_supg(hip, c):
    _gpu_loop(hip, c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", SECTION5C, ids=_ids(SECTION5C))
def test_reversed_flow(hip, c):
    _gpu_loop(hip, c)


# ---- single assemblies -------------------------------------------------------------------------------------------------------
# (id, N, graded, rows per thread of the assembly kernel).  Worst |rhs_i - ref_i| / T_i measured on one MI355X (gate 1e-13),
# in brackets the worst of the rows next to an element under the clamp, then the diagonals over max|di| (gate 1e-13):
#   n96 1.2e-14 (7.0e-15) 3.8e-15, n128 1.1e-14 (1.1e-14) 3.9e-15, n300g 1.8e-15 (1.8e-15) 7.2e-17,
#   n2049 2.0e-15 (1.5e-15) 2.2e-17, n1537g 2.2e-15 (2.2e-15) 2.0e-17.
# The uniform kernels take one h = (x_last - x_0) / (N - 1) where the reference differences the nodes of np.linspace, rounded
# at 1.4e-14 near x = 100: the long-double reference on the ideal nodes x_0 + i h differs from itself on the rounded ones by
# 1.2e-14 (n96) and 1.1e-14 (n128) of T_i, 3.7e-15 on the diagonals, which is all of those two figures; on 2049 nodes
# h = 100 / 2048 and every node is exact.  No row needed a wider gate.
ASSEMBLY_SHAPES = [("n96", 96, False, 2), ("n128", 128, False, 2), ("n300g", 300, True, 5), ("n2049", 2049, False, 12),
                   ("n1537g", 1537, True, 8)]
DT_A, E_A = 0.03, 0.02
SUMS = [0.0, 1e-10, -1e-10, 2e-10, -2e-10, 3e-10, -3e-10, 1e-3, -1e-3]
GRID = 2.0 ** -50
# |u| at the nodes of a chosen element.  The float64 oracle forms u at a Gauss point as a u_l + b u_r, which rounds at
# eps |u| where u_l + u_r is a sum of 1e-10: its SUPG term is then off by eps |u| |du/dx| tau, 6e-13 of the row's terms at
# |u| = 2 on 2049 nodes (measured), where the kernel and the long-double reference hold the sum exactly.  At 2^-4 that loss
# stays under the 1e-14 T_i asked of the oracle in section 0.
ANCHOR = 2.0 ** -4


def _local_rows(R):
    """Local elements of a thread whose sums are set: its first and last row, inside a group of four of supg_terms, the last
    of a full group and the first of the ragged last group.  R = 5: 0, 2, 3, 4."""
    G = R // 4 * 4
    rows = {0, R - 1}
    if R >= 4:
        rows |= {2, G - 1}
    if R % 4:
        rows.add(G)
    return sorted(rows)


def _set_sums(u, R, shift, exact_doubles):
    """Set w_e = u_e + u_{e+1} of the chosen elements e, left to right: u_{e+1} = w - u_e.  Every number is a multiple of
    2^-50 below 8, so the difference and the sum are exact (asserted); thread p gives its k-th chosen element the sum
    SUMS[shift + p + 2 k], so every local position meets every sum.  With ``exact_doubles`` the small sums of one local
    element (the third, or the first where a thread has fewer than four) are the doubles 1e-10, 2e-10, 3e-10 and their
    negatives themselves: u_e is then the power of two next to |w| and u_{e+1} = w - u_e is exact by Sterbenz' lemma; the
    elements next to such a one are left as they are.  Returns the elements and their sums."""
    N = len(u)
    u[:] = np.round(u / GRID) * GRID
    jx = 2 if R >= 4 else 0
    plan = []
    for p in range(0, (N + R - 1) // R):
        for k, j in enumerate(_local_rows(R)):
            e = p * R + j
            if e + 1 < N:
                w = SUMS[(shift + p + 2 * k) % len(SUMS)]
                plan.append((e, w, exact_doubles and j == jx and 0.0 < abs(w) < 1e-9))
    exact = {e for e, _, x in plan if x}
    chosen = []
    for e, w, x in plan:
        if x:
            u[e] = np.sign(w) * 2.0 ** np.ceil(np.log2(abs(w)))
        elif e - 1 in exact or e + 1 in exact:
            continue
        else:
            w = np.round(w / GRID) * GRID
            if not chosen or chosen[-1][0] != e - 1:                  # not the right node of the element set before
                u[e] = ANCHOR * (-1.0) ** (e // R)
        u[e + 1] = w - u[e]
        chosen.append((e, w))
    for e, w in chosen:
        assert u[e] + u[e + 1] == w and LD(u[e]) + LD(u[e + 1]) == LD(w), (e, w)
    return chosen


@functools.lru_cache(maxsize=None)
def assembly_inputs(name):
    _, N, graded, R = next(s for s in ASSEMBLY_SHAPES if s[0] == name)
    rng = np.random.default_rng(5000 + N)
    X = _graded(N) if graded else mesh(N)[0]
    B = 6
    uk = np.empty((B, N))
    uk[0] = 1.0 + 4.0 * rng.random(N)
    uk[1] = -(1.0 + 4.0 * rng.random(N))
    uk[2] = 3.0 * np.sin(7 * np.pi * X / 100) + 0.2 * rng.standard_normal(N)
    chosen = []
    for s in (3, 4, 5):
        uk[s] = 2.0 * np.sin((3 + s) * np.pi * X / 100) + 0.5 * rng.standard_normal(N)
        chosen.append(_set_sums(uk[s], R, 4 * (s - 3), exact_doubles=(s == 5)))
    un = 2.5 * np.cos(5 * np.pi * X / 100)[None, :] + 0.5 * rng.standard_normal((B, N))
    mu1 = rng.uniform(4.25, 5.5, B) * np.array([1, -1, 1, -1, 1, -1.0])
    mu2 = rng.uniform(0.015, 0.03, B)
    for a in (X, uk, un, mu1, mu2):
        a.setflags(write=False)
    return X, uk, un, mu1, mu2, chosen


def assembly_ld(X, uk, un, mu1, mu2, dt, E, supg=True):
    """The oracle's mass / diffusion / convection / system_tridiag, forcing_vector, supg_term and tridiag_matvec restated on
    long doubles from the float64 operands, for one state.  Returns lo, di, up, rhs = b - A uk and T, the sum of the
    absolute values of the terms of every row of rhs."""
    X, uk, un = (np.asarray(a, dtype=LD) for a in (X, uk, un))
    mu1, mu2, dt, E = LD(mu1), LD(mu2), LD(dt), LD(E)
    n = len(X)
    s3 = np.sqrt(LD(3)) / 3
    Ng = np.array([[(1 + s3) / 2, (1 - s3) / 2], [(1 - s3) / 2, (1 + s3) / 2]], dtype=LD)     # N[gp, node]
    Nxi = np.array([-0.5, 0.5], dtype=LD)
    xl, xr = X[:-1], X[1:]
    h = xr - xl
    J = -0.5 * xl + 0.5 * xr
    dV = np.abs(J)
    ul, ur = uk[:-1], uk[1:]

    def scatter(Ell, Elr, Erl, Err):
        lo, di, up = (np.zeros(n, dtype=LD) for _ in range(3))
        di[1:] += Err; di[:-1] += Ell; up[:-1] = Elr; lo[1:] = Erl
        return lo, di, up

    def elem(f):
        return scatter(*[sum(f(gp, i, j) for gp in range(2)) for i in range(2) for j in range(2)])

    M3 = elem(lambda gp, i, j: Ng[gp, i] * Ng[gp, j] * dV)
    K3 = elem(lambda gp, i, j: (Nxi[i] / J) * (Nxi[j] / J) * dV)
    C3 = elem(lambda gp, i, j: Ng[gp, i] * ((Ng[gp, 0] * ul + Ng[gp, 1] * ur) * (Nxi[j] / J)) * dV)
    lo, di, up = ((m + dt * c) + (dt * E) * k for m, c, k in zip(M3, C3, K3))
    lo[0], di[0], up[0] = 0, 1, 0

    def matvec(l, d, p, x):
        return np.concatenate([[LD(0)], l[1:] * x[:-1]]), d * x, np.concatenate([p[:-1] * x[1:], [LD(0)]])

    f_gp = [LD(0.02) * np.exp(mu2 * (Ng[gp, 0] * xl + Ng[gp, 1] * xr)) for gp in range(2)]
    F = np.zeros(n, dtype=LD)
    F[1:] += sum(f_gp[gp] * Ng[gp, 1] * dV for gp in range(2))
    F[:-1] += sum(f_gp[gp] * Ng[gp, 0] * dV for gp in range(2))
    g = sum(matvec(*M3, un)) + dt * F
    Sl, Sr = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)              # the two element contributions to S of a row
    if supg:
        u_e = (ul + ur) / 2
        vel = np.where(np.abs(u_e) > LD(1.0e-10), np.abs(u_e), LD(1.0e-10))
        tau = 0.5 * h / (2 * vel)
        du_dx = (ur - ul) / h
        R_gp = [(Ng[gp, 0] * ul + Ng[gp, 1] * ur) * du_dx - f_gp[gp] for gp in range(2)]
        Sr[1:] = sum(tau * R_gp[gp] * (Nxi[1] / J) * dV for gp in range(2))
        Sl[:-1] = sum(tau * R_gp[gp] * (Nxi[0] / J) * dV for gp in range(2))
    b = g - dt * (Sr + Sl)
    a_lo, a_di, a_up = matvec(lo, di, up, uk)
    rhs = b - (a_lo + a_di + a_up)
    T = np.abs(g) + dt * (np.abs(Sr) + np.abs(Sl)) + np.abs(a_lo) + np.abs(a_di) + np.abs(a_up)
    rhs[0] = mu1 - uk[0]
    T[0] = abs(mu1) + abs(uk[0])
    return lo, di, up, rhs, T


@functools.lru_cache(maxsize=None)
def assembly_reference(name):
    X, uk, un, mu1, mu2, _ = assembly_inputs(name)
    return [assembly_ld(X, uk[b], un[b], mu1[b], mu2[b], DT_A, E_A) for b in range(len(uk))]


def oracle_assembly(X, uk, un, mu1, mu2, dt, E, supg=True):
    """The float64 oracle's assembly of one state: lo, di, up, b - A uk, b."""
    M3, K3 = br.mass_tridiag(X), br.diffusion_tridiag(X)
    l, d, u = br.system_tridiag(M3, K3, br.convection_tridiag(X, uk), dt, E)
    bb = br.tridiag_matvec(*M3, un) + dt * br.forcing_vector(X, mu2)
    if supg:
        bb = bb - dt * br.supg_term(X, uk, mu2)
    bb[0] = mu1
    return l, d, u, bb - br.tridiag_matvec(l, d, u, uk), bb


def _ratios(got, ref):
    """Worst deviation of the three diagonals over max|di|, and of the right-hand side over T, row by row."""
    lo, di, up, rhs, T = ref
    scale = np.abs(di).max()
    dd = max(float(np.abs(LD(a) - r).max() / scale) for a, r in zip(got[:3], (lo, di, up)))
    return dd, (np.abs(LD(got[3]) - rhs) / T).astype(np.float64)


@pytest.mark.parametrize("name", [s[0] for s in ASSEMBLY_SHAPES])
def test_assembly_reference_conditions(name):
    """Section 0 for 5a: the chosen sums are where they should be and of either side of the clamp, every state but the first
    two has element sums of both signs, and the float64 oracle meets the gate with a factor of 10 to spare."""
    X, uk, un, mu1, mu2, chosen = assembly_inputs(name)
    R = next(s[3] for s in ASSEMBLY_SHAPES if s[0] == name)
    w = uk[:, :-1] + uk[:, 1:]
    assert (w[0] > 0).all() and (w[1] < 0).all()
    assert all((w[s] > 0).any() and (w[s] < 0).any() for s in range(2, 6)) and (un > 0).any() and (un < 0).any()
    for ch in chosen[:2]:
        assert {e % R for e, _ in ch} == set(_local_rows(R))
        for j in _local_rows(R):                                      # every local position sees both sides of the clamp and a 0
            ws = [abs(wv) for e, wv in ch if e % R == j]
            assert min(ws) == 0.0 and any(0 < v < 2e-10 for v in ws) and any(2e-10 < v < 1e-9 for v in ws) and max(ws) > 5e-4
    assert {wv for _, wv in chosen[2]} >= {1e-10, -1e-10, 2e-10, -2e-10, 3e-10, -3e-10}
    worst = 0.0
    for b, ref in enumerate(assembly_reference(name)):
        dd, rr = _ratios(oracle_assembly(X, uk[b], un[b], mu1[b], mu2[b], DT_A, E_A), ref)
        worst = max(worst, rr.max())
        assert dd <= 1e-14 and rr.max() <= 1e-14, (b, dd, rr.max(), int(rr.argmax()))
    print(f"{name}: the float64 oracle is within {worst:.2e} T_i of the long-double reference")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [s[0] for s in ASSEMBLY_SHAPES])
def test_assembly_of_states_of_either_sign(hip, name):
    from burgers_hip import fom
    X, uk, un, mu1, mu2, chosen = assembly_inputs(name)
    got = [t.cpu().numpy() for t in fom.fom_assemble(*(a.copy() for a in (X, uk, un, mu1, mu2)), DT_A, E=E_A)]   # the inputs are read-only
    worst_d = worst_r = worst_clamp = 0.0
    for b, ref in enumerate(assembly_reference(name)):
        dd, rr = _ratios([a[b] for a in got], ref)
        w = np.abs(uk[b, :-1] + uk[b, 1:])
        sub = np.zeros(len(X), dtype=bool)
        sub[:-1] |= w < 2e-10; sub[1:] |= w < 2e-10                   # rows next to an element under the clamp
        worst_d, worst_r = max(worst_d, dd), max(worst_r, rr.max())
        worst_clamp = max(worst_clamp, rr[sub].max() if sub.any() else 0.0)
        assert dd <= 1e-13, (b, dd)
        assert rr.max() <= 1e-13, (b, int(rr.argmax()), rr.max())
    print(f"{name}: worst row ratio |rhs - ref| / T {worst_r:.2e} (rows at the clamp {worst_clamp:.2e}), diagonals {worst_d:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [s[0] for s in ASSEMBLY_SHAPES])
def test_assembly_without_supg(hip, name):
    """fom_assemble(..., supg=False) on the states of test_fom_gpu.py::test_assembly_matches_oracle, at that test's gates,
    against the oracle's pieces without the supg_term line; and the switch is seen to do something."""
    from burgers_hip import fom
    _, N, graded, _ = next(s for s in ASSEMBLY_SHAPES if s[0] == name)
    rng = np.random.default_rng(N)
    X = _graded(N) if graded else mesh(N)[0]
    B = 6
    uk = 1.0 + 4.0 * rng.random((B, N)); un = 1.0 + 4.0 * rng.random((B, N))
    uk[1, ::5] = 1e-13; uk[1, 1::5] = -1e-13
    mu1 = rng.uniform(4.25, 5.5, B); mu2 = rng.uniform(0.015, 0.03, B)
    off = [t.cpu().numpy() for t in fom.fom_assemble(X, uk, un, mu1, mu2, DT_A, E=E_A, supg=False)]
    on = [t.cpu().numpy() for t in fom.fom_assemble(X, uk, un, mu1, mu2, DT_A, E=E_A)]
    for b in range(B):
        l, d, u, r, bb = oracle_assembly(X, uk[b], un[b], mu1[b], mu2[b], DT_A, E_A, supg=False)
        scale = np.abs(d).max()
        for a, ref in zip(off[:3], (l, d, u)):
            assert np.abs(a[b] - ref).max() < 1e-13 * scale
        assert np.abs(off[3][b] - r).max() < 1e-12 * max(1.0, np.abs(r).max())
        assert all(np.array_equal(a[b], o[b]) for a, o in zip(off[:3], on[:3]))          # SUPG is in the right-hand side only
        assert np.abs(on[3][b] - off[3][b]).max() > 1e-3 * np.abs(bb).max()
