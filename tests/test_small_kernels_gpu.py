"""Three small kernels through the C ABI, at the sizes and edges their callers never reach.

bg_rbf_eval (csrc/rbf.hip) against np.longdouble numpy of the formulas at the top of that file, both kinds: one, two and
three trips of the Ns loop with a ragged last one, one and two trips of the staging loop over n, the batch grid-stride
beyond 65535 samples; a sample exactly on a centre, a Gaussian that underflows, either output NULL, the refusals.
  The gates are |phi - ref| <= C_PHI (1 + a) (n + 4) 2^-53 phi and |GT - ref| <= C_GT (1 + a) (n + 5) 2^-53 |coef| (2 / dx_k)
  (|d_k| + |xs_k| + 1), a = eps^2 r2: exp(-a) carries a times the relative error of a, r2 is an n-term sum, and d_k is a
  difference whose error is absolute on the scale of xs_k.  C_PHI and C_GT are four times the worst ratio that the same
  formulas in plain float64 numpy reach against the longdouble reference over this file's own inputs (_rbf_cases):
      float64 numpy, worst ratio: phi 0.3924, GT 0.4102  ->  gates C_PHI = 1.57, C_GT = 1.64
      bg_rbf_eval on an MI355X, worst ratio: phi 0.3924, GT 0.4102 (both at n = Ns = 1; 0.19 and 0.08 at n = 17)
bg_quad_features (csrc/rom.hip) bitwise (a product of two doubles is correctly rounded): n = 1 .. 40, a pair table in
  another order than np.triu_indices with i > j among its entries, and 16.86 M elements, one past the 65535 x 256 the
  capped grid covers in one trip.
bg_transpose_batched (csrc/fom.hip) bitwise as int64, NaN payloads, signed zeros and infinities among the entries: one
  element, one row, one column, full and ragged second tiles in either direction.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LD = np.longdouble
GAUSSIAN, IMQ = 0, 1                                                 # BG_RBF_* of include/burgers_hip.h
C_PHI, C_GT = 1.57, 1.64                                             # 4 x 0.3924, 4 x 0.4102: see above
GUARD = 64


def _dev():
    return torch.device("cuda", 0)


def _up(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_dev())


# ------------------------------------------------------------------------------------ bg_rbf_eval
def _rbf_formulas(kind, eps, qp, x_min, dx, Xt, ty):
    """phi (B, Ns), GT (B, n, Ns) and the terms of the gates, all in ``ty`` arithmetic from the float64 operands."""
    qp, x_min, dx, Xt, eps2 = qp.astype(ty), x_min.astype(ty), dx.astype(ty), Xt.astype(ty), ty(eps) * ty(eps)
    xs = ty(2) * ((qp - x_min) / dx) - ty(1)
    d = xs[:, None, :] - Xt[None, :, :]                              # (B, Ns, n)
    r2 = np.zeros(d.shape[:2], dtype=ty)
    for k in range(d.shape[2]):
        r2 = r2 + d[:, :, k] * d[:, :, k]
    a = eps2 * r2
    if kind == GAUSSIAN:
        phi = np.exp(-a); coef = ty(-2) * eps2 * phi
    else:
        phi = ty(1) / np.sqrt(ty(1) + a); coef = -eps2 * (phi * phi * phi)
    GT = (coef[:, None, :] * (ty(2) / dx)[None, :, None]) * d.transpose(0, 2, 1)
    gscale = np.abs(coef)[:, None, :] * (ty(2) / dx)[None, :, None] * (np.abs(d).transpose(0, 2, 1) + np.abs(xs)[:, :, None] + ty(1))
    return phi, GT, a, gscale


def _rbf_ratios(phi, GT, ref):
    """|phi - ref| and |GT - ref| element by element, in units of the gates' right-hand sides without their constants."""
    rphi, rGT, a, gscale = ref
    n = GT.shape[1]
    u = LD(2) ** -53
    e_phi = np.abs(phi.astype(LD) - rphi) / ((1 + a) * (n + 4) * u * rphi)
    e_gt = np.abs(GT.astype(LD) - rGT) / ((1 + a)[:, None, :] * (n + 5) * u * gscale)
    return e_phi.astype(np.float64), e_gt.astype(np.float64)


def _rbf_inputs(B, n, Ns, seed):
    rng = np.random.default_rng(seed)
    Xt = rng.uniform(-1.0, 1.0, (Ns, n))
    x_min, dx = rng.uniform(-2.0, 1.0, n), rng.uniform(0.5, 3.0, n)
    qp = x_min + dx * rng.uniform(0.0, 1.0, (B, n))
    return qp, x_min, dx, Xt


# (B, n, Ns): Ns below, at and past one and two trips of the 256 threads; n = 257 takes the staging loop twice; the last
# case runs the batch grid-stride (65535 workgroups, six of them twice)
RBF_SHAPES = [(3, 17, 1), (3, 17, 255), (3, 17, 256), (3, 17, 257), (3, 17, 700), (3, 1, 65), (3, 20, 65), (3, 257, 65),
              (65541, 1, 1)]
RBF_EPS = 0.6                                                        # a = eps^2 r2 reaches 4 at n = 17 and 70 at n = 257


def _rbf_cases():
    for shape in RBF_SHAPES:
        for kind in (GAUSSIAN, IMQ):
            yield shape, kind, _rbf_inputs(*shape, seed=sum(shape) + kind)


def _rbf_gpu(hip, kind, eps, qp, x_min, dx, Xt, want_phi=True, want_gt=True):
    """(phi, GT) as numpy, each with GUARD doubles of sentinel behind it (returned as the third and fourth value)."""
    B, n = qp.shape
    Ns = Xt.shape[0]
    phi = torch.full((B * Ns + GUARD,), -7.25, dtype=torch.float64, device=_dev())
    GT = torch.full((B * n * Ns + GUARD,), -7.25, dtype=torch.float64, device=_dev())
    ops = [_up(qp), _up(x_min), _up(dx), _up(Xt.T)]                  # (held until the call has run)
    hip.check(hip.load().bg_rbf_eval(B, n, Ns, kind, eps, *[hip.ptr(t) for t in ops], hip.ptr(phi if want_phi else None),
                                     hip.ptr(GT if want_gt else None), hip.stream_ptr(_dev())), "bg_rbf_eval")
    torch.cuda.synchronize()
    phi, GT = phi.cpu().numpy(), GT.cpu().numpy()
    return phi[:B * Ns].reshape(B, Ns), GT[:B * n * Ns].reshape(B, n, Ns), phi[B * Ns:], GT[B * n * Ns:]


def numpy_float64_ratios():
    """What C_PHI and C_GT are four times of: plain float64 numpy of the same formulas against the longdouble reference
    over the inputs of test_rbf_eval_against_longdouble (`python tests/test_small_kernels_gpu.py` prints it)."""
    worst = np.zeros(2)
    for shape, kind, inp in _rbf_cases():
        ref = _rbf_formulas(kind, RBF_EPS, *inp, LD)
        phi, GT, _, _ = _rbf_formulas(kind, RBF_EPS, *inp, np.float64)
        worst = np.maximum(worst, [e.max() for e in _rbf_ratios(phi, GT, ref)])
    return worst


@pytest.mark.parametrize("kind", [GAUSSIAN, IMQ], ids=["gaussian", "imq"])
@pytest.mark.parametrize("B,n,Ns", RBF_SHAPES)
def test_rbf_eval_against_longdouble(hip, B, n, Ns, kind):
    """phi and GT of both kinds within the gates at the top of the file, element by element, over RBF_SHAPES; the
    sentinel behind either buffer untouched."""
    inp = _rbf_inputs(B, n, Ns, seed=B + n + Ns + kind)
    ref = _rbf_formulas(kind, RBF_EPS, *inp, LD)
    phi, GT, g1, g2 = _rbf_gpu(hip, kind, RBF_EPS, *inp)
    assert (g1 == -7.25).all() and (g2 == -7.25).all()
    assert np.isfinite(phi).all() and np.isfinite(GT).all()
    e_phi, e_gt = _rbf_ratios(phi, GT, ref)
    print(f"B {B} n {n} Ns {Ns} kind {kind}: worst ratio phi {e_phi.max():.4f} (gate {C_PHI}), GT {e_gt.max():.4f} (gate {C_GT})")
    if B > 65535:                                                    # both sides of the grid-stride seam, by name
        for b in (0, 65534, 65535, 65536, B - 1):
            assert phi[b, 0] > 0 and e_phi[b].max() <= C_PHI and e_gt[b].max() <= C_GT, b
    assert e_phi.max() <= C_PHI and e_gt.max() <= C_GT, (e_phi.max(), e_gt.max())


def _on_centre_inputs(n=17, Ns=5):
    """Sample b exactly on centre b: x_min = 0 and dx = 2 make xs = qp - 1, exact for centres on a 2^-10 grid."""
    rng = np.random.default_rng(3)
    Xt = rng.integers(-1024, 1025, (Ns, n)) / 1024.0
    return Xt + 1.0, np.zeros(n), np.full(n, 2.0), Xt


@pytest.mark.parametrize("kind", [GAUSSIAN, IMQ], ids=["gaussian", "imq"])
def test_rbf_eval_sample_on_a_centre(hip, kind):
    """r2 = 0: phi is exactly 1 and every gradient factor of that centre exactly 0; the other centres within the gates."""
    inp = _on_centre_inputs()
    phi, GT, _, _ = _rbf_gpu(hip, kind, RBF_EPS, *inp)
    for b in range(len(inp[0])):
        assert phi[b, b] == 1.0 and (GT[b, :, b] == 0.0).all(), (b, phi[b, b], GT[b, :, b])
    e_phi, e_gt = _rbf_ratios(phi, GT, _rbf_formulas(kind, RBF_EPS, *inp, LD))
    assert e_phi.max() <= C_PHI and e_gt.max() <= C_GT, (e_phi.max(), e_gt.max())


def test_rbf_eval_gaussian_underflow(hip):
    """eps = 40: exp(-1600 r2) is below the smallest float64 for every centre but the sample's own.  phi and GT stay
    finite, phi >= 0, and both are exactly 0 where a = eps^2 r2 > 760 (exp(-745.2) is the last non-zero double)."""
    inp = _on_centre_inputs()
    _, _, a, _ = _rbf_formulas(GAUSSIAN, 40.0, *inp, LD)
    phi, GT, _, _ = _rbf_gpu(hip, GAUSSIAN, 40.0, *inp)
    far = np.asarray(a > 760)
    assert far.sum() == far.size - len(inp[0])                       # every centre but the own one
    assert np.isfinite(phi).all() and np.isfinite(GT).all() and (phi >= 0).all()
    assert (phi[far] == 0.0).all() and (GT[np.broadcast_to(far[:, None, :], GT.shape)] == 0.0).all()
    assert (phi[~far] == 1.0).all()


@pytest.mark.parametrize("kind", [GAUSSIAN, IMQ], ids=["gaussian", "imq"])
def test_rbf_eval_either_output_null(hip, kind):
    """phi = NULL with GT given, and the reverse: the buffer that is given holds the bits of a call with both, the
    sentinel behind it and the buffer that was withheld are untouched."""
    inp = _rbf_inputs(3, 20, 300, seed=8)
    phi, GT, _, _ = _rbf_gpu(hip, kind, RBF_EPS, *inp)
    p1, g1, pg, gg = _rbf_gpu(hip, kind, RBF_EPS, *inp, want_phi=False)
    assert np.array_equal(g1.view(np.int64), GT.view(np.int64)) and (p1 == -7.25).all() and (pg == -7.25).all() and (gg == -7.25).all()
    p2, g2, pg, gg = _rbf_gpu(hip, kind, RBF_EPS, *inp, want_gt=False)
    assert np.array_equal(p2.view(np.int64), phi.view(np.int64)) and (g2 == -7.25).all() and (pg == -7.25).all() and (gg == -7.25).all()


def test_rbf_eval_refusals(hip):
    L = hip.load()
    buf = torch.zeros(64, dtype=torch.float64, device=_dev())
    p, z = hip.ptr(buf), ctypes.c_void_p(0)
    call = lambda B, n, Ns, kind, phi=p, GT=p: L.bg_rbf_eval(B, n, Ns, kind, 0.5, p, p, p, p, phi, GT, z)
    assert call(1, 2, 2, 2) == hip.BG_ERR_BAD_ARG                    # unknown kind
    assert call(1, 0, 2, GAUSSIAN) == hip.BG_ERR_BAD_ARG
    assert call(1, 2, 0, IMQ) == hip.BG_ERR_BAD_ARG
    assert call(-1, 2, 2, GAUSSIAN) == hip.BG_ERR_BAD_ARG
    assert call(1, 2, 2, GAUSSIAN, phi=z, GT=z) == hip.BG_ERR_BAD_ARG          # both outputs null
    assert L.bg_rbf_eval(0, 2, 2, IMQ, 0.5, z, z, z, z, z, z, z) == hip.BG_OK  # empty batch: no pointer is looked at
    torch.cuda.synchronize()
    assert not bool(buf.any())


# ------------------------------------------------------------------------------------ bg_quad_features
def _quad(hip, q, I, J):
    B, n = q.shape
    feat = torch.full((B, n + len(I)), -7.25, dtype=torch.float64, device=_dev())
    ops = [_up(q), _up(I, np.int32), _up(J, np.int32)]              # (held until the call has run)
    hip.check(hip.load().bg_quad_features(B, n, *[hip.ptr(t) for t in ops], hip.ptr(feat), hip.stream_ptr(_dev())), "bg_quad_features")
    torch.cuda.synchronize()
    return feat.cpu()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


@pytest.mark.parametrize("B", [1, 7, 300])
@pytest.mark.parametrize("n", [1, 2, 21, 40])
def test_quad_features_bitwise(hip, n, B):
    """[q | q_i q_j] with the pairs in np.triu_indices order and in a shuffled order with half of the pairs turned round
    (i > j): the kernel takes the tables as they are given."""
    rng = np.random.default_rng(100 * n + B)
    q = rng.standard_normal((B, n))
    I, J = np.triu_indices(n)
    perm, flip = rng.permutation(len(I)), rng.random(len(I)) < 0.5
    I2, J2 = np.where(flip, J[perm], I[perm]), np.where(flip, I[perm], J[perm])
    assert n < 3 or ((I2 > J2).any() and not np.array_equal(I2, I))
    for a, b in ((I, J), (I2, J2)):
        want = torch.from_numpy(np.concatenate([q, q[:, a] * q[:, b]], axis=1))
        assert _same_bits(_quad(hip, q, a, b), want)


def test_quad_features_second_trip_of_the_grid_stride(hip):
    """n = 40, B = 19600: 16 856 000 elements, 79 040 more than the 65535 x 256 of the capped grid; compared in full."""
    n, B = 40, 19600
    q = np.random.default_rng(1).standard_normal((B, n))
    I, J = np.triu_indices(n)
    assert B * (n + len(I)) > 65535 * 256
    assert _same_bits(_quad(hip, q, I, J), torch.from_numpy(np.concatenate([q, q[:, I] * q[:, J]], axis=1)))


def test_quad_features_refusals(hip):
    L = hip.load()
    buf = torch.zeros(16, dtype=torch.float64, device=_dev())
    p, z = hip.ptr(buf), ctypes.c_void_p(0)
    assert L.bg_quad_features(0, 3, z, z, z, z, z) == hip.BG_OK
    assert L.bg_quad_features(1, 0, p, p, p, p, z) == hip.BG_ERR_BAD_ARG
    assert L.bg_quad_features(-1, 3, p, p, p, p, z) == hip.BG_ERR_BAD_ARG
    for args in ((z, p, p, p), (p, z, p, p), (p, p, z, p), (p, p, p, z)):
        assert L.bg_quad_features(1, 2, *args, z) == hip.BG_ERR_BAD_ARG


# ------------------------------------------------------------------------------------ bg_transpose_batched
def _transpose(hip, t, B, rows, cols):
    out = torch.full((B, cols, rows), -7.25, dtype=torch.float64, device=_dev())
    hip.check(hip.load().bg_transpose_batched(B, rows, cols, hip.ptr(t), hip.ptr(out), hip.stream_ptr(_dev())), "bg_transpose_batched")
    torch.cuda.synchronize()
    return out


def _special_tensor(B, rows, cols):
    """Random doubles with quiet and signalling NaNs of distinct payloads, +-0.0 and +-inf at random places (as many
    of them as fit), built as bit patterns so that nothing canonicalises them on the way."""
    rng = np.random.default_rng(B + 10 * rows + 1000 * cols)
    bits = rng.standard_normal(B * rows * cols).view(np.int64)
    special = np.array([0x7FF8000000000001, 0x7FF80000DEADBEEF, 0xFFF8000000000123, 0x7FF0000000000001, 0xFFF4000000000042,
                        0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000], dtype=np.uint64).view(np.int64)
    m = min(len(bits), len(special))
    bits[rng.choice(len(bits), size=m, replace=False)] = np.roll(special, rows)[:m]
    return torch.from_numpy(bits.reshape(B, rows, cols)).to(_dev())


@pytest.mark.parametrize("B,rows,cols", [(1, 1, 1), (2, 31, 33), (3, 32, 32), (2, 33, 65), (1, 1, 700), (1, 700, 1), (5, 64, 96), (3, 100, 37)])
def test_transpose_batched_bitwise(hip, B, rows, cols):
    """out[b][c][r] = in[b][r][c] as int64, and back again."""
    t = _special_tensor(B, rows, cols)
    out = _transpose(hip, t.view(torch.float64), B, rows, cols)
    assert torch.equal(out.view(torch.int64).cpu(), t.cpu().transpose(1, 2).contiguous())
    back = _transpose(hip, out, B, cols, rows)
    assert torch.equal(back.view(torch.int64).cpu(), t.cpu())


def test_transpose_batched_empty_and_negative_dimensions(hip):
    L = hip.load()
    src = torch.ones(64, dtype=torch.float64, device=_dev())
    out = torch.full((64,), -7.25, dtype=torch.float64, device=_dev())
    z = ctypes.c_void_p(0)
    for dims in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
        assert L.bg_transpose_batched(*dims, hip.ptr(src), hip.ptr(out), z) == hip.BG_OK
    for dims in ((-1, 4, 4), (2, -1, 4), (2, 4, -1)):
        assert L.bg_transpose_batched(*dims, hip.ptr(src), hip.ptr(out), z) == hip.BG_ERR_BAD_ARG
    assert L.bg_transpose_batched(1, 4, 4, z, hip.ptr(out), z) == hip.BG_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.25).all())


if __name__ == "__main__":
    print("float64 numpy against longdouble, worst ratio: phi %.4f, GT %.4f" % tuple(numpy_float64_ratios()))
