"""The two bf16 decoder kernels of csrc/decoder.hip, bg_decode_mlp_bf16 and bg_decode_modes_bf16, held exactly.

A. Integer networks and integer operands.  Integers up to 256 in magnitude are exact in bf16 and sums of fewer than 2^24
   of them are exact in the float32 accumulators, so an int64 numpy evaluation predicts every float64 result bit for bit:
   torch.equal, no tolerance.  A wrong operand or result lane map, a swapped k-block, a bias read at a neighbouring
   offset, a store routed to the wrong (sample, row, time level) is an exact mismatch.  Every test asserts on its own
   reference that the premises hold (magnitudes, at least half of the coefficients non-zero, output features distinct).
B. The activation epilogue value by value: a 16 -> 32 layer that copies its three inputs (W[j][j % 3] = 1) under the
   identity as mode matrix returns bf16(act(bf16(z))) for z = z1[b], z2[b], ztau[0] in features j % 3 = 0, 1, 2.  Every
   finite bf16 value goes through z1 and, in another order, through z2.  None and ReLU are compared bitwise; Tanh and ELU
   by their distance, in units of the last place of bf16, from the float64 value rounded once to bf16, and so is torch's
   own activation on a DEVICE bf16 tensor of the same values: the kernel is gated at torch's figure plus 1 ulp.
   A zero arrives as +0.0 whatever its sign: the input is one term of a float32 sum that starts from +0.0, in the
   kernel as in a Linear layer.
   Measured on an MI355X, worst ulp over the 65280 finite values, torch on the device | this kernel:
       Tanh 0 | 0;  ELU alpha 1.0: 0 | 0;  alpha 1.7: 1 | 1;  alpha 0.3: 1 | 1;  neither is above 1 ulp at any |v|, and all
       65280 results of each run equal torch's bit for bit (torch's device ELU is alpha expm1(v), and so is the kernel's).
       The former epilogue, alpha (expf(v) - 1):  ELU alpha 1.0: 0 | 255, above 1 ulp up to |v| = 3.78e-6;  alpha 1.7:
       1 | 255, up to 4.44e-6;  alpha 0.3: 1 | 254, up to 6.17e-6;  13952, 13947 and 13929 results differed from torch's
       (255 ulp: the value 0 where alpha v is due, once expf(v) rounds to 1).
   Then three ELU layers with three alphas against the rounding-point emulation of tests/test_rom_gpu.py, which here
   takes alpha per layer; the emulation with alpha[0] everywhere is shown to lie outside the gate.
C. decoder.GridDecoder: the one-kernel plan against the PyTorch bf16 module (fused=False) for models with ELU alphas
   other than 1, a Linear without bias and exactly eight layers; and the models the kernel does not cover take the
   PyTorch path.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import rel_l2

pytestmark = pytest.mark.gpu
NONE, ELU, RELU, TANH = 0, 1, 2, 3                                   # BG_ACT_* of include/burgers_hip.h
SENTINEL = -7.25                                                     # no integer result equals it
N_SET = (32, 64, 96, 128, 160)                                       # 1 to 5 row tiles for the four waves
BNT_SET = ((300, 1), (64, 2), (5, 3), (1, 127), (1, 128), (1, 129), (8, 128), (3, 501))
WIDTHS = {16: [16, 32, 256, 96, 64, 128, 32, 224], 8: [16, 32, 128, 96, 64, 128, 32, 96]}      # by MAXKB; then n


def _dev():
    return torch.device("cuda", 0)


def _bf(a):
    """Integers (or any float32-exact values) as a bf16 device tensor."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(_dev())


def _f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(_dev())


def _run_mlp(hip, N, n, B, Nt, Um, z1, z2, zt, widths, Ws, bs, acts, alphas):
    """bg_decode_mlp_bf16 into a sentinel-filled (B, N, Nt) result; bs[l] None is passed as bias[l] = NULL."""
    nl = len(Ws)
    arr = lambda ty, v: (ty * nl)(*v)
    out = torch.full((B, N, Nt), SENTINEL, dtype=torch.float64, device=_dev())
    hip.check(hip.load().bg_decode_mlp_bf16(
        N, n, B, Nt, hip.ptr(Um), hip.ptr(z1), hip.ptr(z2), hip.ptr(zt), nl, arr(ctypes.c_int, widths[:-1]),
        arr(ctypes.c_int, widths[1:]), arr(ctypes.c_void_p, [w.data_ptr() for w in Ws]),
        arr(ctypes.c_void_p, [None if b is None else b.data_ptr() for b in bs]), arr(ctypes.c_int, acts),
        arr(ctypes.c_float, alphas), hip.ptr(out), hip.stream_ptr(_dev())), "bg_decode_mlp_bf16")
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------ A. exact integers
def _int_network(rng, widths, null_bias, relu):
    """[(W int64 (wout, win), bias int64 (wout,) or None, kind)]: entries in {-1, 0, 1}, two non-zeros per row in the first
    three layers and one afterwards, layer 0 in its three real input columns only; bias in [-2, 2], None on the layers
    of ``null_bias``; the last layer's bias is j - n / 2 unless it is in ``null_bias``; ReLU after the layers of ``relu``."""
    nl, net = len(widths) - 1, []
    for l in range(nl):
        win, wout = widths[l], widths[l + 1]
        W = np.zeros((wout, win), dtype=np.int64)
        for j in range(wout):
            k = rng.choice(3 if l == 0 else win, size=2 if l < 3 else 1, replace=False)
            W[j, k] = rng.choice([-1, 1], size=len(k))
        b = rng.integers(-2, 3, wout)                                # drawn on every layer: the weights do not depend on null_bias
        if l == nl - 1:
            b = np.arange(wout, dtype=np.int64) - wout // 2
        net.append((W, None if l in null_bias else b.astype(np.int64), RELU if l in relu else NONE))
    return net


def _int_inputs(rng, N, n, B, Nt):
    return (rng.integers(-4, 5, (N, n)), rng.integers(-2, 3, B), rng.integers(-2, 3, B), rng.integers(-3, 4, Nt))


def _int_reference(net, Um, z1, z2, zt):
    """(coefficients (B Nt, n), result (B, N, Nt), the largest magnitude among inputs, pre- and post-activations), int64."""
    B, Nt = len(z1), len(zt)
    x = np.zeros((B * Nt, 16), dtype=np.int64)
    x[:, 0], x[:, 1], x[:, 2] = np.repeat(z1, Nt), np.repeat(z2, Nt), np.tile(zt, B)
    peak = int(np.abs(x).max())
    for W, b, kind in net:
        x = x @ W.T + (0 if b is None else b)
        peak = max(peak, int(np.abs(x).max()))
        if kind == RELU:
            x = np.maximum(x, 0)
    return x, np.matmul(Um, x.reshape(B, Nt, -1).transpose(0, 2, 1)), peak


def _check_premises(net, Q, ref, peak, distinct):
    assert peak <= 256 and max(int(np.abs(W).max()) for W, _, _ in net) <= 256        # exact in bf16
    assert all(b is None or int(np.abs(b).max()) <= 256 for _, b, _ in net)
    assert int(np.abs(ref).max()) < 2 ** 24                                           # exact in float32
    assert np.count_nonzero(Q) >= 0.5 * Q.size
    if distinct:                                                                      # no two output features coincide
        assert len(np.unique(Q.T, axis=0)) == Q.shape[1]


def _int_case(hip, seed, widths, N, B, Nt, null_bias, relu, distinct=True):
    n = widths[-1]
    rng = np.random.default_rng(seed)
    net = _int_network(rng, widths, null_bias, relu)
    Um, z1, z2, zt = _int_inputs(rng, N, n, B, Nt)
    Q, ref, peak = _int_reference(net, Um, z1, z2, zt)
    _check_premises(net, Q, ref, peak, distinct)
    Ws = [_bf(W) for W, _, _ in net]
    bs = [None if b is None else _bf(b) for _, b, _ in net]
    out = _run_mlp(hip, N, n, B, Nt, _bf(Um), _f64(z1), _f64(z2), _f64(zt), widths, Ws, bs, [k for _, _, k in net],
                   [1.0] * len(net))
    want = torch.from_numpy(ref.astype(np.float64))
    got = out.cpu()
    if not torch.equal(got, want):
        bad = np.argwhere((got != want).numpy())
        raise AssertionError(f"{len(bad)} of {want.numel()} results differ; the first (b, i, t): {bad[:8].tolist()}, "
                             f"got {got.numpy()[tuple(bad[0])]}, want {want.numpy()[tuple(bad[0])]}; rows "
                             f"{sorted(set(bad[:, 1].tolist()))[:16]}, time levels {sorted(set(bad[:, 2].tolist()))[:16]}")


# (n, MAXKB, N, (B, Nt), seed): every n / 32 class, both fragment counts, every N and every (B, Nt) of the sets above at
# least once, and the corners of Nt in {1, 2, 501} by N in {32, 160}.  The seed is the first one from 0 whose network and
# inputs meet _check_premises: two output features coincide whenever both hang on hidden features that are constant over
# the columns (behind a dead ReLU) at the right distance, which most draws have somewhere among 256 features.
MLP_CASES = [(32, 16, 32, (300, 1), 2), (64, 16, 64, (64, 2), 0), (96, 16, 96, (5, 3), 47), (128, 16, 128, (1, 127), 474),
             (160, 16, 160, (1, 128), 614), (192, 16, 32, (1, 129), 2668), (224, 16, 64, (8, 128), 88),
             (256, 16, 96, (3, 501), 614), (256, 8, 160, (300, 1), 1405), (32, 8, 160, (3, 501), 5),
             (160, 8, 32, (3, 501), 98), (64, 8, 160, (64, 2), 9), (96, 8, 32, (64, 2), 11), (128, 8, 128, (8, 128), 54),
             (224, 8, 160, (5, 3), 194), (192, 8, 96, (1, 127), 1545), (160, 8, 64, (1, 129), 1222),
             (32, 16, 128, (1, 128), 18), (256, 16, 160, (8, 128), 88)]


def test_the_mlp_cases_cover_every_axis():
    assert {c[0] for c in MLP_CASES} == set(range(32, 257, 32)) and {c[1] for c in MLP_CASES} == {8, 16}
    assert {c[2] for c in MLP_CASES} == set(N_SET) and {c[3] for c in MLP_CASES} == set(BNT_SET)
    assert {(c[3][1], c[2]) for c in MLP_CASES} >= {(nt, N) for nt in (1, 2, 501) for N in (32, 160)}


@pytest.mark.parametrize("n,maxkb,N,bnt,seed", MLP_CASES)
def test_decode_mlp_eight_integer_layers_exactly(hip, n, maxkb, N, bnt, seed):
    """Eight layers (DEC_MAX_LAYERS), padded widths 16-32-256-96-64-128-32-224-n (sixteen register fragments) or
    16-32-128-96-64-128-32-96-n (eight), ReLU after layers 1 and 4, bias[l] = NULL on layers 2 and 5 (layer 3 has one
    again), the last layer's bias j - n / 2: bit for bit the int64 reference."""
    assert max(WIDTHS[maxkb]) == 16 * maxkb
    _int_case(hip, seed, WIDTHS[maxkb] + [n], N, *bnt, null_bias=(2, 5), relu=(1, 4))


@pytest.mark.parametrize("n,N,bnt,seed", [(32, 32, (5, 3), 0), (160, 96, (1, 129), 69), (256, 160, (64, 2), 0)])
def test_decode_mlp_one_integer_layer_exactly(hip, n, N, bnt, seed):
    """n_layers == 1: the 16 padded inputs straight to the n coefficients, with the j - n / 2 bias."""
    _int_case(hip, seed, [16, n], N, *bnt, null_bias=(), relu=())


@pytest.mark.parametrize("null_bias,seed", [((), 45), (tuple(range(8)), 392)], ids=["every-bias", "no-bias"])
def test_decode_mlp_bias_everywhere_and_nowhere_exactly(hip, null_bias, seed):
    """The network of the eight-layer test with a bias on every layer, and with bias[l] = NULL on every layer (the last
    one included, so two of its output features may then coincide)."""
    _int_case(hip, seed, WIDTHS[16] + [160], 96, 5, 77, null_bias=null_bias, relu=(1, 4), distinct=not null_bias)


@pytest.mark.parametrize("kb", range(1, 17))
def test_decode_modes_integers_exactly(hip, kb):
    """bg_decode_modes_bf16 for all sixteen n / 16 classes, Um in [-4, 4] and Q in [-8, 8], N and (B, Nt) walking
    through the sets of the MLP tests: exactly the int64 product."""
    n, N, (B, Nt) = 16 * kb, N_SET[kb % 5], BNT_SET[kb % 8]
    rng = np.random.default_rng(kb)
    Um, Q = rng.integers(-4, 5, (N, n)), rng.integers(-8, 9, (B * Nt, n))
    ref = np.matmul(Um, Q.reshape(B, Nt, n).transpose(0, 2, 1))
    assert int(np.abs(ref).max()) < 2 ** 24 and np.count_nonzero(ref) >= 0.5 * ref.size
    out = torch.full((B, N, Nt), SENTINEL, dtype=torch.float64, device=_dev())
    Ud, Qd = _bf(Um), _bf(Q)
    hip.check(hip.load().bg_decode_modes_bf16(N, n, B, Nt, hip.ptr(Ud), hip.ptr(Qd), hip.ptr(out), hip.stream_ptr(_dev())),
              "bg_decode_modes_bf16")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(ref.astype(np.float64)))


def test_the_modes_cases_cover_every_axis():
    assert {N_SET[kb % 5] for kb in range(1, 17)} == set(N_SET) and {BNT_SET[kb % 8] for kb in range(1, 17)} == set(BNT_SET)


# ------------------------------------------------------------------------------------ B. the epilogue, value by value
def _finite_bf16():
    """Every finite bf16 value, as float64: 2 x 32640 of them, subnormals and both zeros included."""
    bits = np.arange(0x10000, dtype=np.uint32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    return (bits << 16).view(np.float32).astype(np.float64)


def _round_bf16(x):
    """float64 -> the nearest bf16 (ties to even), as float64, in ONE rounding: through float32 with the discarded part
    kept sticky, so that no float32 tie is made up on the way."""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    bits = f.view(np.uint32).astype(np.int64)
    inexact = f.astype(np.float64) != x
    tie = inexact & ((bits & 0xFFFF) == 0x8000)
    bits = np.where(tie, bits + np.where(np.abs(x) > np.abs(f.astype(np.float64)), 1, -1), bits)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


def _ulp_bf16(ref):
    """The unit in the last place of bf16 at ``ref`` (8 significant bits; 2^-133 in the subnormal range and at 0)."""
    _, e = np.frexp(ref)
    return np.ldexp(1.0, np.maximum(np.where(ref == 0, -126, e - 1), -126) - 7)


def _act64(kind, alpha, v):
    a = float(np.float32(alpha))
    if kind == ELU:
        return np.where(v > 0, v, a * np.expm1(np.minimum(v, 0.0)))
    return {NONE: v, RELU: np.maximum(v, 0.0), TANH: np.tanh(v)}[kind] + 0.0      # + 0.0: -0.0 arrives as +0.0


@pytest.fixture(scope="module")
def probe_inputs():
    v1 = _finite_bf16()
    v2 = v1[np.random.default_rng(2).permutation(len(v1))]
    return v1, v2, -0.75


def _probe(hip, kind, alpha, v1, v2, vt):
    """(B, 3) float64: bf16(act(bf16(z))) for z = v1[b], v2[b], vt as the kernel has it, after asserting that every
    feature j holds the value of input j % 3."""
    B = len(v1)
    W = np.zeros((32, 16)); W[np.arange(32), np.arange(32) % 3] = 1.0
    out = _run_mlp(hip, 32, 32, B, 1, _bf(np.eye(32)), _f64(v1), _f64(v2), _f64([vt]), [16, 32], [_bf(W)], [None], [kind],
                   [alpha]).cpu().numpy()[:, :, 0]
    for j in range(3, 32):
        assert np.array_equal(out[:, j].view(np.int64), out[:, j % 3].view(np.int64)), (kind, alpha, j)
    return out[:, :3]


@pytest.mark.parametrize("kind", [NONE, RELU], ids=["none", "relu"])
def test_epilogue_none_and_relu_bitwise(hip, probe_inputs, kind):
    """Every finite bf16 value through the first and the second input: the float64 result holds exactly that value
    (ReLU: or +0.0), subnormals included; which input reaches which feature is pinned on the way."""
    v1, v2, vt = probe_inputs
    got = _probe(hip, kind, 1.0, v1, v2, vt)
    for c, v in enumerate((v1, v2, np.full(len(v1), vt))):
        want = _act64(kind, 1.0, v)
        bad = np.flatnonzero(got[:, c].view(np.int64) != want.view(np.int64))
        print(f"kind {kind} input {c}: {len(bad)} of {len(v)} values differ" + (f", e.g. {v[bad[:4]]} -> {got[bad[:4], c]}" if len(bad) else ""))
        assert len(bad) == 0, (kind, c, v[bad[:8]], got[bad[:8], c])


def _distances(kind, alpha, v, got):
    """(worst distance in bf16 ulp from the float64 value rounded to bf16, the largest |v| where it exceeds 1 ulp or 0)."""
    ref = _round_bf16(_act64(kind, alpha, v))
    d = np.abs(got - ref) / _ulp_bf16(ref)
    assert np.isfinite(d).all()
    return float(d.max()), float(np.abs(v[d > 1.0]).max(initial=0.0))


@pytest.mark.parametrize("kind,alpha", [(TANH, 1.0), (ELU, 1.0), (ELU, 1.7), (ELU, 0.3)], ids=["tanh", "elu-1.0", "elu-1.7", "elu-0.3"])
def test_epilogue_tanh_and_elu_within_one_ulp_of_torch_on_the_device(hip, probe_inputs, kind, alpha):
    """tanh(v) and alpha expm1(v) in float64, rounded once to bf16, are the reference for both the kernel and
    torch.tanh / torch.nn.functional.elu on a device bf16 tensor of the same 65280 values; the kernel may be one bf16 ulp
    further from it than torch is, anywhere in the range.  The former epilogue alpha (expf(v) - 1) returned 0 where
    expf(v) rounds to 1, 255 ulp from alpha v, and failed this gate for all three alphas (figures at the top)."""
    v1, v2, vt = probe_inputs
    got = _probe(hip, kind, alpha, v1, v2, vt)
    x = torch.from_numpy(v1).to(_dev()).to(torch.bfloat16)
    assert np.array_equal(x.double().cpu().numpy().view(np.int64), v1.view(np.int64))
    y = torch.tanh(x) if kind == TANH else torch.nn.functional.elu(x, alpha=alpha)
    assert y.dtype == torch.bfloat16
    t_worst, t_above = _distances(kind, alpha, v1, y.double().cpu().numpy())
    k_worst, k_above = _distances(kind, alpha, v1, got[:, 0])
    k2_worst, _ = _distances(kind, alpha, v2, got[:, 1])
    differ = int((got[:, 0] != y.double().cpu().numpy()).sum())
    print(f"kind {kind} alpha {alpha}: worst ulp {t_worst:.3f} | {k_worst:.3f} (second input {k2_worst:.3f}); above 1 ulp up to "
          f"|v| = {t_above:.3g} | {k_above:.3g}; {differ} values differ from torch's")
    want_t = _round_bf16(_act64(kind, alpha, np.array([vt])))
    assert np.abs(got[:, 2] - want_t).max() <= (t_worst + 1.0) * _ulp_bf16(want_t)[0]
    assert k_worst <= t_worst + 1.0 and k2_worst <= t_worst + 1.0, (kind, alpha, k_worst, k2_worst, t_worst)


def _emulate(Ws, bs, acts, alphas, Um, z1, z2, zt):
    """The rounding points of the kernel in PyTorch on the device (tests/test_rom_gpu.py, with alpha per layer): bf16
    operands, float32 accumulate, Linear output -> bf16, activation in float32 -> bf16; the contraction in float64."""
    bf = lambda t: t.to(torch.bfloat16)
    B, Nt, n = len(z1), len(zt), Um.shape[1]
    x = torch.zeros((B * Nt, 16), dtype=torch.float32, device=_dev())
    x[:, 0] = bf(z1.float())[:, None].expand(B, Nt).reshape(-1).float()
    x[:, 1] = bf(z2.float())[:, None].expand(B, Nt).reshape(-1).float()
    x[:, 2] = bf(zt.float())[None, :].expand(B, Nt).reshape(-1).float()
    fn = {NONE: lambda v, a: v, ELU: lambda v, a: torch.nn.functional.elu(v, alpha=a), RELU: lambda v, a: torch.relu(v),
          TANH: lambda v, a: torch.tanh(v)}
    for W, b, kind, a in zip(Ws, bs, acts, alphas):
        y = x @ W.float().t()
        x = bf(fn[kind](bf(y if b is None else y + b.float()).float(), a)).float()
    return torch.matmul(Um.double(), x.double().reshape(B, Nt, n).transpose(1, 2))


def test_elu_alpha_is_taken_per_layer(hip):
    """Three ELU layers, alphas 1.7, 0.4, 1.0 (the last one after the output layer), random float weights: the gate of
    test_decode_mlp_c_abi_random_models_and_refusals against the emulation with alpha per layer.  The emulation with
    alpha[0] on every layer, which is what a kernel reading m.alpha[0] would compute, must lie outside that gate."""
    g = torch.Generator(device="cuda").manual_seed(11)
    N, n, B, Nt = 64, 64, 3, 77
    widths, acts, alphas = [16, 64, 96, n], [ELU] * 3, [1.7, 0.4, 1.0]
    bf = lambda t: t.to(torch.bfloat16)
    Ws = [bf(torch.randn((widths[i + 1], widths[i]), device="cuda", generator=g) / widths[i] ** 0.5) for i in range(3)]
    Ws[0][:, 3:] = 0
    bs = [bf(0.1 * torch.randn((widths[i + 1],), device="cuda", generator=g)) for i in range(3)]
    Um = bf(torch.randn((N, n), device="cuda", generator=g))
    z1 = torch.randn((B,), dtype=torch.float64, device="cuda", generator=g)
    z2 = torch.randn((B,), dtype=torch.float64, device="cuda", generator=g)
    zt = torch.linspace(-1.7, 1.7, Nt, dtype=torch.float64, device="cuda")
    out = _run_mlp(hip, N, n, B, Nt, Um, z1, z2, zt, widths, Ws, bs, acts, alphas)
    dist = lambda ref: (float((out - ref).abs().max() / ref.abs().max()), float(torch.linalg.norm(out - ref) / torch.linalg.norm(ref)))
    right = dist(_emulate(Ws, bs, acts, alphas, Um, z1, z2, zt))
    wrong = dist(_emulate(Ws, bs, acts, [alphas[0]] * 3, Um, z1, z2, zt))
    print(f"alpha per layer: max {right[0]:.2e}, rel-L2 {right[1]:.2e}; alpha[0] everywhere: max {wrong[0]:.2e}, rel-L2 {wrong[1]:.2e}")
    assert wrong[0] > 2e-2 and wrong[1] > 2e-3, wrong
    assert right[0] < 2e-2 and right[1] < 2e-3, right


# ------------------------------------------------------------------------------------ C. decoder.GridDecoder
NT_C, MEAN_C, STD_C = 50, [4.8, 0.02, 0.5], [0.4, 0.005, 0.3]


def _stack(dims, acts, bias_off=()):
    lins = [nn.Linear(dims[i], dims[i + 1], bias=i not in bias_off) for i in range(len(dims) - 1)]
    mods = []
    for lin, act in zip(lins, list(acts) + [None]):
        mods += [lin] + ([act] if act is not None else [])
    return nn.Sequential(*mods).eval()


def _decoders(model, N=64, n=32, seed=0):
    from burgers_hip import decoder
    Um = np.random.default_rng(seed).standard_normal((N, n))
    make = lambda fused: decoder.GridDecoder(NT_C, Um, copy.deepcopy(model), MEAN_C, STD_C, dtype=torch.bfloat16, fused=fused)
    return make(True), make(False)


def _draw_mu(B=7):
    rng = np.random.default_rng(9)
    return rng.uniform(4.25, 5.5, B), rng.uniform(0.015, 0.03, B)


@pytest.mark.parametrize("name", ["elu-alphas", "no-bias-in-the-middle", "eight-layers"])
def test_grid_decoder_plan_matches_the_pytorch_bf16_module(hip, name):
    """The plan GridDecoder builds for bg_decode_mlp_bf16 (padding, alphas, a missing bias, eight layers) against the same
    model as a PyTorch bf16 module followed by bg_decode_modes_bf16: the rel-L2 < 5e-3 gate of
    test_decoder_mlp_in_kernel_matches_the_pytorch_bf16_module (one bf16 rounding that falls the other way moves a
    coefficient by 2^-8)."""
    torch.manual_seed(3)
    model = {"elu-alphas": lambda: _stack([3, 32, 64, 32], [nn.ELU(alpha=1.7), nn.ELU(alpha=0.4)]),
             "no-bias-in-the-middle": lambda: _stack([3, 32, 64, 32], [nn.ELU(), nn.Tanh()], bias_off=(1,)),
             "eight-layers": lambda: _stack([3, 32, 64, 96, 128, 96, 64, 40, 32],
                                            [nn.ELU(), nn.Tanh(), nn.ELU(alpha=0.7), nn.ReLU(), nn.ELU(), nn.Tanh(), nn.ELU(alpha=1.3)])}[name]()
    dec, ref = _decoders(model)
    assert dec.plan is not None and ref.plan is None
    assert dec.plan["nl"] == sum(isinstance(m, nn.Linear) for m in model)
    mu1, mu2 = _draw_mu()
    U, V = dec.predict(mu1, mu2), ref.predict(mu1, mu2)
    torch.cuda.synchronize()
    assert U.shape == V.shape == (7, 64, NT_C) and bool(torch.isfinite(U).all())
    err = rel_l2(U.cpu().numpy(), V.cpu().numpy())
    print(f"{name}: rel-L2 between the one-kernel plan and the PyTorch bf16 module {err:.2e}")
    assert err < 5e-3


@pytest.mark.parametrize("name", ["nine-layers", "288-wide", "N-48"])
def test_grid_decoder_takes_the_pytorch_path_beyond_the_kernel(hip, name):
    """Nine Linear layers, a 288-wide hidden layer and a mesh that is no multiple of 32: no plan, the PyTorch module, a
    finite result of the right shape."""
    torch.manual_seed(4)
    N = 48 if name == "N-48" else 64
    model = {"nine-layers": lambda: _stack([3] + [32] * 9, [nn.ELU()] * 8),
             "288-wide": lambda: _stack([3, 288, 32], [nn.ELU()]),
             "N-48": lambda: _stack([3, 32, 32], [nn.ELU()])}[name]()
    dec, _ = _decoders(model, N=N)
    assert dec.plan is None
    U = dec.predict(*_draw_mu())
    torch.cuda.synchronize()
    assert U.shape == (7, N, NT_C) and U.dtype == torch.float64 and bool(torch.isfinite(U).all())
