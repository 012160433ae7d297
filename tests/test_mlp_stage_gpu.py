"""The activation stage of the POD-ANN closure: bg_mlp_act_jvp (csrc/mlp.hip) alone through the C ABI, inside
rom.AnnEvaluator against float64 autograd, and its device-loop twin mlp_activate (csrc/wave_ops.hpp, called with m.act[l]
and m.alpha[l] by csrc/rom_ann_device.hpp) inside bg_ann_rom_run, bg_ann_rom_run_wide and bg_hyper_ann_rom_run.  Every entry
point takes the activation kind and alpha PER LAYER.  The stage and the evaluator are given alpha per call, so only the
loop tests can see a loop that reads alpha[0] or a neighbour's kind: their closure (_loop_closure) has two ELU layers
with different alpha, the second one last but one, and each test first asserts that the closure with alpha[0] everywhere
differs by more than 1e-2, where the gate is 5e-6."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import ann_wide_cases as aw
import hyper_ann_ref as har
from conftest import rel_l2
from loop_cases import draw, to_np

pytestmark = pytest.mark.gpu
EPS32, TINY32 = float(np.finfo(np.float32).eps), float(np.finfo(np.float32).tiny)
TOL32 = aw.TOL32
SPECIAL = np.array([0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 100.0, -100.0], dtype=np.float32)
KINDS = {"NONE": 0, "ELU": 1, "RELU": 2, "TANH": 3}                 # BG_ACT_* of include/burgers_hip.h


# ------------------------------------------------------------------------------------ bg_mlp_act_jvp alone
def _stage_inputs(rng, B, n1, h, with_bias, shift):
    """z (B, n1, h) float32 and bias (h,) or None: random values, the SPECIAL ones at the head of the value row, at every
    third place and rotated by ``shift``; every third bias is 0, so that they survive the bias."""
    z = (2.0 * rng.standard_normal((B, n1, h))).astype(np.float32)
    v = z[:, 0, :].reshape(-1)
    m = min(len(v), 3 * len(SPECIAL))
    v[:m] = 0.0
    v[:m:3] = np.roll(SPECIAL, -shift)[:len(v[:m:3])]                # at columns j % 3 == 0 when h % 3 == 0 or B = 1
    z[:, 0, :] = v.reshape(B, h)
    bias = None
    if with_bias:
        bias = rng.standard_normal(h).astype(np.float32)
        bias[::3] = 0.0
    return z, bias


def _stage_ref(z, bias, kind, alpha):
    """float64 numpy from the float32 inputs: act(z0 + bias) and act'(z0 + bias) z_k; act' at 0 as torch autograd has it
    (ELU: alpha, ReLU: 0)."""
    v = z[:, 0, :].astype(np.float64) + (0.0 if bias is None else bias.astype(np.float64))
    a = float(np.float32(alpha))
    with np.errstate(over="ignore"):
        if kind == "ELU":
            val, d = np.where(v > 0, v, a * np.expm1(np.minimum(v, 0.0))), np.where(v > 0, 1.0, a * np.exp(np.minimum(v, 0.0)))
        elif kind == "RELU":
            val, d = np.where(v > 0, v, 0.0), (v > 0).astype(np.float64)
        elif kind == "TANH":
            val, d = np.tanh(v), 1.0 / np.cosh(np.clip(v, -300, 300)) ** 2      # 1 - tanh^2 without its cancellation
        else:
            val, d = v, np.ones_like(v)
    return np.concatenate([val[:, None, :], d[:, None, :] * z[:, 1:, :].astype(np.float64)], axis=1)


def _stage_torch32(z, bias, kind, alpha):
    """The formulas of rom._mlp_forward_jacobian in torch float32 on the CPU: the reference's own arithmetic."""
    zt = torch.from_numpy(z)
    v = zt[:, 0, :] if bias is None else zt[:, 0, :] + torch.from_numpy(bias)
    if kind == "ELU":
        x, d = torch.nn.functional.elu(v, alpha=alpha), torch.where(v > 0, torch.ones_like(v), alpha * torch.exp(v))
    elif kind == "RELU":
        x, d = torch.relu(v), (v > 0).to(v.dtype)
    elif kind == "TANH":
        x = torch.tanh(v); d = 1.0 - x * x
    else:
        x, d = v, torch.ones_like(v)
    return torch.cat([x[:, None, :], d[:, None, :] * zt[:, 1:, :]], dim=1).numpy()


def _ulps(got, ref, z):
    """(value row, tangent rows): the largest |got - ref| / (eps32 max(|ref|, |z_k|, tiny)); the |z_k| term (tangent rows
    only) because 1 - tanh^2 cancels near saturation: its error is an absolute one on the scale of the factor it
    multiplies.  tiny is float32's smallest normal number: it only keeps a reference of 0 from dividing by 0."""
    scale = np.maximum(np.abs(ref), TINY32)
    scale[:, 1:, :] = np.maximum(scale[:, 1:, :], np.abs(z[:, 1:, :]))
    e = np.abs(got.astype(np.float64) - ref) / (EPS32 * scale)
    return float(e[:, 0, :].max()), float(e[:, 1:, :].max(initial=0.0))


def _stage_gpu(hip, z, bias, kind, alpha):
    zd = torch.from_numpy(z).cuda()
    bd = None if bias is None else torch.from_numpy(bias).cuda()
    B, n1, h = z.shape
    hip.check(hip.load().bg_mlp_act_jvp(B, n1, h, hip.ptr(zd), hip.ptr(bd), KINDS[kind], alpha,
                                        hip.stream_ptr(torch.device("cuda", 0))), "bg_mlp_act_jvp")
    torch.cuda.synchronize()
    return zd.cpu().numpy()


def _check_stage(hip, z, bias, kind, alpha, rows=(0, 1)):
    """(cpu, gpu, got): the figures of _ulps as (value row, tangent rows) pairs.  The bound on each of ``rows`` is the
    reference's own arithmetic on the same inputs, times four, and at least 4: expf and tanhf differ between libraries by
    an ulp or two."""
    ref = _stage_ref(z, bias, kind, alpha)
    cpu = _ulps(_stage_torch32(z, bias, kind, alpha), ref, z)
    got = _stage_gpu(hip, z, bias, kind, alpha)
    assert np.isfinite(got).all()                                    # nothing of expf(100) = inf reaches the result
    gpu = _ulps(got, ref, z)
    for r in rows:
        assert gpu[r] <= max(4.0, 4.0 * cpu[r]), (kind, alpha, z.shape, bias is not None, ("value", "tangent")[r], gpu[r], cpu[r])
    return cpu, gpu, got


def _stage_grid(kind):
    """(alpha, z, bias) over alpha in {1, 0.7, 1.7} (ELU), bias given and NULL, n1 in {1, 2, 9}, h in {1, 7, 256, 257} (below,
    at and past one block), B in {1, 5}; 0, -0, +-1e-30, +-20, +-100 among the pre-activations.  The small widths, which
    hold fewer places than there are special values, are run with all eight rotations of them: every special value is met
    at h = 1, with and without a bias, in every kind."""
    rng = np.random.default_rng(KINDS[kind])
    for alpha in ((1.0, 0.7, 1.7) if kind == "ELU" else (1.0,)):
        for with_bias in (True, False):
            for n1 in (1, 2, 9):
                for h in (1, 7, 256, 257):
                    for B in (1, 5):
                        for shift in (range(len(SPECIAL)) if h <= 7 else (0,)):
                            z, bias = _stage_inputs(rng, B, n1, h, with_bias, shift)
                            yield alpha, z, bias


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_act_jvp_against_float64(hip, kind):
    """All four kinds over _stage_grid, value row and tangent rows of every case.  Catches a bias added to the tangent rows, a
    derivative taken after the activation overwrote row 0, alpha missing from the derivative, the wrong side at 0, an
    index that mixes j and k, and a value below zero that has lost its digits: the ELU value used to be
    alpha expf(v) - alpha, exact to eps32 alpha / 2 in absolute terms only, 8388608 ulp (2^23: the value 0 where it should
    be -alpha 1e-30) at v = -1e-30; the kernel now rounds alpha expm1(v) from double once, as torch's ELU takes
    alpha expm1(v).  The device loops' mlp_activate keeps e - alpha (csrc/wave_ops.hpp says why that is enough there).
    Measured, worst over the grid, value | tangent rows, in the unit of _ulps (torch float32 on the CPU, then
    this kernel): ELU 1.00 | 1.13, 0.77 | 1.29; RELU 0.50 | 0, 0.50 | 0; TANH 0.82 | 1.01, 1.10 | 1.08; NONE 0.50 | 0, 0.50 | 0."""
    worst_cpu, worst_gpu = np.zeros(2), np.zeros(2)
    for alpha, z, bias in _stage_grid(kind):
        cpu, gpu, got = _check_stage(hip, z, bias, kind, alpha)
        worst_cpu, worst_gpu = np.maximum(worst_cpu, cpu), np.maximum(worst_gpu, gpu)
        v = z[:, 0, :] + (0.0 if bias is None else bias)
        tangent = lambda mask: np.broadcast_to(mask[:, None, :], z[:, 1:, :].shape)
        if kind == "NONE":                                           # the tangent rows are not touched at all
            assert np.array_equal(got[:, 1:, :].view(np.uint32), z[:, 1:, :].view(np.uint32))
        if kind == "ELU":
            far = v == -100.0                                        # the value is -alpha, the derivative 0
            assert (got[:, 0, :][far] == np.float32(-np.float32(alpha))).all()
            assert (np.abs(got[:, 1:, :]) <= 1e-40 * np.abs(z[:, 1:, :]))[tangent(far)].all()
            big = v == 100.0                                         # expf(100) = inf in the arm that is not taken
            assert (got[:, 0, :][big] == 100.0).all()
            assert np.array_equal(got[:, 1:, :][tangent(big)], z[:, 1:, :][tangent(big)])
    print(f"{kind}: worst value | tangent {worst_cpu[0]:.2f} | {worst_cpu[1]:.2f} ulp (torch float32, CPU), "
          f"{worst_gpu[0]:.2f} | {worst_gpu[1]:.2f} ulp (bg_mlp_act_jvp)")


def test_act_jvp_grid_stride(hip):
    """B = 65537, h = 257, n1 = 1: more than 65536 * 256 elements (67 MB), so the grid is capped and every thread of the
    first blocks takes a second trip; the whole array against the same reference.  Catches a stride computed in 32 bits
    or from the uncapped grid, and a tail that is skipped.  Tanh with a bias; with one row this is a test of the value alone.
    Measured: 0.98 ulp (torch float32 on the CPU), 1.50 ulp (the kernel)."""
    rng = np.random.default_rng(65537)
    z, bias = _stage_inputs(rng, 65537, 1, 257, True, 0)
    assert z.shape[0] * z.shape[2] > 65536 * 256
    cpu, gpu, _ = _check_stage(hip, z, bias, "TANH", 1.0)
    print(f"grid stride: {cpu[0]:.2f} ulp (torch float32, CPU), {gpu[0]:.2f} ulp (bg_mlp_act_jvp)")


# ------------------------------------------------------------------------------------ AnnEvaluator against float64 autograd
def _mixed_model(widths, bias=True, final_tanh=False, seed=0):
    """Linear, ELU(0.7), Linear, Tanh, Linear, ReLU, Linear [, Tanh] over ``widths`` (five of them)."""
    torch.manual_seed(seed)
    lins = [nn.Linear(widths[i], widths[i + 1], bias=bias) for i in range(4)]
    mods = [lins[0], nn.ELU(0.7), lins[1], nn.Tanh(), lins[2], nn.ReLU(), lins[3]] + ([nn.Tanh()] if final_tanh else [])
    return nn.Sequential(*mods).eval()


def _value_and_jacobian(model, q):
    with torch.no_grad():
        val = model(q)
    jac = torch.stack([torch.autograd.functional.jacobian(model, q[i]) for i in range(len(q))])
    return val.numpy().astype(np.float64), jac.numpy().astype(np.float64)


@pytest.mark.parametrize("bias,final_tanh", [(True, False), (False, False), (True, True)])
def test_evaluator_mixed_model_against_float64_autograd(hip, bias, final_tanh):
    """The fused evaluation (one GEMM per layer over the 1 + n rows, bg_mlp_act_jvp per activation) of a model with a
    different kind on every layer, alpha != 1 and, once, an activation on the last layer, against
    torch.autograd.functional.jacobian of the same model in float64 on the CPU.  float32-limited: the float32 module's own
    distance from the float64 result on these inputs, times four.  Measured, max |a - ref| / max |ref|, value | Jacobian:
    float32 module 1.2e-7 .. 2.4e-7 | 2.5e-7 .. 2.8e-7, fused evaluation 1.5e-7 .. 2.2e-7 | 2.1e-7 .. 2.2e-7 (three models).  A stage that took
    alpha or the kind from another layer is off by 1e-1."""
    from burgers_hip import rom
    model = _mixed_model([5, 33, 64, 17, 20], bias, final_tanh, seed=3)
    B, n, nbar = 50, 5, 20
    q32 = torch.from_numpy(np.random.default_rng(4).uniform(-1.0, 1.0, (B, n)).astype(np.float32))
    val64, jac64 = _value_and_jacobian(copy.deepcopy(model).double(), q32.double())
    val32, jac32 = _value_and_jacobian(model, q32)
    dist = lambda a, ref: float(np.abs(a - ref).max() / np.abs(ref).max())
    own = dist(val32, val64), dist(jac32, jac64)
    dev = torch.device("cuda", 0)
    ev = rom.AnnEvaluator(copy.deepcopy(model).cuda(), n, torch.float32)
    jt = torch.zeros((B, n, nbar), dtype=torch.float64, device=dev)
    qs = torch.zeros((B, nbar), dtype=torch.float64, device=dev)
    ev.bind(B, n, dev, jt, qs)
    try:
        assert ev.fused
        ev.eval(q32.double().cuda())
        torch.cuda.synchronize()
        got = dist(to_np(qs), val64), dist(to_np(jt.transpose(1, 2)), jac64)
    finally:
        ev.release()
    print(f"bias={bias} final_tanh={final_tanh}: float32 module {own[0]:.2e} | {own[1]:.2e}, fused {got[0]:.2e} | {got[1]:.2e}")
    assert got[0] <= 4.0 * own[0] and got[1] <= 4.0 * own[1], (got, own)


# ------------------------------------------------------------------------------------ the device loops with a mixed closure
B_LOOP, NT_LOOP = 19, 5


def _loop_closure(n, nbar, seed, scale=0.02):
    """Linear, ELU(1.7), Linear, Tanh, Linear, ReLU, Linear, ELU(0.7), Linear: alphas = [1.7, 1, 1, 0.7, 1] at the entry
    points, so a loop that read alpha[0] (or alpha[l +- 1]) for every layer computes another closure, as does one that
    read the kind of a neighbouring layer.  Scaled as ann_wide_cases.mlp scales its closures: every weight x 0.5, then the
    last layer x ``scale``."""
    torch.manual_seed(seed)
    widths = [n, 33, 64, 17, 24, nbar]
    lins = [nn.Linear(widths[i], widths[i + 1]) for i in range(5)]
    with torch.no_grad():
        for lin in lins:
            lin.weight.mul_(0.5)
        lins[-1].weight.mul_(scale)
        lins[-1].bias.mul_(scale)
    return nn.Sequential(lins[0], nn.ELU(1.7), lins[1], nn.Tanh(), lins[2], nn.ReLU(), lins[3], nn.ELU(0.7), lins[4]).eval()


def _alpha_sensitivity(model, q):
    """Relative change of the closure value on the inputs q (B, n) when every ELU takes the alpha of the first one: what
    a loop that read alpha[0] everywhere would be off by.  The tests need it far above their 5e-6 gate."""
    wrong = copy.deepcopy(model)
    first = next(m.alpha for m in wrong if isinstance(m, nn.ELU))
    for m in wrong:
        if isinstance(m, nn.ELU):
            m.alpha = first
    with torch.no_grad():
        a, b = model(q), wrong(q)
    return float((a - b).norm() / a.norm())


def _compare_with_host(f, b, what):
    """The criteria of test_ann_fused_shapes_and_activations.  Returns the share of samples clean in both paths."""
    fi, bi = to_np(f.iters), to_np(b.iters)
    assert np.abs(fi - bi).max() <= 1
    assert int((f.flags != b.flags).sum().item()) <= 1, (what, f.flags.tolist(), b.flags.tolist())
    ok = to_np((f.flags == 0) & (b.flags == 0))
    print(f"{what}: clean in both paths {ok.mean():.0%}, clean on the host path {float((b.flags == 0).float().mean()):.0%}")
    assert ok.mean() >= 0.8, (what, f.flags.tolist())
    fh, bh = to_np(f.hist), to_np(b.hist)
    errs = [rel_l2(fh[s], bh[s]) for s in np.flatnonzero(ok)]
    print(f"{what}: worst rel-L2 against the host path {max(errs):.2e}")
    assert max(errs) < TOL32, what
    return ok.mean()


@pytest.mark.parametrize("entry,n,nbar", [("bg_ann_rom_run", 4, 12), ("bg_ann_rom_run_wide", 12, 30)])
def test_device_loops_mixed_closure_against_host_path(hip, entry, n, nbar):
    """mlp_activate inside bg_ann_rom_run (N = 100, n = 4, nbar = 12) and bg_ann_rom_run_wide (n = 12, nbar = 30) with
    the layers of _loop_closure, against the host-driven path, whose stage and evaluator the tests above pin to float64.
    Closure scaled as ann_wide_cases.mlp scales its own (last layer x 0.02); 19 samples, 5 steps, both projections.  With
    this draw every sample is clean on the host path and in both paths (100 % in all four runs)."""
    from burgers_hip import rom
    N = 100
    X, Up, Us = aw.bases(N, n, nbar)
    model = _loop_closure(n, nbar, seed=N + n)
    mu1, mu2 = draw(B_LOOP, seed=n)
    q0 = torch.from_numpy((np.ones(N) @ Up).astype(np.float32))[None, :]        # the primary coordinates of u0
    sens = _alpha_sensitivity(model, q0)
    print(f"{entry}: closure with every alpha = alpha[0] differs by {sens:.1e}")
    assert sens > 1e-2
    for proj in ("LSPG", "Galerkin"):
        f = rom.pod_ann_run(X, np.ones(N), mu1, mu2, 0.05, NT_LOOP, Up, Us, model, projection=proj, E=0.001,
                            wide=entry.endswith("wide"))
        b = rom.pod_ann_run(X, np.ones(N), mu1, mu2, 0.05, NT_LOOP, Up, Us, model, projection=proj, E=0.001, fused=False)
        torch.cuda.synchronize()
        assert f.path == entry and b.path == "host"
        _compare_with_host(f, b, f"{entry} {proj}")


def _np_closure(model):
    """(forward, jacobian) with the signatures of oracle.burgers_ref.mlp_forward / mlp_jacobian for ``model``: float32
    numpy, the kind and alpha of every layer read off the nn.Sequential here, not through the library's own parser (the
    weights passed in are ignored)."""
    spec = []
    for m in model:
        if isinstance(m, nn.Linear):
            spec.append([m.weight.detach().cpu().numpy().astype(np.float32),
                         np.zeros(m.out_features, np.float32) if m.bias is None else m.bias.detach().cpu().numpy().astype(np.float32),
                         None])
        else:
            assert spec[-1][2] is None and isinstance(m, (nn.ELU, nn.ReLU, nn.Tanh))
            spec[-1][2] = m

    def activate(act, z):
        if isinstance(act, nn.ELU):
            a = np.float32(act.alpha)
            zn = np.minimum(z, np.float32(0))
            return np.where(z > 0, z, a * np.expm1(zn)).astype(np.float32), np.where(z > 0, np.float32(1), a * np.exp(zn)).astype(np.float32)
        if isinstance(act, nn.ReLU):
            return np.maximum(z, np.float32(0)), (z > 0).astype(np.float32)
        if isinstance(act, nn.Tanh):
            t = np.tanh(z).astype(np.float32)
            return t, (np.float32(1) - t * t).astype(np.float32)
        return z, np.ones_like(z)

    def both(q):
        x = np.asarray(q, dtype=np.float32)
        J = np.eye(len(x), dtype=np.float32)
        for W, b, act in spec:
            z = (W @ x + b).astype(np.float32)
            J = (W @ J).astype(np.float32)
            x, d = activate(act, z)
            J = (d[:, None] * J).astype(np.float32)
        return x, J

    return (lambda Ws, bs, q: both(q)[0]), (lambda Ws, bs, q: both(q)[1])


@pytest.mark.parametrize("proj", ["Galerkin", "LSPG"])
def test_hyper_loop_mixed_closure_against_its_restatement(hip, monkeypatch, proj):
    """bg_hyper_ann_rom_run with the closure of _loop_closure on the smallest sampling tests/hyper_ann_ref.py builds (perturbed-96:
    N = 96, n = 8, nbar = 40, every row with unit weight), against hyper_ann_ref.hyper_ann_prom with the oracle's ELU
    network replaced by a float32 numpy restatement of the mixed model: the gate of tests/test_rom_hyper_ann_gpu.py
    (rel-L2 < 5e-6 on history, q and q_s, counts within 1, no flag)."""
    from burgers_hip import pod, rom
    from oracle import burgers_ref as br
    N, dt, n, nbar, _, _, _, E, _ = har.CASES["perturbed-96"]
    X, Up, Us, _ = har.case_data("perturbed-96")
    model = _loop_closure(n, nbar, seed=96)
    sens = _alpha_sensitivity(model, torch.from_numpy((np.ones(N) @ Up).astype(np.float32))[None, :])
    print(f"{har.ENTRY}: closure with every alpha = alpha[0] differs by {sens:.1e}")
    assert sens > 1e-2
    fwd, jac = _np_closure(model)
    monkeypatch.setattr(br, "mlp_forward", fwd)
    monkeypatch.setattr(br, "mlp_jacobian", jac)
    s = pod.RowSampling(np.arange(N, dtype=np.int32), np.ones(N), proj.lower(), 0.0, 0, 0.0)
    mu1, mu2 = draw(B_LOOP, seed=8)
    res = rom.pod_ann_run_hyper(X, np.ones(N), mu1, mu2, dt, NT_LOOP, Up, Us, model, s, rom.PROJ[proj.lower()], E=E)
    torch.cuda.synchronize()
    assert res.path == har.ENTRY and bool((res.info == 0).all()) and not bool(res.flags.any())
    hist, q, qs, iters = to_np(res.hist), to_np(res.q), to_np(res.q_s), to_np(res.iters)
    worst = 0.0
    for b in range(B_LOOP):
        Q, Qs, it = har.hyper_ann_prom(X, dt, NT_LOOP, np.ones(N), mu1[b], E, mu2[b], Up, Us, None, None, proj,
                                       s.rows.numpy(), s.xi.numpy())
        assert it.max() < 50
        err = rel_l2(hist[b].T, har.decode(Up, Us, Q, Qs, np.ones(N)))
        worst = max(worst, err)
        assert err < TOL32, (proj, b, err)
        assert rel_l2(q[b].T, Q) < TOL32 and rel_l2(qs[b].T, Qs) < TOL32
        assert np.abs(iters[b] - it).max() <= 1, (proj, b)
    print(f"{har.ENTRY} {proj}: worst rel-L2 against the restatement {worst:.2e}")
