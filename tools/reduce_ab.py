#!/usr/bin/env python3
"""A/B of two library builds on the reduce entry points: one process per build (BG_LIB_PATH picks the library) runs a fixed,
seeded list of bg_rom_reduce / _indexed / _lifted / _frag / bg_rom_lift calls and prints one JSON line per call with a
SHA-256 per output tensor (Ar, br, wtu, Uout); two runs are compared with diff or with --against:

  BG_LIB_PATH=/path/to/libother.so python tools/reduce_ab.py > a.jsonl
  python tools/reduce_ab.py --against a.jsonl

Every call has B = 700 samples with holes in the active mask (more samples than workgroups: the persistent loop iterates).
The kernels sum in a fixed order, so two builds that claim the same arithmetic must agree in every hash."""
import argparse
import hashlib
import json
import os
import sys

from _timing import np, torch                  # also puts the package on the import path

ap = argparse.ArgumentParser()
ap.add_argument("--against", help="the output of another run: exit 1 unless every hash matches")
a = ap.parse_args()

from burgers_hip import lib, rom

B = 700
BOTH = [(512, 40), (512, 21), (256, 40), (255, 17), (130, 8)]        # every mode, also with BG_OPT_MFMA_16X16
WIDE = [(512, 47), (300, 44), (128, 41)]                             # the default route to the 16x16x4 shape
FRAG = [(512, 40), (256, 21)]                                        # bg_quad_tangent -> bg_rom_reduce_frag
L = lib.load()
dev = torch.device("cuda", 0)
f64 = dict(dtype=torch.float64, device=dev)


def holes(rng):
    act = np.ones(B, dtype=np.int32)
    act[rng.choice(B, B // 7, replace=False)] = 0
    act[300:340] = 0
    act[5::256] = 0
    act[0] = 1; act[B - 1] = 1
    return act


def digest(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]


lines = []


def report(tag, **tensors):
    lines.append(json.dumps({"call": tag, **{k: digest(v) for k, v in tensors.items()}}))
    print(lines[-1], flush=True)


def outs(r):
    return torch.full((B, r, r), -7.0, **f64), torch.full((B, r), -7.0, **f64), torch.full((B, r), -7.0, **f64)


def case(N, r, seed):
    rng = np.random.default_rng(seed)
    X = np.linspace(0, 100, N)
    Un = 1 + 4 * rng.random((B, N))
    c = rom._setup(X, Un, rng.uniform(4.25, 5.5, B), rng.uniform(0.015, 0.03, B), 0.05, 0.004, None)
    Ud = torch.as_tensor(1 + 4 * rng.random((B, N)), device=dev)
    G = torch.empty_like(Ud); rom._mass_rhs(c, torch.as_tensor(Un, device=dev), G)
    return rng, c, Ud, G, torch.as_tensor(holes(rng), device=dev)


def modes(N, r, opts, tag):
    rng, c, Ud, G, act = case(N, r, 1000 * N + r)
    Wsh = torch.as_tensor(rng.standard_normal((N, r)), device=dev)
    Wps = torch.as_tensor(rng.standard_normal((B, N, r)), device=dev)
    stack = torch.as_tensor(rng.standard_normal((5, N, r)), device=dev)
    widx = rng.integers(0, 5, B).astype(np.int32)
    widx[256:512] = widx[0:256]; widx[512:] = (widx[0:B - 512] + 1) % 5
    widx = torch.as_tensor(widx, device=dev)
    q = torch.as_tensor(rng.standard_normal((B, r)) * 3.0, device=dev)
    for proj, pname in ((0, "galerkin"), (1, "lspg")):
        for mode in ("shared", "persample", "colmajor", "indexed"):
            Ar, br, wtu = outs(r)
            if mode == "indexed":
                rom.rom_reduce(c, stack, Ud, G, proj, True, act, Ar, br, wtu, w_index=widx, extra_opts=opts)
            else:
                W = Wsh if mode == "shared" else (Wps.transpose(1, 2).contiguous() if mode == "colmajor" else Wps)
                rom.rom_reduce(c, W, Ud, G, proj, True, act, Ar, br, wtu, colmajor=(mode == "colmajor"), extra_opts=opts)
            report(f"{tag} N={N} r={r} {pname} {mode}", Ar=Ar, br=br, wtu=wtu)
        Ar, br, wtu = outs(r)
        Uout = torch.full((B, N), -7.0, **f64)
        rom.rom_reduce_lifted(c, Wsh, q, Uout, G, proj, True, act, Ar, br, wtu, extra_opts=opts)
        report(f"{tag} N={N} r={r} {pname} lifted", Ar=Ar, br=br, wtu=wtu, Uout=Uout)


for N, r in BOTH:
    modes(N, r, 0, "default")
    modes(N, r, lib.BG_OPT_MFMA_16X16, "force16")
for N, r in WIDE:
    modes(N, r, 0, "default")
for N, r in FRAG:
    rng, c, Ud, G, act = case(N, r, 3 * N + r)
    NP, per = int(L.bg_rom_frag_pad(r)), int(L.bg_rom_frag_elems(N, r))
    Phi = torch.as_tensor(rng.standard_normal((N, r)), device=dev)
    H3p = torch.nn.functional.pad(torch.as_tensor(rng.standard_normal((N, r, r)), device=dev), (0, NP - r)).contiguous()
    qp = torch.nn.functional.pad(torch.as_tensor(rng.standard_normal((B, r)), device=dev), (0, NP - r)).contiguous()
    Wf = torch.full((B, per), -7.0, **f64)
    lib.check(L.bg_quad_tangent(N, B, r, lib.ptr(Phi), lib.ptr(H3p), lib.ptr(qp), lib.ptr(act), lib.ptr(Wf), c.stream()),
              "bg_quad_tangent")
    for proj, pname in ((0, "galerkin"), (1, "lspg")):
        for with_wtu in (True, False):
            Ar, br, wtu = outs(r)
            lib.check(L.bg_rom_reduce_frag(N, B, r, proj, lib.ptr(c.X), lib.ptr(Wf), lib.ptr(Ud), lib.ptr(G), lib.ptr(c.hfs),
                                           lib.ptr(c.mu1), c.dt, c.E, c.mesh_opt, lib.ptr(act), lib.ptr(Ar), lib.ptr(br),
                                           lib.ptr(wtu if with_wtu else None), c.stream()), "bg_rom_reduce_frag")
            report(f"frag N={N} r={r} {pname} wtu={with_wtu}", Wf=Wf, Ar=Ar, br=br, wtu=wtu)
rng, c, Ud, G, act = case(300, 21, 77)
Phi = torch.as_tensor(rng.standard_normal((300, 21)), device=dev)
q = torch.as_tensor(rng.standard_normal((B, 21)), device=dev)
Uout = torch.full((B, 300), -7.0, **f64)
rom.rom_lift(c, Phi, q, Uout, act)
report("lift N=300 r=21", Uout=Uout)

if a.against:
    other = [l.strip() for l in open(a.against) if l.startswith("{")]
    bad = [(x, y) for x, y in zip(lines, other) if x != y]
    print(json.dumps({"library": os.path.basename(os.environ.get("BG_LIB_PATH", "product")), "against": a.against,
                      "calls": len(lines), "calls_other": len(other), "mismatches": len(bad)}))
    for x, y in bad:
        print("this :", x); print("other:", y)
    sys.exit(1 if bad or len(lines) != len(other) else 0)
