#!/usr/bin/env python3
"""A/B of two library builds on the LDS-streaming POD loops and the hyper-reduced loops: one process per build (BG_LIB_PATH
picks the library), every output array compared bit for bit through a file.

  BG_LIB_PATH=1d-burgers-equation-roms_amd/build/libvar_parent.so python tools/stream_ab.py --save /tmp/stream_a.npz
  python tools/stream_ab.py --against /tmp/stream_a.npz
  ... --only table/       only the workloads whose names start with one of these comma-separated prefixes

Workloads (the shapes of the tests, built by the test modules' own functions):
  hyper/<case>/<proj>/<fast|pivoted>  the two FULL cases of tests/test_rom_hyper_gpu.py, without and with BG_OPT_FORCE_PIVOTED
  hyper/sampled/<proj>                that file's sampled_case (N = 2049), B = 3
  wide/<proj>                         bg_rom_run_wide, the committed r = 96 basis (N = 512), B = 8, 12 steps
  long/<proj>/<fast|pivoted>          bg_rom_run_long, N = 1024, r = 40, B = 4, 12 steps
  long_wide/<proj>                    bg_rom_run_long_wide, N = 1024, r = 96, B = 4, 12 steps
  local_long/<proj>                   bg_local_rom_run_long on the clustering of tests/test_local_long_rom_gpu.py, 40 steps
  table/<loop>/<shape>/<proj>         the four loops that run on the table of a row sampling (csrc/rom_hyper_table_device.hpp),
                                      <loop> = rbf, ann, ann_wide, quad, one <shape> per instantiation of the loop's kernel:
      full-256    all rows of a uniform mesh of 256 nodes, the S = 4 kernels' whole table (quad: four full slabs)
      left-out    perturbed-96 with rows 10, 50, 51, 70 left out: table nodes that are only neighbours between sampled rows
      committed   rbf, ann: the builder's sampling of the committed closure, N = 512   } a table of 257 .. 512 nodes
      spread      ann_wide: the tests' sampling of that name on N = 2049                }
      limits      256 rows, a table of 513 .. 768 nodes (quad: N = 1024, the others N = 2049)
    Rows and table nodes are kept with the outputs and printed; "instantiation": false marks a shape that missed its kernel.
The second call prints one JSON line per workload: the iterations run and whether q / hist, q_s, iters, flags, info (and
clusters) are identical as bit patterns."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "1d-burgers-equation-roms_amd"), os.path.join(REPO, "tests")]

ap = argparse.ArgumentParser()
ap.add_argument("--save")
ap.add_argument("--against")
ap.add_argument("--only", default="")
a = ap.parse_args()

import torch
import test_local_long_rom_gpu as tl
import test_rom_hyper_gpu as th
from burgers_hip import lib, rom
from loop_cases import draw, pod_basis

out = {}


def want(group):
    return not a.only or any(group.startswith(p) or p.startswith(group) for p in a.only.split(","))


def keep(name, res, fields=("hist", "iters", "flags", "info")):
    torch.cuda.synchronize()
    for k in fields:
        out[f"{name}:{k}"] = getattr(res, k).cpu().numpy()


PROJS = ("Galerkin", "LSPG")
for proj in PROJS:
    p = rom.PROJ[proj.lower()]
    for case in sorted(th.FULL) if want("hyper/") else ():
        for tag, opts in (("fast", 0), ("pivoted", lib.BG_OPT_FORCE_PIVOTED)):
            keep(f"hyper/{case}/{proj}/{tag}", th.full_run(case, proj, opts)[0], ("q", "iters", "flags", "info"))
    if want("hyper/"):
        X, Phi, s = th.sampled_case(proj)
        mu1, mu2 = draw(3, seed=11)
        keep(f"hyper/sampled/{proj}", rom.pod_prom_run_hyper(X, np.ones(th.LN), mu1, mu2, th.LDT, th.NT, Phi, s, p),
             ("q", "iters", "flags", "info"))
        out[f"hyper/sampled/{proj}:rows"] = s.rows.cpu().numpy()
        out[f"hyper/sampled/{proj}:xi"] = s.xi.cpu().numpy()

    if want("wide/"):
        X5 = np.linspace(0.0, 100.0, 512)
        Phi96 = np.load(os.path.join(REPO, "tests", "golden", "committed_pod_r96.npz"))["Phi"]
        mu1, mu2 = draw(8)
        res = rom.pod_prom_run_wide(X5, np.ones(512), mu1, mu2, 0.05, 12, Phi96, p)
        assert res.path == "bg_rom_run_wide"
        keep(f"wide/{proj}", res)

    N, dt = 1024, 0.025
    mu1, mu2 = draw(4)
    if want("long/"):
        X, Phi = pod_basis(N, dt, 40)
        for tag, opts in (("fast", 0), ("pivoted", lib.BG_OPT_FORCE_PIVOTED)):
            keep(f"long/{proj}/{tag}", rom.pod_prom_run_long(X, np.ones(N), mu1, mu2, dt, 12, Phi, p, options=opts))
    if want("long_wide/"):
        X, Phi = pod_basis(N, dt, 96)
        keep(f"long_wide/{proj}", rom.pod_prom_run_long_wide(X, np.ones(N), mu1, mu2, dt, 12, Phi, p))

    if want("local_long/"):
        X, centres, bases, Ug = tl._clustering(N, dt)
        mus = tl.MUS[proj]
        res = rom.local_prom_run_long(X, np.ones(N), [m[0] for m in mus], [m[1] for m in mus], dt, tl.NT, centres, bases, Ug, 12,
                                      projection=proj)
        assert res.path == tl.ENTRY
        keep(f"local_long/{proj}", res, ("hist", "iters", "flags", "info", "clusters"))

if want("table/"):
    import hyper_ann_ref as har
    import hyper_ann_wide_cases as hw
    import hyper_quad_ref as hq
    import hyper_rbf_ref as hrr
    import test_rom_hyper_ann_gpu as ta
    import test_rom_hyper_ann_wide_gpu as tw
    import test_rom_hyper_quad_gpu as tq
    import test_rom_hyper_rbf_gpu as tr

    BUCKET = {"full-256": (256, 256), "left-out": (1, 256), "committed": (257, 512), "spread": (257, 512), "limits": (513, 768)}

    def keep_table(loop, shape, proj, res, fields=("q", "q_s", "iters", "flags", "info")):
        lo, hi = BUCKET[shape]
        keep(f"table/{loop}/{shape}/{proj}", res, fields)
        out[f"table/{loop}/{shape}/{proj}:nodes"] = np.array([res.plan.m, res.plan.n_nodes, lo <= res.plan.n_nodes <= hi])

    for proj in PROJS:
        p = rom.PROJ[proj.lower()]
        ones = lambda N: (np.arange(N), np.ones(N))
        # bg_hyper_rbf_rom_run: the runs of tests/test_rom_hyper_rbf_gpu.py
        if want("table/rbf/"):
            X, dt, E, cl = hrr.case_data("full-256", "gaussian")
            keep_table("rbf", "full-256", proj, tr.run(X, dt, E, cl, "gaussian", hrr.sampling(*ones(256), proj), proj, *draw(3), hrr.NT_ALL))
            kernel, pick = hrr.LEFT_OUT_RUNS[proj]
            X, dt, E, cl = hrr.case_data("perturbed-96", kernel)
            rows = hrr.left_out_rows()
            mu1, mu2 = (v[list(pick)] for v in draw(10))
            keep_table("rbf", "left-out", proj, tr.run(X, dt, E, cl, kernel, hrr.sampling(rows, np.ones(len(rows)), proj), proj, mu1, mu2,
                                                       hrr.NT_LEFT))
            kernel = {"Galerkin": "gaussian", "LSPG": "imq"}[proj]
            X, dt, cl = hrr.committed(kernel)
            keep_table("rbf", "committed", proj, tr.run(X, dt, 0.0, cl, kernel, hrr.committed_sampling(kernel, proj), proj, *draw(4), 8))
            X, dt, E, cl = hrr.long_data()
            keep_table("rbf", "limits", proj, tr.run(X, dt, E, cl, hrr.LONG_KERNEL, hrr.long_sampling("limits", proj), proj,
                                                     *draw(2, seed=11), hrr.NT_LONG))
        # bg_hyper_ann_rom_run: tests/test_rom_hyper_ann_gpu.py
        if want("table/ann/"):
            keep_table("ann", "full-256", proj, ta.run("full-256", ta.sampling(*ones(256), proj), proj, *draw(3)))
            rows = np.setdiff1d(np.arange(96), [10, 50, 51, 70])
            mu1, mu2 = (v[[4, 5]] for v in draw(10))
            keep_table("ann", "left-out", proj, ta.run("perturbed-96", ta.sampling(rows, np.ones(len(rows)), proj), proj, mu1, mu2))
            X, Up, Us, model, _, _, dt = har.committed()
            res = rom.pod_ann_run_hyper(X, np.ones(512), *draw(4), dt, 12, Up, Us, model, har.committed_sampling(proj), p)
            keep_table("ann", "committed", proj, res)
            keep_table("ann", "limits", proj, ta.run(har.LONG, ta.long_sampling("limits", proj), proj, *draw(2, seed=11)))
        # bg_hyper_ann_rom_run_wide: tests/test_rom_hyper_ann_wide_gpu.py
        if want("table/ann_wide/"):
            keep_table("ann_wide", "full-256", proj, tw.run("wide-full-256", tw.sampling(*ones(256), proj), proj, *draw(3)))
            mu1, mu2 = (v[[4, 5]] for v in draw(10))
            keep_table("ann_wide", "left-out", proj, tw.run("wide-perturbed-96", tw.left_out_sampling(proj), proj, mu1, mu2))
            for kind in ("spread", "limits"):
                keep_table("ann_wide", kind, proj, tw.run(hw.LONG17, tw.long_sampling(kind, proj), proj, *draw(2, seed=11)))
        # bg_hyper_quad_rom_run: tests/test_rom_hyper_quad_gpu.py (at most 512 table nodes, and more)
        if want("table/quad/"):
            F = ("q", "iters", "flags", "info")
            keep_table("quad", "full-256", proj, tq.run("full-256", tq.sampling(*ones(256), proj), proj, *draw(6)), F)
            rows = tq.edge_rows("left-out")
            keep_table("quad", "left-out", proj, tq.run("perturbed-96", tq.sampling(rows, np.ones(len(rows)), proj), proj,
                                                        *draw(2, seed=11)), F)
            keep_table("quad", "limits", proj, tq.run(hq.MID, tq.limits_sampling(proj), proj, *draw(2, seed=11), nT=4), F)

name = os.path.basename(os.environ.get("BG_LIB_PATH", "product"))
if a.save:
    np.savez(a.save, **out)
    print(json.dumps({"library": name, "saved": a.save, "arrays": len(out)}))
if a.against:
    with np.load(a.against) as g:
        assert sorted(g.files) == sorted(out), "not the same workloads"
        for w in sorted({k.split(":")[0] for k in out}):
            line = {"library": name, "workload": w, "iterations": int(out[f"{w}:iters"].sum())}
            if f"{w}:nodes" in out:
                m, nodes, hit = out[f"{w}:nodes"].tolist()
                line.update(rows=m, nodes=nodes, instantiation=bool(hit))
            for k in sorted(k for k in out if k.split(":")[0] == w):
                x, y = out[k], g[k]
                line[k.split(":")[1] + "_identical"] = bool(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes())
            print(json.dumps(line))
