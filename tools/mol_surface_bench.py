#!/usr/bin/env python
"""Molecular surfaces (shapemol_amd.mol_surface): molecules per second for a batch of MOSES-sized synthetic molecules at grid
spacings 0.5 and 0.25 with the sampling script's probe radius 0.5, the split over the six kernel stages (HIP events inside
shapemol_msurf_build), and -- for context only, no gate -- the numpy oracle of the same rule on a few of the molecules.

    python tools/mol_surface_bench.py [--mols 256] [--reps 5] [--out profiles/mol_surface/bench.json]
    python tools/mol_surface_bench.py --oracle-profile profiles/mol_surface/oracle_convergence.txt      (host only; also
                                                        writes skimage_comparison.txt beside it)
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def molecules(n, seed=2021):
    from shapemol_amd import synth
    from shapemol_amd.mol_surface import radii_of
    bb = synth.synthetic_batch(n, seed=seed)
    o = np.concatenate([[0], np.cumsum(bb["counts"])])
    pos = bb["init_pos"].astype(np.float64) * 1.5          # unit normals are denser than a molecule; 1.5 A spread: ~8 A across
    return [(pos[o[i]:o[i + 1]], radii_of(atom_types=bb["init_v"][o[i]:o[i + 1]])) for i in range(n)]


def oracle_profile(path):
    import mol_surface_oracle as O
    lines = ["Marching tetrahedra (Kuhn split) of the numpy oracle, one sphere r = 1.7 at (0.1, 0.2, 0.3), p = 0:",
             "relative error of the enclosed volume and of the area against 4/3 pi r^3 and 4 pi r^2.",
             "", "      h   volume error     area error"]
    for h, ev, ea in O.convergence_table():
        lines.append(f"{h:7.3f}   {ev:12.4e}   {ea:12.4e}")
    lines += ["", "Both errors fall by about 4 per halving of h (second order), as tests/test_mol_surface_cpu.py asserts (monotone)."]
    sk = ["Comparison with skimage.measure.marching_cubes on the oracle's own node field g",
          "(tests/test_mol_surface_cpu.py::test_against_skimage_marching_cubes).",
          "",
          "NOT MEASURED: skimage is not installed where these figures were taken, and the test has not run anywhere yet.",
          "Until it has, the test's margin is reasoned, not measured: 4 e(h), with e(h) the oracle's own relative error on the",
          "sphere r = 1.7 at the fixture's spacing -- each triangulation lies within about e(h) of the smooth level set (both",
          "interpolate g linearly along grid edges, order h^2), so two of them differ by at most 2 e(h), doubled for surfaces more",
          "curved than the sphere.  Volume and area each use their own e(h):",
          "", "fixture                     h    margin volume   margin area"]
    for name, (_, p, h) in O.SKIMAGE_FIXTURES.items():
        (_, ev, ea), = O.convergence_table((h,))
        sk.append(f"{name:25s} {h:5.2f}   {4 * ev:10.4f}   {4 * ea:10.4f}")
    sk += ["", "To be replaced by 2 x the difference measured on these three fixtures once skimage can be run (two triangulations of",
           "one field differ at order h^2)."]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(os.path.join(os.path.dirname(os.path.abspath(path)), "skimage_comparison.txt"), "w").write("\n".join(sk) + "\n")
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--probe", type=float, default=0.5)
    ap.add_argument("--cpu-mols", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--oracle-profile", default=None)
    a = ap.parse_args()
    if a.oracle_profile:
        return oracle_profile(a.oracle_profile)
    import torch
    from shapemol_amd import _lib
    from shapemol_amd.mol_surface import get_mesh_batch
    import mol_surface_oracle as O
    mols = molecules(a.mols)
    res = dict(mols=a.mols, atoms=int(sum(len(c) for c, _ in mols)), probe_radius=a.probe, reps=a.reps,
               library_sha256=hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(), device=torch.cuda.get_device_name(0), runs=[])
    for h in (0.5, 0.25):
        get_mesh_batch(mols, a.probe, 1.0, h, device="cuda:0")                   # warm-up: workspaces grow here
        wall, stages = [], []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            meshes, info = get_mesh_batch(mols, a.probe, 1.0, h, device="cuda:0", details=True)
            wall.append(time.perf_counter() - t0)
            stages.append(info["stage_ms"])
        kernels_ms = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
        t0 = time.perf_counter()
        for c, r in mols[:a.cpu_mols]:
            O.get_mesh(c, r, a.probe, h)
        cpu = (time.perf_counter() - t0) / a.cpu_mols
        run = dict(spacing=h, nodes=int(info["dims"].astype(np.int64).prod(1).sum()), vertices=int(sum(len(v) for v, _ in meshes)),
                   faces=int(sum(len(f) for _, f in meshes)), wall_s_median=float(np.median(wall)),
                   mols_per_s_wall=a.mols / float(np.median(wall)), stage_ms_median=kernels_ms,
                   mols_per_s_kernels=a.mols / (sum(kernels_ms.values()) / 1e3), numpy_oracle_s_per_mol=cpu, numpy_oracle_mols_per_s=1.0 / cpu)
        res["runs"].append(run)
        print(json.dumps(run))
    res["note"] = ("wall includes the host plan, the upload, the copy of the meshes to host numpy arrays and the copy of the node field "
                   "(details=True); the stage 'scan' includes the host round trip that sizes the outputs.  The numpy oracle is context, not a gate.")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
