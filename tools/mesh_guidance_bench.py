#!/usr/bin/env python3
"""Cost of mesh shape guidance inside the sampling chain: wall time per reverse step (captured graph, no trajectories) of an
unguided chain, a chain guided by the fixture mesh (tests/golden/mesh_fixture.npz, ~5k faces) and one guided by a finer
~10k-face mesh of the same shape, at B = 256 and B = 1024 (synthetic weights and batches).  Every step of the timed chains
is guided (grad_step = 0).  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/mesh_guidance_bench.py`.

    python tools/mesh_guidance_bench.py [--steps 100] [--batches 256,1024]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_oracle as M  # noqa: E402
from util import hip_model, synth, T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    fx = np.load(os.path.join(ROOT, "tests", "golden", "mesh_fixture.npz"))
    fine_v, fine_f = M.sphere_union_mesh(M.FIXTURE_CENTRES, M.FIXTURE_RADII, 0.35, seed=1)
    meshes = {"none": None, f"fixture_{len(fx['faces'])}f": ((fx["verts"], fx["faces"]), fx["cloud"], None),
              f"fine_{len(fine_f)}f": ((fine_v, fine_f), M.sample_surface(fine_v, fine_f, 512, seed=2), None)}
    m = hip_model()
    dev = "cuda:0"
    out = []
    for B in [int(b) for b in a.batches.split(",")]:
        bb = synth.synthetic_batch(B, seed=11)
        args = (T(bb["init_pos"], dev), T(bb["init_v"], dev), T(bb["batch"], dev), T(bb["shape"], dev).view(B, -1))
        for name, data in meshes.items():
            kw = dict(num_steps=a.steps, center_pos_mode="none", return_traj=False, seed=3, use_mesh_data=data, grad_step=0)
            m.sample_diffusion(*args, **kw)                  # capture + warm-up
            best = None
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                m.sample_diffusion(*args, **kw)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / a.steps
                best = ms if best is None else min(best, ms)
            rec = dict(B=B, atoms=len(bb["batch"]), mesh=name, ms_per_step=round(best, 4))
            out.append(rec)
            print(json.dumps(rec), flush=True)
    base = {r["B"]: r["ms_per_step"] for r in out if r["mesh"] == "none"}
    for r in out:
        r["overhead_pct"] = round(100.0 * (r["ms_per_step"] / base[r["B"]] - 1.0), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
