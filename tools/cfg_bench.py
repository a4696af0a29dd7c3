#!/usr/bin/env python3
"""Cost of classifier-free guidance inside the sampling chain: wall time per reverse step (captured graph, no trajectories) of
an unguided chain and of CFG chains with each threshold type, at B = 256 and B = 1024 (synthetic weights, cond_mask_prob =
0.1, synthetic batches, a box that clamps).  Kernel times of the statistic stage (cfg_partial / cfg_hist / cfg_finalize):
run it in a process of its own under `rocprofv3 --kernel-trace --stats -- python tools/cfg_bench.py --types dynamic_threshold`.

    python tools/cfg_bench.py [--steps 100] [--batches 256,1024] [--types none,reference_threshold,dynamic_threshold,rescale]
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
from util import hip_model, synth, T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--types", default="none,reference_threshold,dynamic_threshold,rescale")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    m = hip_model(cond_mask_prob=0.1)
    dev = "cuda:0"
    box = np.array([[-3.0, 3.5], [-2.5, 3.0], [-3.5, 2.5]])
    runs = {"unguided": None}
    runs.update({f"cfg_{t}": (None if t == "none" else t) for t in a.types.split(",")})
    out = []
    for B in [int(b) for b in a.batches.split(",")]:
        bb = synth.synthetic_batch(B, seed=11)
        args = (T(bb["init_pos"], dev), T(bb["init_v"], dev), T(bb["batch"], dev), T(bb["shape"], dev).view(B, -1))
        for name, ttype in runs.items():
            kw = dict(num_steps=a.steps, center_pos_mode="none", return_traj=False, seed=3)
            if name != "unguided":
                kw.update(guide_stren=1.5, threshold_type=ttype, threshold_args={}, bounds=box)
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
            rec = dict(B=B, atoms=len(bb["batch"]), run=name, ms_per_step=round(best, 4))
            out.append(rec)
            print(json.dumps(rec), flush=True)
    base = {r["B"]: r["ms_per_step"] for r in out if r["run"] == "unguided"}
    for r in out:
        r["x_unguided"] = round(r["ms_per_step"] / base[r["B"]], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
