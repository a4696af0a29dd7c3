#!/usr/bin/env python3
"""Throughput of the shipped guided workload over many shape conditions: 16 conditions x 50 samples, 512-point clouds, radius 0.2,
1000 steps guided while t > 300, device Philox noise, synthetic weights and shapes, atom counts from the MOSES prior.

  baseline   one call of sample_diffusion_ligand(batch_size = 50) per condition, one after the other (all that a single cloud per
             chain allows)
  multi      sample_diffusion_ligand_multi at each --batch-sizes value (256: four chains; 800: one chain)

The runs alternate --reps times in one process (baseline, multi..., baseline, ...); every figure is wall time around the whole
call, trajectories delivered to the host as the drivers do, after a warm-up of every shape.  Prints one JSON line per run and a
summary line (median and spread of molecules/s per variant).

    python tools/guided_multi_bench.py [--conditions 16] [--samples 50] [--steps 1000] [--grad-step 300] [--batch-sizes 256,800]

Kernel cost (a process of its own, without counters):
    rocprofv3 --kernel-trace --stats -- python tools/guided_multi_bench.py --kernels single       # pc_guidance_kernel, tuple form
    rocprofv3 --kernel-trace --stats -- python tools/guided_multi_bench.py --kernels g16          # pc_guidance_kernel, 16 groups
runs B = 256 chains of --kernel-steps guided steps with one cloud (tuple form: a set of one group, so "single" and "g1" run the
same kernel), one group over the batch as a list, or 16 groups of 16.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from util import hip_model, synth, T  # noqa: E402
from shapemol_amd.sampling import sample_diffusion_ligand, sample_diffusion_ligand_multi  # noqa: E402

DEV = "cuda:0"


def conditions(n, points=512, radius=0.2):
    shapes = synth.hash_normal((n, 32, 3), 103, 41)
    return [(shapes[c], ((synth.hash_normal((points, 3), 320 + c, 5) * 1.2).astype(np.float64), None, radius)) for c in range(n)]


def prior_func():
    nums, p = synth.moses_atom_prior()
    return lambda n: np.random.choice(nums, n, p=p).tolist()


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def kernel_runs(m, which, steps):
    B = 256
    bb = synth.synthetic_batch(B, seed=11)
    args = (T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1))
    conds = conditions(16)
    forms = {"single": conds[0][1], "g1": [conds[0][1] + (B,)], "g16": [c[1] + (B // 16,) for c in conds]}
    for name in which:
        quiet(m.sample_diffusion, *args, num_steps=steps, center_pos_mode="none", return_traj=False, seed=3,
              use_pointcloud_data=forms[name], grad_step=0)
        torch.cuda.synchronize()
        print(json.dumps(dict(kernel_run=name, B=B, atoms=len(bb["batch"]), guided_steps=steps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conditions", type=int, default=16)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--grad-step", type=int, default=300)
    ap.add_argument("--batch-sizes", default="256,800")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels", default="")
    ap.add_argument("--kernel-steps", type=int, default=200)
    a = ap.parse_args()
    m = hip_model()
    if a.kernels:
        kernel_runs(m, a.kernels.split(","), a.kernel_steps)
        return
    conds = conditions(a.conditions)
    total = a.conditions * a.samples
    common = dict(num_steps=a.steps, sample_func=prior_func(), sample_num_atoms="size", grad_step=a.grad_step)

    def baseline():
        for c, (shape, pc) in enumerate(conds):
            sample_diffusion_ligand(m, shape, a.samples, batch_size=a.samples, use_pointcloud_data=pc, seed=100 + c, **common)

    variants = {"baseline_per_condition_b%d" % a.samples: baseline}
    for bs in [int(x) for x in a.batch_sizes.split(",")]:
        variants["multi_b%d" % bs] = lambda bs=bs: sample_diffusion_ligand_multi(m, conds, a.samples, batch_size=bs, seed=100, **common)
    rates = {k: [] for k in variants}
    for rep in range(-1, a.reps):                  # rep -1: warm-up of every variant (captures, workspaces, pinned buffers)
        for name, fn in variants.items():
            np.random.seed(7)
            torch.cuda.synchronize()
            t0 = time.time()
            quiet(fn)
            torch.cuda.synchronize()
            dt = time.time() - t0
            if rep >= 0:
                rates[name].append(total / dt)
            print(json.dumps(dict(run=name, rep=rep, seconds=round(dt, 3), mols_per_s=round(total / dt, 1))), flush=True)
    base = float(np.median(next(iter(rates.values()))))
    print(json.dumps({"conditions": a.conditions, "samples": a.samples, "steps": a.steps, "grad_step": a.grad_step,
                      "summary": {k: dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1),
                                          x_baseline=round(float(np.median(v)) / base, 2)) for k, v in rates.items()}}))


if __name__ == "__main__":
    main()
