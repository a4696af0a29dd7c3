#!/usr/bin/env python3
"""Throughput of classifier-free guidance over many shape conditions: 16 conditions x 50 samples, dynamic_threshold (p = 0.995),
per-condition strengths and boxes, model.eval(), 100 steps, device Philox noise, synthetic weights and shapes, atom counts from
the MOSES prior.

  baseline   one call of sample_diffusion_ligand(batch_size = 50) per condition, one after the other (all that the scalar form
             allows: one strength, one statistic and one box per chain)
  multi      sample_diffusion_ligand_multi at each --batch-sizes value (256: four chains; 800: one chain), the conditions as
             groups of each chain

The runs alternate --reps times in one process after a warm-up of every variant; every figure is wall time around the whole
call.  Prints one JSON line per run and a summary line (median and spread of molecules/s per variant).

    python tools/cfg_groups_bench.py [--conditions 16] [--samples 50] [--steps 100] [--batch-sizes 256,800]

Cost of the statistic stage (a process of its own, without counters):
    rocprofv3 --kernel-trace --stats -- python tools/cfg_groups_bench.py --kernels whole     # scalar form: the whole-batch stage
    rocprofv3 --kernel-trace --stats -- python tools/cfg_groups_bench.py --kernels g1        # list form, one group
    rocprofv3 --kernel-trace --stats -- python tools/cfg_groups_bench.py --kernels g16       # list form, 16 groups of 16
runs B = 256 chains of --kernel-steps steps; the stage is cfg_hist_kernel<0..2> + cfg_finalize_kernel.
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
CFG = dict(threshold_type="dynamic_threshold", threshold_args={"p": 0.995})


def eval_model():
    m = hip_model(cond_mask_prob=0.1)
    run = synth.running_stats(m.dims.L, m.dims.heads, 23)
    sd = m.state_dict()
    sd.update({k: torch.from_numpy(v).to(sd[k].device) for k, v in run.items()})
    m.load_state_dict(sd)
    return m.eval()


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def kernel_runs(m, which, steps):
    B = 256
    bb = synth.synthetic_batch(B, seed=11)
    args = (T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1))
    forms = {"whole": 0.7, "g1": [(0.7, B)], "g16": [(0.5 + 0.1 * g, B // 16) for g in range(16)]}
    for name in which:
        quiet(m.sample_diffusion, *args, num_steps=steps, center_pos_mode="none", return_traj=False, seed=3, guide_stren=forms[name],
              bounds=np.array([[-3.0, 3.0]] * 3), **CFG)
        torch.cuda.synchronize()
        print(json.dumps(dict(kernel_run=name, B=B, atoms=len(bb["batch"]), steps=steps)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conditions", type=int, default=16)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch-sizes", default="256,800")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels", default="")
    ap.add_argument("--kernel-steps", type=int, default=100)
    a = ap.parse_args()
    m = eval_model()
    if a.kernels:
        kernel_runs(m, a.kernels.split(","), a.kernel_steps)
        return
    shapes = synth.hash_normal((a.conditions, 32, 3), 103, 41)
    conds = [(shapes[c], None) for c in range(a.conditions)]
    strens = [0.5 + 0.1 * c for c in range(a.conditions)]
    boxes = [np.array([[-3.0 - 0.1 * c, 3.0 + 0.1 * c]] * 3) for c in range(a.conditions)]
    total = a.conditions * a.samples
    nums, p = synth.moses_atom_prior()
    common = dict(num_steps=a.steps, sample_func=lambda n: np.random.choice(nums, n, p=p).tolist(), sample_num_atoms="size", **CFG)

    def baseline():
        for c, (shape, _) in enumerate(conds):
            sample_diffusion_ligand(m, shape, a.samples, batch_size=a.samples, guide_stren=strens[c], bounds=boxes[c], seed=100 + c, **common)

    variants = {"baseline_per_condition_b%d" % a.samples: baseline}
    for bs in [int(x) for x in a.batch_sizes.split(",")]:
        variants["multi_b%d" % bs] = lambda bs=bs: sample_diffusion_ligand_multi(m, conds, a.samples, batch_size=bs, seed=100, guide_stren=strens,
                                                                                 bounds=boxes, **common)
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
    print(json.dumps({"conditions": a.conditions, "samples": a.samples, "steps": a.steps, "threshold": CFG,
                      "summary": {k: dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1),
                                          x_baseline=round(float(np.median(v)) / base, 2)) for k, v in rates.items()}}))


if __name__ == "__main__":
    main()
