#!/usr/bin/env python3
"""Mesh shape guidance with one mesh per group of molecules: what it costs and what packing conditions into one chain gains.

  --mode step      B = 256, every step guided by the ~5k-face fixture mesh (tests/golden/mesh_fixture.npz): wall time per reverse
                   step (captured graph, no trajectories) of the single-mesh call and of a one-group list over the batch (the same
                   kernels since the tuple form runs as a set of one group: the pair now measures the run-to-run spread),
                   alternating --reps times in one process after a warm-up of both; medians and min / max.
  --mode workload  16 mesh conditions x 50 samples, 1000 steps guided while t > 300, atom counts from the MOSES prior:
                   sample_diffusion_ligand per condition (16 chains of 50) against sample_diffusion_ligand_multi (one chain of
                   800), alternating --reps times; molecules/s.  The conditions' meshes are the fixture mesh scaled and shifted.
                   --bn eval (default): the model in evaluation mode (running batch-norm statistics), in which molecules are
                   independent and both variants compute the same molecules; --bn train: batch statistics, as the reference's
                   sampling script leaves the module (a mixed batch is then another computation than the chains of 50).
  --mode kernels   chains of --kernel-steps guided steps for `rocprofv3 --kernel-trace --stats -- python
                   tools/mesh_groups_bench.py --mode kernels --kernels NAME` (a process of its own, without counters; one NAME
                   per process keeps the variants' statistics apart): single, g1, g16 at B = 256 (one mesh as a tuple -- a set of
                   one group, the same kernels as g1 --, one group as a list, 16 groups of 16); w800 = the workload's chain, 16 groups of 50 molecules.

A chain in which a group runs out of atoms inside its mesh runs to the end with that group left unguided in such steps, and the
call then raises MeshGuidanceError instead of returning molecules.  A timing that contains such a call does not measure the
guided workload: the tool counts the calls ("mesh_errors") and the (group, step) pairs left unguided ("unguided_pairs", from the
library's per-group count) per variant, and marks the summary "valid" only when both are 0 everywhere.
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
from util import hip_model, model_cfg, synth, T  # noqa: E402
from shapemol_amd import _lib  # noqa: E402
from shapemol_amd.sampling import sample_diffusion_ligand, sample_diffusion_ligand_multi  # noqa: E402

DEV = "cuda:0"
ERRORS = [0]          # calls that raised MeshGuidanceError
PAIRS = [0]           # (group, step) pairs left unguided in them
SCALE = [0.55, 0.85]


def fixture_mesh():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "mesh_fixture.npz"))
    return fx["verts"], fx["faces"], fx["cloud"]


def conditions(n):
    """n mesh conditions: the fixture mesh (centred) scaled by --mesh-scale (0.55 .. 0.85) and shifted by a few tenths."""
    v, f, c = fixture_mesh()
    mid = 0.5 * (v.max(0) + v.min(0))
    shapes = synth.hash_normal((n, 32, 3), 103, 41)
    shift = synth.hash_normal((n, 3), 104, 41) * 0.2
    out = []
    for k in range(n):
        s = SCALE[0] + (SCALE[1] - SCALE[0]) * k / max(n - 1, 1)
        out.append((shapes[k], None, (((v - mid) * s + shift[k], f), (c - mid) * s + shift[k], None)))
    return out


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        try:
            return fn(*a, **k)
        except _lib.MeshGuidanceError as e:
            ERRORS[0] += 1
            steps = getattr(e, "group_steps", None)
            PAIRS[0] += int(steps.sum()) if steps is not None else 1          # (a single-mesh chain: the library keeps no count)


def batch_args(B):
    bb = synth.synthetic_batch(B, seed=11)
    return bb, (T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1))


def forms(B):
    v, f, c = fixture_mesh()
    conds = conditions(16)
    return {"single": ((v, f), c, None), "g1": [((v, f), c, None, B)], "g16": [cd[2] + (B // 16,) for cd in conds],
            "w800": [cd[2] + (B // 16,) for cd in conds]}


def eval_model():
    """A model in evaluation mode with non-trivial running statistics (as the tests' independence checks)."""
    import shapemol_amd
    cfg = model_cfg()
    m = shapemol_amd.ScorePosNet3D(cfg, 15)
    sdn = synth.synthetic_state_dict(cfg, seed=7)
    sdn.update(synth.running_stats(m.dims.L, m.dims.heads, 23))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=True)
    return m.to(DEV).eval()


def mode_step(m, a):
    B = 256
    bb, args = batch_args(B)
    fm = forms(B)
    kw = dict(num_steps=a.steps, center_pos_mode="none", return_traj=False, seed=3, grad_step=0)
    times = {"single": [], "g1": []}
    for rep in range(-1, a.reps):
        for name in times:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            quiet(m.sample_diffusion, *args, use_mesh_data=fm[name], **kw)
            e1.record()
            torch.cuda.synchronize()
            if rep >= 0:
                times[name].append(e0.elapsed_time(e1) / a.steps)
    print(json.dumps({"mode": "step", "B": B, "atoms": len(bb["batch"]), "steps": a.steps, "reps": a.reps, "mesh_errors": ERRORS[0],
                      "ms_per_step": {k: dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))
                                      for k, v in times.items()}}))


def mode_kernels(m, a):
    for name in a.kernels.split(","):
        B = 800 if name == "w800" else 256
        bb, args = batch_args(B)
        fm = forms(B)
        quiet(m.sample_diffusion, *args, num_steps=a.kernel_steps, center_pos_mode="none", return_traj=False, seed=3,
              use_mesh_data=fm[name], grad_step=0)
        torch.cuda.synchronize()
        print(json.dumps(dict(kernel_run=name, B=B, atoms=len(bb["batch"]), guided_steps=a.kernel_steps, bn=a.bn, mesh_errors=ERRORS[0],
                              unguided_pairs=PAIRS[0])), flush=True)


def mode_workload(m, a):
    conds = conditions(a.conditions)
    total = a.conditions * a.samples
    nums, p = synth.moses_atom_prior()
    common = dict(num_steps=a.steps, sample_func=lambda n: np.random.choice(nums, n, p=p).tolist(), sample_num_atoms="size",
                  grad_step=a.grad_step)

    def baseline():
        for c, (shape, _pc, md) in enumerate(conds):
            quiet(sample_diffusion_ligand, m, shape, a.samples, batch_size=a.samples, use_mesh_data=md, seed=100 + c, **common)

    variants = {"per_condition_b%d" % a.samples: baseline,
                "multi_b%d" % total: lambda: quiet(sample_diffusion_ligand_multi, m, conds, a.samples, batch_size=total, seed=100, **common)}
    rates = {k: [] for k in variants}
    flagged = {k: [0, 0] for k in variants}        # calls that raised, (group, step) pairs left unguided
    for rep in range(-1, a.reps):                  # rep -1: warm-up of every variant (captures, workspaces, pinned buffers)
        for name, fn in variants.items():
            np.random.seed(7)
            e0, p0 = ERRORS[0], PAIRS[0]
            torch.cuda.synchronize()
            t0 = time.time()
            fn()
            torch.cuda.synchronize()
            dt = time.time() - t0
            if rep >= 0:
                rates[name].append(total / dt)
            flagged[name][0] += ERRORS[0] - e0
            flagged[name][1] += PAIRS[0] - p0
            print(json.dumps(dict(run=name, rep=rep, seconds=round(dt, 3), mols_per_s=round(total / dt, 1), mesh_errors=ERRORS[0] - e0,
                                  unguided_pairs=PAIRS[0] - p0)), flush=True)
    base = float(np.median(next(iter(rates.values()))))
    print(json.dumps({"mode": "workload", "conditions": a.conditions, "samples": a.samples, "steps": a.steps, "grad_step": a.grad_step,
                      "bn": a.bn, "guided_pairs_per_run": a.conditions * max(a.steps - 1 - a.grad_step, 0), "mesh_errors": ERRORS[0],
                      "unguided_pairs": PAIRS[0], "valid": ERRORS[0] == 0,
                      "summary": {k: dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1),
                                          x_baseline=round(float(np.median(v)) / base, 2), mesh_errors=flagged[k][0],
                                          unguided_pairs=flagged[k][1]) for k, v in rates.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("step", "workload", "kernels"), default="step")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--conditions", type=int, default=16)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--grad-step", type=int, default=300)
    ap.add_argument("--kernels", default="single,g1,g16")
    ap.add_argument("--kernel-steps", type=int, default=100)
    ap.add_argument("--bn", choices=("eval", "train"), default=None, help="batch-norm mode (default: eval for workload, train otherwise)")
    ap.add_argument("--mesh-scale", default="0.55,0.85", help="workload: the fixture mesh is scaled from lo to hi over the conditions")
    a = ap.parse_args()
    if a.steps is None:
        a.steps = 100 if a.mode == "step" else 1000
    if a.bn is None:
        a.bn = "eval" if a.mode == "workload" else "train"
    SCALE[:] = [float(x) for x in a.mesh_scale.split(",")]
    m = eval_model() if a.bn == "eval" else hip_model()
    {"step": mode_step, "workload": mode_workload, "kernels": mode_kernels}[a.mode](m, a)


if __name__ == "__main__":
    main()
