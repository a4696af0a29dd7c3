#!/usr/bin/env python3
"""Fixtures of point-cloud shape guidance with one cloud per GROUP of molecules, from the reference itself.

    python tests/golden/make_golden_guided_multi.py

The reference guides a whole batch towards one cloud (models/molopt_score_model.py:583-586, 699-740).  Here a batch of B = 6
molecules is cut into G = 3 contiguous groups of 1 / 3 / 2 molecules, each with its own cloud (64 / 512 / 300 points, different
centres) and radius (0.2 / 0.3 / 0.2).  Everything is the reference's own ``sample_diffusion`` and its own
``pointcloud_shape_guidance`` on the CPU.  The ONE adaptation: the module-level name ``pointcloud_shape_guidance`` that the loop
calls is bound to a dispatcher which calls the reference's real function once per group, on that group's atom slice with that
group's ``(cloud, kdtree, radius)``, and writes the slices back.  The uniform draws are recorded by one ``GuideRecorder``
(make_golden_r2.py: the KD-tree / ``np.random.random`` stand-in) per group and scattered into one table per
(step, iteration, batch-global atom).  Weights: synthetic, seed 7; noise: the hash noise of the other chain fixtures.

Writes chain_guided_multi_b6_s20.npz (all three groups guided) and chain_guided_multi_b6_s20_gap.npz (the middle group has no
cloud): 20 reverse steps from t = 999, guided while t > 990.  Stored: the final state, v_traj at every step, pos_traj and
pos_cond_traj at TRAJ_STEPS, and the dispatcher's input and output of the first step (``fn_pred`` / ``fn_out``).

Asserted here and again by tests/test_guided_multi_cpu.py: in every guided step every group that has a cloud moves at least one
atom, and at least one atom somewhere needs two or more pulls.
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
from make_golden_r2 import GuideRecorder  # noqa: E402
from shapemol_amd import synth  # noqa: E402

B, S, SEED, GRAD_STEP = 6, 20, 31, 990
GROUP_MOLS = (1, 3, 2)
CLOUD_POINTS = (64, 512, 300)
CLOUD_CENTRES = ((0.4, -0.2, 0.1), (-0.3, 0.3, 0.0), (0.0, 0.2, -0.4))
CLOUD_SCALES = (0.9, 1.2, 1.0)
RADII = (0.2, 0.3, 0.2)
TRAJ_STEPS = np.array([0, 1, 8, 9, 19])


def clouds():
    return [(synth.hash_normal((p, 3), 310 + g, 5) * s + np.array(c)).astype(np.float64)
            for g, (p, c, s) in enumerate(zip(CLOUD_POINTS, CLOUD_CENTRES, CLOUD_SCALES))]


def run(model, R, bb, eps, u, cls, tag):
    """One chain; `cls[g]` is None for a group without a cloud."""
    real = R.pointcloud_shape_guidance
    counts = bb["counts"]
    mol_off = np.concatenate([[0], np.cumsum(GROUP_MOLS)])
    atom_off = np.concatenate([[0], np.cumsum(counts)])[mol_off]
    na = int(atom_off[-1])
    recs = [None if c is None else GuideRecorder(c, RADII[g], int(atom_off[g + 1] - atom_off[g])) for g, c in enumerate(cls)]
    for g, rec in enumerate(recs):
        if rec is not None:
            rec._rs = np.random.RandomState(80 + g)
    first = {}

    def dispatcher(use_pointcloud_data, pred_ligand_pos, k=3, ratio=0.2):
        if not first:
            first["pred"] = pred_ligand_pos.numpy().copy()
        real_random = np.random.random
        try:
            for g, rec in enumerate(recs):
                if rec is None:
                    continue
                np.random.random = rec.random
                lo, hi = int(atom_off[g]), int(atom_off[g + 1])
                part = pred_ligand_pos[lo:hi].clone()
                pred_ligand_pos[lo:hi] = real((cls[g], rec, RADII[g]), part, k, ratio)
        finally:
            np.random.random = real_random
        if "out" not in first:
            first["out"] = pred_ligand_pos.numpy().copy()
        return pred_ligand_pos

    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda t, *a, **k: t      # the reference hard-codes .cuda() (:738); this harness runs on the CPU
    R.pointcloud_shape_guidance = dispatcher
    try:
        with G.fed_noise(list(eps), list(u)), contextlib.redirect_stdout(open(os.devnull, "w")):
            r = model.sample_diffusion(G.t_(bb["init_pos"]), G.t_(bb["init_v"]), G.t_(bb["batch"]), G.t_(bb["shape"]).view(B, -1),
                                       num_steps=S, center_pos_mode="none", use_pointcloud_data=("per group", None, None),
                                       grad_step=GRAD_STEP)
    finally:
        R.pointcloud_shape_guidance, torch.Tensor.cuda = real, real_cuda
    guided_steps = max(len(rec.steps) for rec in recs if rec is not None)
    assert guided_steps == 999 - GRAD_STEP
    draws = np.full((S, 5, na), 0.5)
    pulls = np.zeros((guided_steps, na), dtype=np.int64)        # pulls per (step, atom): entries of the table that were drawn
    for g, rec in enumerate(recs):
        if rec is None:
            continue
        assert len(rec.steps) == guided_steps
        st = np.stack(rec.steps)
        draws[:guided_steps, :, atom_off[g]:atom_off[g + 1]] = st
        pulls[:, atom_off[g]:atom_off[g + 1]] = (st != 0.5).sum(1)
    for g, rec in enumerate(recs):
        if rec is not None:
            moved = (pulls[:, atom_off[g]:atom_off[g + 1]] > 0).sum(1)
            assert (moved > 0).all(), f"{tag}: group {g} moves no atom in some guided step: {moved}"
            print(tag, "group", g, "moved atoms per guided step", moved.tolist(), flush=True)
    assert (pulls >= 2).any(), f"{tag}: no atom needs two pulls"
    print(tag, "atoms with >= 2 pulls per step", (pulls >= 2).sum(1).tolist(), "max pulls", int(pulls.max()), flush=True)
    st = lambda k: torch.stack([torch.as_tensor(x) for x in r[k]]).numpy()      # noqa: E731
    has = np.array([c is not None for c in cls])
    np.savez_compressed(
        os.path.join(HERE, f"{tag}.npz"), B=B, S=S, seed=SEED, grad_step=GRAD_STEP, guided_steps=guided_steps,
        group_mols=np.array(GROUP_MOLS), has_cloud=has, radii=np.array(RADII),
        cloud_off=np.concatenate([[0], np.cumsum([0 if c is None else len(c) for c in cls])]),
        clouds=np.concatenate([c for c in cls if c is not None]), draws=draws, traj_steps=TRAJ_STEPS,
        pos=r["pos"].numpy(), v=r["v"].numpy(), v_traj=st("v_traj").astype(np.int8), pos_traj=st("pos_traj")[TRAJ_STEPS],
        pos_cond_traj=st("pos_cond_traj")[TRAJ_STEPS], fn_pred=first["pred"], fn_out=first["out"])


def main():
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", 8)))
    model, _ = G.load_reference_model()
    G.synthetic_load(model, seed=7)
    import models.molopt_score_model as R
    bb = synth.synthetic_batch(B, seed=SEED)
    n = len(bb["batch"])
    eps, u = zip(*[synth.step_noise(n, 15, s, seed=SEED) for s in range(S)])
    cls = clouds()
    run(model, R, bb, eps, u, cls, "chain_guided_multi_b6_s20")
    run(model, R, bb, eps, u, [cls[0], None, cls[2]], "chain_guided_multi_b6_s20_gap")


if __name__ == "__main__":
    main()
