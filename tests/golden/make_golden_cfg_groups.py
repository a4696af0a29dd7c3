#!/usr/bin/env python3
"""Classifier-free guidance with one threshold statistic and one box per GROUP of molecules, from the reference itself.

    python tests/golden/make_golden_cfg_groups.py

The reference's ``sample_diffusion`` (with the keyword adaptation of make_golden_cfg.py) runs one chain of B = 6 molecules in
groups of 2 / 3 / 1, train mode, one strength.  Its module function ``threshold_CFG`` is wrapped: the wrapper calls the REAL
function once per group, with that group's slice of the two tensors and that group's box, and concatenates the results --
what the reference computes for a group when the group is a batch of its own.  The wrapper holds the full (B,3,2) bounds,
since the sampling loop hands ``threshold_CFG`` only ``bounds[0]``; a group's box is the row of its first molecule.

Writes chain_cfg_groups_<type>_b6_s20.npz for the four threshold types (strengths and p of make_golden_cfg.py): 20 steps from
t = 999 on the hash noise of the other chain fixtures.  The boxes of groups 0 and 2 are tight enough to clamp atoms, group
1's is wide; the script asserts the clamp counts and that the three groups' statistics differ.  Stored: the final state,
v_traj at every step, the other trajectories at TRAJ_STEPS, and the inputs and outputs of the wrapped calls of the first
step (positions, then logits; whole tensors, the groups' atom offsets beside).
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
from shapemol_amd import synth  # noqa: E402

B, S, SEED = 6, 20, 13
GROUPS = (2, 3, 1)
TRAJ_STEPS = np.array([0, 1, 19])
CHAINS = (("none", None, 0.5, None), ("reference_threshold", "reference_threshold", 2.0, 0.9),
          ("dynamic_threshold", "dynamic_threshold", 0.5, 0.995), ("rescale", "rescale", 2.0, 0.7))
BOXES = (np.array([[-2.0, 2.5], [-1.5, 2.0], [-2.5, 1.5]]), np.array([[-50.0, 50.0]] * 3),
         np.array([[-1.0, 1.5], [-2.0, 1.0], [-1.5, 2.0]]))


def group_statistic(x, cond, ttype, p):
    if ttype == "reference_threshold":
        return float(cond.abs().max())
    if ttype == "dynamic_threshold":
        return float(torch.quantile(x.reshape(-1), p))
    return float(cond.std() / x.std())


def main():
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", 8)))
    model, _ = G.load_reference_model(overrides={"cond_mask_prob": 0.1})
    G.synthetic_load(model, seed=7)
    import models.molopt_score_model as R

    class KeywordAdapted(R.ScorePosNet3D):
        def forward(self, *a, init_ligand_pos=None, init_ligand_v=None, **k):
            if init_ligand_pos is not None:
                k["ligand_pos_perturbed"], k["ligand_v_perturbed"] = init_ligand_pos, init_ligand_v
            return super().forward(*a, **k)
    model.__class__ = KeywordAdapted

    bb = synth.synthetic_batch(B, seed=SEED)
    n = len(bb["batch"])
    mol_off = np.concatenate([[0], np.cumsum(GROUPS)])
    atom_off = np.searchsorted(bb["batch"], mol_off)
    bounds = np.concatenate([np.stack([BOXES[g]] * GROUPS[g]) for g in range(len(GROUPS))])
    full_bounds = torch.from_numpy(bounds).float()

    calls, stats = [], []
    real_threshold = R.threshold_CFG

    def per_group_threshold(x0, x0_cond, threshold_type, threshold_args, bounds=None):
        outs = []
        for g in range(len(GROUPS)):
            sl = slice(int(atom_off[g]), int(atom_off[g + 1]))
            box = None if bounds is None else full_bounds[int(mol_off[g])]
            outs.append(real_threshold(x0[sl], x0_cond[sl], threshold_type, threshold_args, bounds=box))
            if len(calls) < 2 and threshold_type is not None:
                stats.append(group_statistic(x0[sl], x0_cond[sl], threshold_type, threshold_args["p"]))
        out = torch.cat(outs)
        if len(calls) < 2:           # the first step: positions, then logits
            calls.append((x0.numpy().copy(), x0_cond.numpy().copy(), out.numpy().copy()))
        return out
    R.threshold_CFG = per_group_threshold

    eps, u = zip(*[synth.step_noise(n, 15, s, seed=SEED) for s in range(S)])
    for tag, ttype, w, p in CHAINS:
        calls.clear(), stats.clear()
        targs = {} if p is None else {"p": p}
        with G.fed_noise(list(eps), list(u)), contextlib.redirect_stdout(open(os.devnull, "w")):
            r = model.sample_diffusion(G.t_(bb["init_pos"]), G.t_(bb["init_v"]), G.t_(bb["batch"]), G.t_(bb["shape"]).view(B, -1),
                                       threshold_type=ttype, threshold_args=targs, num_steps=S, center_pos_mode="none",
                                       guide_stren=w, bounds=full_bounds)
        st = lambda k: torch.stack([torch.as_tensor(x) for x in r[k]]).numpy()      # noqa: E731
        pos_out = calls[0][2]
        clamped = []
        for g in range(len(GROUPS)):
            o, bx = pos_out[atom_off[g]:atom_off[g + 1]], BOXES[g].astype(np.float32)
            clamped.append(int(((o == bx[:, 0]) | (o == bx[:, 1])).sum()))
        print(tag, "clamped per group in the first step:", clamped, "statistics:", stats, flush=True)
        assert clamped[0] > 0 and clamped[2] > 0 and clamped[1] == 0, clamped
        if ttype is not None:       # positions of the three groups, then logits
            assert len(set(stats[:3])) == 3 and len(set(stats[3:])) == 3, stats
        np.savez_compressed(
            os.path.join(HERE, f"chain_cfg_groups_{tag}_b6_s20.npz"), B=B, S=S, seed=SEED, threshold_type=tag, guide_stren=w,
            p=np.nan if p is None else p, bounds=bounds, groups=np.array(GROUPS), atom_off=atom_off, traj_steps=TRAJ_STEPS,
            pos=r["pos"].numpy(), v=r["v"].numpy(), pos_traj=st("pos_traj")[TRAJ_STEPS], pos_cond_traj=st("pos_cond_traj")[TRAJ_STEPS],
            pos_uncond_traj=st("pos_uncond_traj")[TRAJ_STEPS], v_traj=st("v_traj").astype(np.int8),
            v0_traj=st("v0_traj")[TRAJ_STEPS], vt_traj=st("vt_traj")[TRAJ_STEPS],
            v_cond_traj=st("v_cond_traj")[TRAJ_STEPS], v_uncond_traj=st("v_uncond_traj")[TRAJ_STEPS],
            call_x=np.concatenate([c[0].reshape(-1) for c in calls]), call_cond=np.concatenate([c[1].reshape(-1) for c in calls]),
            call_out=np.concatenate([c[2].reshape(-1) for c in calls]), call_sizes=np.array([c[0].size for c in calls]),
            call_cols=np.array([c[0].shape[1] for c in calls]))
    R.threshold_CFG = real_threshold


if __name__ == "__main__":
    main()
