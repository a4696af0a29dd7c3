#!/usr/bin/env python3
"""Fixtures of the 10-type (`basic`) and 23-type (`full`) atom vocabularies, from the reference itself (utils/transforms.py;
scripts/sample_diffusion.py:192-197 falls back to `full` when the checkpoint's config has no transform section).

    python tests/golden/make_golden_vocab.py

For C in (10, 23): the reference's own ScorePosNet3D(cfg, ligand_atom_feature_dim=C) with the synthetic weights of seed 7
(stand-ins and helpers of make_golden.py), B = 4 molecules of MOSES-prior sizes, and

  forward_vocab_c{C}.npz        one forward at mixed timesteps (0 and 999 among them): pred_ligand_pos / _h / _v
  chain_vocab_c{C}_b4_s20.npz   20 steps of sample_diffusion on hash noise (synth.step_noise(n, C, ...)): the final pos and v, and
                                the pos, v, v0 and vt trajectories of every step

The batch seed is the first (from SEED0) for which init_v holds every class, every step's kNN graph has a relative margin of
at least precision.MARGIN between the k-th and (k+1)-th neighbour, and the reference's top-two Gumbel scores differ by at least
GUMBEL_GAP at every (step, atom); all three are asserted on what is written.
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
from precision import MARGIN  # noqa: E402
from tools_knn import knn_margin_rel  # noqa: E402

CLASSES = (10, 23)
B, S, SEED0 = 4, 20, 41
T_FORWARD = np.array([0, 999, 250, 640], np.int64)
GUMBEL_GAP = 1e-4


def load_reference_model(num_classes):
    """make_golden.load_reference_model with another ligand_atom_feature_dim."""
    import yaml
    G.install_stand_ins()
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        from models.molopt_score_model import ScorePosNet3D
    cfg = G.EasyDict(yaml.safe_load(open(os.path.join(G.REF, "config/training",
                                                      "dgcnn_signeddist_512_attention_residue_uniform_pos0_10_pos1.e-7_0.01_6_v001.yml"))))
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        return ScorePosNet3D(cfg.model, ligand_atom_feature_dim=num_classes), int(cfg.model.knn)


def chain_margins(bb, pos_traj, vt_traj, u, k):
    """(least relative kNN margin over the states the chain's graphs are built from, least top-two Gumbel score gap)."""
    start = np.concatenate([[0], np.cumsum(bb["counts"])])
    states = [bb["init_pos"]] + [pos_traj[s] for s in range(len(pos_traj) - 1)]
    knn = min(knn_margin_rel(x[start[i]:start[i + 1]], k) for x in states for i in range(len(bb["counts"])))
    score = -np.log(-np.log(u.astype(np.float64) + 1e-30) + 1e-30) + vt_traj.astype(np.float64)
    top = np.sort(score, -1)
    return knn, float((top[..., -1] - top[..., -2]).min())


def run_chain(model, bb, seed, C):
    n = len(bb["batch"])
    eps, u = zip(*[synth.step_noise(n, C, s, seed=seed) for s in range(S)])
    with G.fed_noise(list(eps), list(u)), contextlib.redirect_stdout(open(os.devnull, "w")):
        r = model.sample_diffusion(G.t_(bb["init_pos"]), G.t_(bb["init_v"]), G.t_(bb["batch"]), G.t_(bb["shape"]).view(B, -1),
                                   num_steps=S, center_pos_mode="none")
    st = lambda key: torch.stack([torch.as_tensor(x) for x in r[key]]).numpy()      # noqa: E731
    return r, st, np.stack(u)


def main():
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", 8)))
    for C in CLASSES:
        model, k = load_reference_model(C)
        G.synthetic_load(model, seed=7)
        for seed in range(SEED0, SEED0 + 64):
            bb = synth.synthetic_batch(B, seed=seed, num_classes=C)
            if len(np.unique(bb["init_v"])) != C:
                continue
            r, st, u = run_chain(model, bb, seed, C)
            knn, gap = chain_margins(bb, st("pos_traj"), st("vt_traj"), u, k)
            print(f"C = {C} seed {seed}: N = {len(bb['batch'])}, kNN margin {knn:.3e}, Gumbel gap {gap:.3e}", flush=True)
            if knn >= MARGIN and gap >= GUMBEL_GAP:
                break
        else:
            raise SystemExit(f"no batch seed found for C = {C}")
        assert set(bb["init_v"].tolist()) == set(range(C)) and knn >= MARGIN and gap >= GUMBEL_GAP
        np.savez_compressed(
            os.path.join(HERE, f"chain_vocab_c{C}_b4_s20.npz"), B=B, S=S, seed=seed, num_classes=C, knn_margin=knn, gumbel_gap=gap,
            pos=r["pos"].numpy(), v=r["v"].numpy(), pos_traj=st("pos_traj"), v_traj=st("v_traj").astype(np.int8),
            v0_traj=st("v0_traj"), vt_traj=st("vt_traj"))
        with torch.no_grad():
            out = model(G.t_(bb["init_pos"]), G.t_(bb["init_v"]), G.t_(bb["batch"]), G.t_(bb["shape"]), time_step=G.t_(T_FORWARD))
        np.savez_compressed(os.path.join(HERE, f"forward_vocab_c{C}.npz"), B=B, seed=seed, num_classes=C, t=T_FORWARD,
                            **{key: out[key].numpy() for key in ("pred_ligand_pos", "pred_ligand_h", "pred_ligand_v")})


if __name__ == "__main__":
    main()
