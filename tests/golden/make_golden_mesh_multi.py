#!/usr/bin/env python3
"""Fixtures of mesh shape guidance with one mesh per GROUP of molecules, from the reference itself.

    python tests/golden/make_golden_mesh_multi.py

The reference guides a whole batch with one mesh (models/molopt_score_model.py:571-580, 742-775).  Here a batch of B = 6
molecules is cut into G = 3 contiguous groups of 1 / 3 / 2 molecules, each with its own union-of-spheres mesh
(tests/mesh_oracle.py; different centres, sizes and face counts) and its own cloud sampled from that mesh's surface.  Everything
is the reference's own ``sample_diffusion`` and its own ``mesh_shape_guidance`` on the CPU with the real sklearn KD-trees.  The
ONE adaptation, as in make_golden_guided_multi.py: the module-level name ``mesh_shape_guidance`` that the loop calls is bound to
a dispatcher which calls the reference's real function once per group, on that group's atom slice with that group's
``(mesh, cloud, kdtree)``, and writes the slices back.  Each group has its own recorder (make_golden_mesh.py's MeshRecorder: the
mesh / ``np.random.random`` stand-in that answers ``.contains`` with the ray parity after asserting, on every query, that it
equals the winding number); the draws are scattered into one table per (step, iteration, batch-global atom).  Weights:
synthetic, seed 7; noise: the hash noise of the other chain fixtures.

Writes mesh_guidance_multi_fn.npz (the three meshes and clouds, and the dispatcher on scattered atoms),
chain_mesh_guided_multi_b6_s20.npz (all three groups guided) and chain_mesh_guided_multi_b6_s20_gap.npz (the middle group has
no mesh): 20 reverse steps from t = 999, guided while t > 990.  Stored per chain: the final state, v_traj at every step,
pos_traj and pos_cond_traj at TRAJ_STEPS, the dispatcher's input and output of the first step (``fn_pred`` / ``fn_out``), and
per guided step the dispatcher's input (``guided_pred``: pos_cond_traj holds the guided prediction, as in the reference), the
pulls of every atom, the atoms never accepted and every group's number of within-atoms.

Asserted here and again by tests/test_mesh_multi_cpu.py, for each of the three files: in every guided step every group that has
a mesh pulls at least one atom, some atom needs two or more pulls, some atom is never accepted, every group always has >= 3
within-atoms; the 3rd and 4th nearest within-atoms of a pulled atom never tie (MeshRecorder.random).
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
import mesh_oracle as M  # noqa: E402
from make_golden_mesh import MeshRecorder  # noqa: E402
from shapemol_amd import synth  # noqa: E402

B, S, SEED, GRAD_STEP = 6, 20, 31, 990
GROUP_MOLS = (1, 3, 2)
TRAJ_STEPS = np.array([0, 1, 8, 9, 19])
# three non-convex unions of spheres (C shapes: the mean of three within-atoms of different arms can lie in the gap)
MESHES = (
    dict(centres=[(-1.6, -0.9, 0.5), (-0.4, -1.3, 0.5), (0.8, -0.9, 0.5), (1.0, 0.4, 0.5), (-1.8, 0.4, 0.5)],
         radii=[1.3, 1.3, 1.3, 1.2, 1.2], h=0.85, cloud=200),
    dict(centres=[(-1.5, 1.2, -0.4), (-1.7, -0.2, -0.4), (-0.9, -1.4, -0.4), (0.5, -1.6, -0.4), (1.6, -0.6, -0.4), (1.5, 0.9, -0.4),
                  (0.0, 0.1, -1.6)],
         radii=[1.4, 1.4, 1.4, 1.4, 1.4, 1.3, 1.0], h=0.6, cloud=512),
    dict(centres=[(0.0, 1.5, 0.0), (-1.3, 0.6, 0.2), (-1.4, -0.9, 0.0), (1.3, 0.6, -0.2), (1.4, -0.9, 0.0)],
         radii=[1.4, 1.3, 1.4, 1.3, 1.4], h=0.7, cloud=300),
)
FN_ATOMS = (24, 30, 36, 28, 40, 32)           # atoms of the six molecules of the function fixture (groups: 24 | 94 | 72)
FN_FAR = 6                                    # far atoms per group there


def meshes():
    out = []
    for g, m in enumerate(MESHES):
        verts, faces = M.sphere_union_mesh(m["centres"], m["radii"], m["h"], seed=11 + g)
        assert M.check_closed(faces) and 200 <= len(faces) <= 2500, len(faces)
        out.append((verts, faces, M.sample_surface(verts, faces, m["cloud"], seed=21 + g)))
    assert len({len(f) for _v, f, _c in out}) == 3
    return out


class GroupRecorder(MeshRecorder):
    """MeshRecorder that also keeps, per call, the number of within-atoms and the atoms never accepted."""

    def __init__(self, verts, faces, cloud, n_atoms, seed):
        super().__init__(verts, faces, cloud, n_atoms)
        self._rs = np.random.RandomState(seed)
        self.n_within, self.never = [], []

    def contains(self, x):
        was_fresh = self.fresh
        c = super().contains(x)
        if was_fresh:
            self.n_within.append(len(self.within))
            self.never.append(np.zeros(self.n, dtype=bool))
        elif self.it == 5:
            self.never[-1][self.rem] = True
        return c


class Dispatcher:
    """Stands in for the reference's module-level mesh_shape_guidance: the real function once per group on the group's slice."""

    def __init__(self, real, mesh_set, atom_off, seed):
        from sklearn.neighbors import KDTree
        self.real, self.atom_off, self.first, self.preds = real, atom_off, {}, []
        self.recs = [None if m is None else GroupRecorder(m[0], m[1], m[2], int(atom_off[g + 1] - atom_off[g]), seed + g)
                     for g, m in enumerate(mesh_set)]
        self.data = [None if m is None else (rec, m[2], KDTree(m[2])) for m, rec in zip(mesh_set, self.recs)]

    def __call__(self, use_mesh_data, pred_ligand_pos, k=3, ratio=0.5):
        self.preds.append(pred_ligand_pos.numpy().copy())          # the prediction before guidance, of every guided step
        if not self.first:
            self.first["pred"] = pred_ligand_pos.numpy().copy()
        real_random, real_cuda = np.random.random, torch.Tensor.cuda
        torch.Tensor.cuda = lambda t, *a, **kw: t         # the reference hard-codes .cuda() (:774); this harness runs on the CPU
        try:
            for g, rec in enumerate(self.recs):
                if rec is None:
                    continue
                np.random.random = rec.random
                lo, hi = int(self.atom_off[g]), int(self.atom_off[g + 1])
                part = pred_ligand_pos[lo:hi].clone()
                pred_ligand_pos[lo:hi] = self.real(self.data[g], part, k, ratio)
        finally:
            np.random.random, torch.Tensor.cuda = real_random, real_cuda
        if "out" not in self.first:
            self.first["out"] = pred_ligand_pos.numpy().copy()
        return pred_ligand_pos

    def tables(self, n_steps, tag):
        """Draws (n_steps, 5, N) and per guided step: pulls and never-accepted per atom, within-atoms per group; with the asserts."""
        na, off = int(self.atom_off[-1]), self.atom_off
        guided = max(len(r.steps) for r in self.recs if r is not None)
        draws = np.full((n_steps, 5, na), 0.5)
        pulls, never = np.zeros((guided, na), dtype=np.int8), np.zeros((guided, na), dtype=bool)
        n_within = np.full((guided, len(self.recs)), -1, dtype=np.int32)
        for g, rec in enumerate(self.recs):
            if rec is None:
                continue
            assert len(rec.steps) == guided and rec.fresh
            st = np.stack(rec.steps)
            draws[:guided, :, off[g]:off[g + 1]] = st
            pulls[:, off[g]:off[g + 1]] = (st != 0.5).sum(1)
            never[:, off[g]:off[g + 1]] = np.stack(rec.never)
            n_within[:, g] = rec.n_within
            assert (pulls[:, off[g]:off[g + 1]] > 0).any(1).all(), f"{tag}: group {g} pulls no atom in some guided step"
            assert (n_within[:, g] >= 3).all(), f"{tag}: group {g} has fewer than 3 within-atoms in some step"
            print(tag, "group", g, "pulled per step", (pulls[:, off[g]:off[g + 1]] > 0).sum(1).tolist(), "within", rec.n_within,
                  "never", never[:, off[g]:off[g + 1]].sum(1).tolist(), rec.seen, flush=True)
        assert (pulls >= 2).any(), f"{tag}: no atom needs two pulls"
        assert never.any(), f"{tag}: every pulled atom is accepted"
        assert (pulls[never] == 5).all()
        return guided, draws, pulls, never, n_within


def group_meta(mesh_set):
    return dict(group_mols=np.array(GROUP_MOLS), has_mesh=np.array([m is not None for m in mesh_set]))


def run_fn(R, ms):
    """The dispatcher alone on atoms scattered over and beyond each group's mesh."""
    counts = np.array(FN_ATOMS)
    batch = np.repeat(np.arange(B), counts)
    atom_off = np.concatenate([[0], np.cumsum(counts)])[np.concatenate([[0], np.cumsum(GROUP_MOLS)])]
    pred = synth.hash_normal((len(batch), 3), 412, 5) * np.array([1.9, 1.7, 1.1])
    for g in range(3):
        pred[atom_off[g]:atom_off[g + 1]] += np.mean(MESHES[g]["centres"], 0)
        pred[atom_off[g + 1] - FN_FAR:atom_off[g + 1]] *= 9.0          # a few far atoms: some are never accepted in five pulls
    pred = pred.astype(np.float32)
    d = Dispatcher(R.mesh_shape_guidance, ms, atom_off, 90)
    out = d(("per group", None, None), torch.from_numpy(pred.copy())).numpy()
    guided, draws, pulls, never, n_within = d.tables(1, "mesh_guidance_multi_fn")
    assert guided == 1
    ora = pred.copy()
    for g, (v, f, c) in enumerate(ms):
        lo, hi = atom_off[g], atom_off[g + 1]
        ora[lo:hi] = M.mesh_shape_guidance(v, f, c, pred[lo:hi], draws[0][:, lo:hi])
    assert np.array_equal(ora, out), "the oracle per group does not reproduce the reference per group"
    off = lambda k: np.concatenate([[0], np.cumsum([len(m[k]) for m in ms])])      # noqa: E731
    np.savez_compressed(
        os.path.join(HERE, "mesh_guidance_multi_fn.npz"), verts=np.concatenate([m[0] for m in ms]), vert_off=off(0),
        faces=np.concatenate([m[1] for m in ms]).astype(np.int32), face_off=off(1), clouds=np.concatenate([m[2] for m in ms]),
        cloud_off=off(2), batch=batch, pred=pred, out=out, draws=draws[0], pulls=pulls[0], never=never[0], n_within=n_within[0],
        **group_meta(ms))


def run_chain(model, R, bb, eps, u, ms, tag):
    """One chain; `ms[g]` is None for a group without a mesh."""
    mol_off = np.concatenate([[0], np.cumsum(GROUP_MOLS)])
    atom_off = np.concatenate([[0], np.cumsum(bb["counts"])])[mol_off]
    real = R.mesh_shape_guidance
    d = Dispatcher(real, ms, atom_off, 80)
    R.mesh_shape_guidance = d
    try:
        with G.fed_noise(list(eps), list(u)), contextlib.redirect_stdout(open(os.devnull, "w")):
            r = model.sample_diffusion(G.t_(bb["init_pos"]), G.t_(bb["init_v"]), G.t_(bb["batch"]), G.t_(bb["shape"]).view(B, -1),
                                       num_steps=S, center_pos_mode="none", use_mesh_data=("per group", None, None),
                                       grad_step=GRAD_STEP)
    finally:
        R.mesh_shape_guidance = real
    guided, draws, pulls, never, n_within = d.tables(S, tag)
    assert guided == 999 - GRAD_STEP
    st = lambda k: torch.stack([torch.as_tensor(x) for x in r[k]]).numpy()      # noqa: E731
    np.savez_compressed(
        os.path.join(HERE, f"{tag}.npz"), B=B, S=S, seed=SEED, grad_step=GRAD_STEP, guided_steps=guided, draws=draws,
        pulls=pulls, never=never, n_within=n_within, traj_steps=TRAJ_STEPS, pos=r["pos"].numpy(), v=r["v"].numpy(),
        v_traj=st("v_traj").astype(np.int8), pos_traj=st("pos_traj")[TRAJ_STEPS], pos_cond_traj=st("pos_cond_traj")[TRAJ_STEPS],
        fn_pred=d.first["pred"], fn_out=d.first["out"], guided_pred=np.stack(d.preds), **group_meta(ms))


def main():
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", 8)))
    model, _ = G.load_reference_model()                   # also puts the reference's `models` package on the path
    G.synthetic_load(model, seed=7)
    import models.molopt_score_model as R
    ms = meshes()
    for g, (v, f, c) in enumerate(ms):
        print("mesh", g, len(v), "vertices", len(f), "faces", len(c), "cloud points; extent", (v.max(0) - v.min(0)).round(2), flush=True)
    run_fn(R, ms)
    bb = synth.synthetic_batch(B, seed=SEED)
    n = len(bb["batch"])
    eps, u = zip(*[synth.step_noise(n, 15, s, seed=SEED) for s in range(S)])
    run_chain(model, R, bb, eps, u, ms, "chain_mesh_guided_multi_b6_s20")
    run_chain(model, R, bb, eps, u, [ms[0], None, ms[2]], "chain_mesh_guided_multi_b6_s20_gap")


if __name__ == "__main__":
    main()
