#!/usr/bin/env python3
"""Mesh shape guidance fixtures, from the reference itself (models/molopt_score_model.py:742-775, called from
sample_diffusion at :571-580).

    python tests/golden/make_golden_mesh.py

Same harness as make_golden_r2.py's point-cloud fixtures: the reference's own mesh_shape_guidance and sample_diffusion run on
the CPU with the real sklearn KDTree; np.random.random is recorded into the dense (5, N) / (S, 5, N) tables the device path
takes.  trimesh is not needed: the mesh is a marching-tetrahedra surface of a union of spheres (tests/mesh_oracle.py), and the
stub handed to the reference as `mesh` answers `.contains` with the test-local ray parity -- after asserting, on EVERY query,
that it agrees with the generalized winding number (|w - round(w)| < 1e-6).  No fixture point's answer then depends on the
containment method.  The 3rd and 4th nearest within-atoms of every pulled atom never tie.

Writes mesh_fixture.npz (mesh + 512-point cloud), mesh_guidance_fn.npz (the function on 300 scattered atoms) and
chain_mesh_guided_b4_s20.npz (B = 4, 20 reverse steps, grad_step = 990, hash noise as chain_guided_b4_s20.npz).
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
from shapemol_amd import synth  # noqa: E402

t_ = G.t_


class MeshRecorder:
    """Stands in for the trimesh mesh handed to the reference's mesh_shape_guidance and for np.random.random during the
    call: answers `.contains` with the ray parity (checked against the winding number) and mirrors the function's control
    flow to learn WHICH atoms receive each uniform draw (one per remaining outmesh atom, in index order)."""

    def __init__(self, verts, faces, cloud, n_atoms):
        self.verts, self.faces, self.cloud, self.n = verts, faces, cloud, n_atoms
        self.tables = M.MeshTables(verts, faces)
        self.steps, self.fresh, self.queries = [], True, 0
        self.seen = dict(inside=0, outside=0, near_cloud_inside=0, accepted_first=0, accepted_later=0, never=0)

    def _contains(self, x):
        x = np.asarray(x, dtype=np.float64)
        par = M.contains_parity(self.tables, x)
        w = M.winding_number(self.verts, self.faces, x)
        assert np.abs(w - np.round(w)).max() < 1e-6, "a query point is too close to the surface: change the seed"
        assert np.array_equal(par, np.round(w) == 1), "ray parity and winding number disagree"
        self.queries += len(x)
        return par

    def contains(self, x):
        c = self._contains(x)
        d = M.nearest_dist(self.cloud, x)
        if self.fresh:                               # first query of a call: all atoms
            assert len(x) == self.n
            self.steps.append(np.full((5, self.n), 0.5))
            self.within = np.asarray(x, dtype=np.float32)[c & (d > 0.4)]
            self.rem = np.where(~c | (d < 0.2))[0]
            self.cur, self.it = np.asarray(x)[self.rem], 0
            self.fresh = len(self.rem) == 0
            self.seen["inside"] += int(c.sum()); self.seen["outside"] += int((~c).sum())
            self.seen["near_cloud_inside"] += int((c & (d < 0.2)).sum())
        else:                                        # re-check of the pulled atoms
            assert len(x) == len(self.rem)
            ok = c & (d > 0.2)
            self.seen["accepted_first" if self.it == 0 else "accepted_later"] += int(ok.sum())
            self.rem, self.cur = self.rem[~ok], np.asarray(x)[~ok]
            self.it += 1
            self.fresh = len(self.rem) == 0 or self.it == 5
            if self.it == 5:
                self.seen["never"] += len(self.rem)
        return c

    def random(self, n):
        assert not self.fresh and n == len(self.rem)
        if len(self.within) >= 4:
            _, d2 = M.knn3(self.within, self.cur)
            assert (d2[:, 2] < d2[:, 3]).all(), "3rd / 4th nearest within-atoms tie: change the seed"
        u = self._rs.random_sample(n)
        self.steps[-1][self.it, self.rem] = u
        return u

    @contextlib.contextmanager
    def active(self, seed):
        self._rs = np.random.RandomState(seed)
        real_random, real_cuda = np.random.random, torch.Tensor.cuda
        np.random.random = self.random
        torch.Tensor.cuda = lambda t, *a, **k: t          # the reference hard-codes .cuda() (:774); this harness runs on the CPU
        try:
            yield self
        finally:
            np.random.random, torch.Tensor.cuda = real_random, real_cuda


def main():
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", 8)))
    from sklearn.neighbors import KDTree
    model, _ = G.load_reference_model()                   # also puts the reference's `models` package on the path
    G.synthetic_load(model, seed=7)
    from models.molopt_score_model import mesh_shape_guidance
    verts, faces = M.sphere_union_mesh(M.FIXTURE_CENTRES, M.FIXTURE_RADII, 0.5, seed=1)
    assert M.check_closed(faces) and len(faces) >= 1000
    cloud = M.sample_surface(verts, faces, 512, seed=2)
    np.savez_compressed(os.path.join(HERE, "mesh_fixture.npz"), verts=verts, faces=faces, cloud=cloud)
    print("mesh:", len(verts), "vertices,", len(faces), "faces; extent", (verts.max(0) - verts.min(0)).round(2), flush=True)
    kdtree = KDTree(cloud)
    # (A) the function alone: atoms scattered over and beyond the mesh
    n = 300
    pred = synth.hash_normal((n, 3), 402, 5) * np.array([2.4, 1.6, 1.2])
    pred[-40:] *= 12.0                                     # a few far atoms: some are never accepted in five pulls
    pred = pred.astype(np.float32)
    rec = MeshRecorder(verts, faces, cloud, n)
    with rec.active(79):
        out = mesh_shape_guidance((rec, cloud, kdtree), torch.from_numpy(pred.copy())).numpy()
    draws = rec.steps[0]
    ora = M.mesh_shape_guidance(verts, faces, cloud, pred, draws)
    assert np.array_equal(ora, out), "the oracle does not reproduce the reference"
    s = rec.seen
    print("mesh_guidance_fn:", s, "moved", int((out != pred).any(1).sum()), "of", n, flush=True)
    assert s["inside"] and s["outside"] and s["near_cloud_inside"] and s["accepted_first"] and s["accepted_later"] and s["never"]
    np.savez_compressed(os.path.join(HERE, "mesh_guidance_fn.npz"), pred=pred, out=out, draws=draws)
    # (B) inside a chain: B = 4, 20 reverse steps, guided while t > 990
    B, S, seed, grad_step = 4, 20, 21, 990
    bb = synth.synthetic_batch(B, seed=seed)
    na = len(bb["batch"])
    eps, u = zip(*[synth.step_noise(na, 15, s_, seed=seed) for s_ in range(S)])
    rec = MeshRecorder(verts, faces, cloud, na)
    with G.fed_noise(list(eps), list(u)), rec.active(80), contextlib.redirect_stdout(open(os.devnull, "w")):
        r = model.sample_diffusion(t_(bb["init_pos"]), t_(bb["init_v"]), t_(bb["batch"]), t_(bb["shape"]).view(B, -1), num_steps=S,
                                   center_pos_mode="none", use_mesh_data=(rec, cloud, kdtree), grad_step=grad_step)
    draws = np.full((S, 5, na), 0.5)
    draws[:len(rec.steps)] = np.stack(rec.steps)          # guided steps come first (t = 999 ... grad_step + 1)
    print("chain_mesh_guided: guided steps", len(rec.steps), "of", S, rec.seen, "contains queries", rec.queries, flush=True)
    np.savez_compressed(os.path.join(HERE, "chain_mesh_guided_b4_s20.npz"), B=B, S=S, seed=seed, grad_step=grad_step,
                        draws=draws, guided_steps=len(rec.steps), pos=r["pos"].numpy(), v=r["v"].numpy(),
                        pos_traj=torch.stack(r["pos_traj"]).numpy(), v_traj=torch.stack(r["v_traj"]).numpy(),
                        pos_cond_traj=torch.stack(r["pos_cond_traj"]).numpy())


if __name__ == "__main__":
    main()
