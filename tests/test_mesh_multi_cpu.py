"""Mesh shape guidance with one mesh per group of molecules, the parts that need no GPU: the fixtures of
tests/golden/make_golden_mesh_multi.py (self-consistency against tests/mesh_oracle.py's single-mesh function applied per group,
and the conditions the generator promises), the argument checks of sample_diffusion, the host arrays and the driver's planning."""
import os
import re

import numpy as np
import pytest
import torch

import mesh_oracle as M
from mesh_multi_util import CHAINS, FN, atom_ranges, chain_batch, mesh_groups, meshes
from util import ROOT, golden, model_cfg, synth


def walk(verts, faces, cloud, pred, draws):
    """The guidance of one group step by step (as mesh_oracle.mesh_shape_guidance) -> (pulls per atom, never accepted per atom,
    number of within-atoms); asserts that the 3rd and 4th nearest within-atoms of a pulled point never tie."""
    t = M.MeshTables(verts, faces)
    inside, d = M.contains_parity(t, pred), M.nearest_dist(cloud, pred)
    within = pred[inside & (d > 0.4)]
    idx = np.where(~inside | (d < 0.2))[0]
    pts = pred[idx]
    pulls, never = np.zeros(len(pred), dtype=np.int64), np.zeros(len(pred), dtype=bool)
    for j in range(5):
        if not len(idx):
            break
        nb, d2 = M.knn3(within, pts)
        if len(within) >= 4:
            assert (d2[:, 2] < d2[:, 3]).all()
        w = within[nb]
        mean = ((w[:, 0] + w[:, 1]) + w[:, 2]) / np.float32(3)
        new = pts - (draws[j, idx][:, None] * 0.8 + 0.2) * (pts - mean)
        pulls[idx] += 1
        ok = M.contains_parity(t, new) & (M.nearest_dist(cloud, new) > 0.2)
        idx, pts = idx[~ok], new[~ok]
    never[idx] = True
    return pulls, never, len(within)


def fn_ranges(f):
    counts = np.bincount(f["batch"])
    return atom_ranges(counts, f["group_mols"])[1]


def test_header_declares_and_lib_exports_the_entry_points():
    from shapemol_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "shapemol_hip.h")).read()
    assert re.search(r"\bint shapemol_set_mesh_guidance_groups\(shapemol_ctx \*ctx, int32_t n_groups, const int64_t \*h_mol_off, "
                     r"const double \*h_verts,\s+const int64_t \*h_vert_off, const int32_t \*h_faces, const int64_t \*h_face_off,\s+"
                     r"const double \*h_clouds, const int64_t \*h_cloud_off, int32_t grad_step, const double \*d_draws\);", hdr)
    assert re.search(r"\bint shapemol_guide_points_mesh_groups\(shapemol_ctx \*ctx, float \*d_pos, const int64_t \*d_batch, int64_t n_atoms,", hdr)
    assert {"shapemol_set_mesh_guidance_groups", "shapemol_guide_points_mesh_groups"} <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 5 and re.search(r"#define SHAPEMOL_ABI_VERSION 5\b", hdr)
    from shapemol_amd.molopt_score_model import ScorePosNet3D
    assert hasattr(ScorePosNet3D, "mesh_shape_guidance_groups")


def test_fixture_layout():
    f = golden(FN)
    ms = meshes()
    assert f["group_mols"].tolist() == [1, 3, 2] and len(ms) == 3
    assert f["verts"].dtype == np.float64 and f["faces"].dtype == np.int32 and f["clouds"].dtype == np.float64
    n_faces = [len(m[1]) for m in ms]
    assert len(set(n_faces)) == 3 and 200 <= min(n_faces) and max(n_faces) <= 2500
    assert len({len(m[2]) for m in ms}) == 3 and all(3 <= len(m[2]) <= 2048 for m in ms)
    for v, fc, cl in ms:
        assert fc.min() >= 0 and fc.max() < len(v) and M.check_closed(fc)         # indices relative to the group's vertices
        assert np.abs(M.nearest_dist(v, cl)).max() < 1.0                          # the cloud lies on this mesh's surface
    centres = [m[0].mean(0) for m in ms]
    assert min(np.abs(centres[a] - centres[b]).max() for a in range(3) for b in range(a)) > 0.2
    c, g = golden(CHAINS[0]), golden(CHAINS[1])
    for x in (c, g):
        assert int(x["B"]) == 6 and x["group_mols"].tolist() == [1, 3, 2] and int(x["S"]) == 20 and int(x["grad_step"]) == 990
        assert int(x["guided_steps"]) == 9 and x["draws"].shape == (20, 5, len(x["fn_pred"])) and x["fn_pred"].dtype == np.float32
        assert ((x["draws"] >= 0) & (x["draws"] < 1)).all() and not (x["draws"][9:] != 0.5).any()
    assert c["has_mesh"].tolist() == [True, True, True] and g["has_mesh"].tolist() == [True, False, True]


def test_oracle_per_group_reproduces_the_function_fixture():
    """tests/mesh_oracle.py's single-mesh guidance applied once per group to the group's slice, with the group's mesh, cloud and
    draws, gives the reference dispatcher's output exactly (the single-mesh CPU test's tolerance: equality)."""
    f = golden(FN)
    off = fn_ranges(f)
    out = f["pred"].copy()
    for g, (v, fc, cl) in enumerate(meshes()):
        lo, hi = off[g], off[g + 1]
        out[lo:hi] = M.mesh_shape_guidance(v, fc, cl, f["pred"][lo:hi], f["draws"][:, lo:hi])
    assert np.array_equal(out, f["out"])
    assert (out != f["pred"]).any(1).sum() > 100


@pytest.mark.parametrize("name", CHAINS)
def test_oracle_per_group_reproduces_the_chain_first_step(name):
    c = golden(name)
    _, off = atom_ranges(chain_batch(c)["counts"], c["group_mols"])
    out = c["fn_pred"].copy()
    for g, (mesh, cloud, _, _n) in enumerate(mesh_groups(c)):
        lo, hi = off[g], off[g + 1]
        if mesh is not None:
            out[lo:hi] = M.mesh_shape_guidance(mesh[0], mesh[1], cloud, c["fn_pred"][lo:hi], c["draws"][0][:, lo:hi])
        else:
            assert np.array_equal(c["fn_out"][lo:hi], c["fn_pred"][lo:hi])
    assert np.array_equal(out, c["fn_out"])
    # the per-group search matters: with the within-atoms of the whole batch (one KD-tree for all) group 0 comes out differently
    lo, hi = off[0], off[1]
    m0 = mesh_groups(c)[0]
    whole = M.mesh_shape_guidance(m0[0][0], m0[0][1], m0[1], c["fn_pred"], c["draws"][0])
    assert not np.array_equal(whole[lo:hi], c["fn_out"][lo:hi])


@pytest.mark.parametrize("name", (FN,) + CHAINS)
def test_fixture_coverage(name):
    """What the generator promises, from the stored tables: in every guided step every meshed group pulls at least one atom and
    has >= 3 within-atoms, some atom needs two or more pulls, some atom is never accepted; the tables agree with the draws, and
    with a re-walk of the guidance of EVERY guided step from its stored prediction (``guided_pred``; the function fixture's
    ``pred``), in which the 3rd and 4th nearest within-atoms of a pulled atom never tie."""
    c = golden(name)
    fn = name == FN
    pulls, never, n_within = (c[k][None] if fn else c[k] for k in ("pulls", "never", "n_within"))
    draws = c["draws"][None] if fn else c["draws"]
    off = fn_ranges(c) if fn else atom_ranges(chain_batch(c)["counts"], c["group_mols"])[1]
    steps = 1 if fn else int(c["guided_steps"])
    assert pulls.shape == never.shape == (steps, off[-1]) and n_within.shape == (steps, 3)
    drawn = draws[:steps] != 0.5
    assert np.array_equal(drawn.sum(1), pulls)                      # an atom's draw differs from the filler iff it was pulled
    assert (np.diff(drawn.astype(int), axis=1) <= 0).all()          # ... in consecutive iterations from the first on
    assert (pulls >= 2).any() and never.any() and (pulls[never] == 5).all()
    preds = c["pred"][None] if fn else c["guided_pred"]
    res = c["out"] if fn else c["fn_out"]
    assert preds.shape == (steps, off[-1], 3) and preds.dtype == np.float32
    if not fn:
        assert np.array_equal(preds[0], c["fn_pred"])
    ms = meshes()
    for g in range(3):
        lo, hi = off[g], off[g + 1]
        if not c["has_mesh"][g]:
            assert not pulls[:, lo:hi].any() and (n_within[:, g] == -1).all()
            continue
        assert (pulls[:, lo:hi] > 0).any(1).all() and (n_within[:, g] >= 3).all()
        for s in range(steps):
            p, nv, nw = walk(*ms[g], preds[s, lo:hi], draws[s][:, lo:hi])
            assert np.array_equal(p, pulls[s, lo:hi]) and np.array_equal(nv, never[s, lo:hi]) and nw == n_within[s, g], (g, s)
            if s == 0:
                assert np.array_equal((res[lo:hi] != preds[0, lo:hi]).any(1), (p > 0) & ~nv)        # never accepted: original position


class _NoLibrary(RuntimeError):
    pass


def _cpu_model(monkeypatch):
    import shapemol_amd
    from shapemol_amd import _lib

    def no_load():
        raise _NoLibrary("the library must not be loaded by an argument check")
    monkeypatch.setattr(_lib, "load", no_load)
    return shapemol_amd.ScorePosNet3D(model_cfg(), 15)


def test_argument_checks_raise_before_the_library_is_loaded(monkeypatch):
    m = _cpu_model(monkeypatch)
    bb = synth.synthetic_batch(6, seed=31)
    args = (torch.from_numpy(bb["init_pos"]), torch.from_numpy(bb["init_v"]), torch.from_numpy(bb["batch"]),
            torch.from_numpy(bb["shape"]).view(6, -1))
    v, f, cloud = meshes()[0]
    mesh = (v, f)
    with pytest.raises(ValueError, match="5 molecules, the batch has 6"):
        m.sample_diffusion(*args, num_steps=2, use_mesh_data=[(mesh, cloud, None, 2), (None, None, None, 3)])
    with pytest.raises(ValueError, match="7 molecules, the batch has 6"):
        m.sample_diffusion(*args, num_steps=2, use_mesh_data=[(mesh, cloud, None, 7)])
    with pytest.raises(ValueError, match=r"use_mesh_data\[1\] must be"):
        m.sample_diffusion(*args, num_steps=2, use_mesh_data=[(mesh, cloud, None, 3), (mesh, cloud, None)])
    with pytest.raises(ValueError, match="empty"):
        m.sample_diffusion(*args, num_steps=2, use_mesh_data=[])
    with pytest.raises(ValueError, match=r"use_mesh_data\[0\]: n_mols < 0"):
        m.sample_diffusion(*args, num_steps=2, use_mesh_data=[(mesh, cloud, None, -1), (None, None, None, 7)])
    with pytest.raises(NotImplementedError, match="mesh groups and point-cloud groups in one chain"):
        m.sample_diffusion(*args, num_steps=2, use_mesh_data=[(mesh, cloud, None, 6)], use_pointcloud_data=[(cloud, None, 0.2, 6)])
    with pytest.raises(ValueError, match="a face names a vertex outside"):
        m.sample_diffusion(*args, num_steps=2, use_mesh_data=[((v[:10], f), cloud, None, 6)])
    # a well-formed list (also beside a single cloud: the mesh wins) passes the checks and gets as far as the device check
    with pytest.raises(RuntimeError, match="HIP device"):
        m.sample_diffusion(*args, num_steps=2, use_mesh_data=[(mesh, cloud, None, 4), (None, None, None, 2)])
    with pytest.raises(RuntimeError, match="HIP device"):
        m.sample_diffusion(*args, num_steps=2, use_mesh_data=[(mesh, cloud, None, 6)], use_pointcloud_data=(cloud, None, 0.2))


def test_group_arrays():
    from shapemol_amd.guidance import _mesh_guidance_groups
    (v0, f0, c0), (v1, f1, c1), _ = meshes()

    class TrimeshLike:
        vertices, faces = v1, f1.astype(np.int64)
    mol_off, verts, vert_off, faces, face_off, clouds, cloud_off = _mesh_guidance_groups(
        [((v0, f0), c0, None, 2), (None, None, None, 1), (TrimeshLike(), torch.from_numpy(c1), "tree", 4)], 7)
    for a in (mol_off, vert_off, face_off, cloud_off):
        assert a.dtype == np.int64
    assert mol_off.tolist() == [0, 2, 3, 7]
    assert vert_off.tolist() == [0, len(v0), len(v0), len(v0) + len(v1)]
    assert face_off.tolist() == [0, len(f0), len(f0), len(f0) + len(f1)]
    assert cloud_off.tolist() == [0, len(c0), len(c0), len(c0) + len(c1)]
    assert verts.dtype == np.float64 and verts.flags["C_CONTIGUOUS"] and np.array_equal(verts, np.concatenate([v0, v1]))
    assert faces.dtype == np.int32 and faces.flags["C_CONTIGUOUS"] and np.array_equal(faces, np.concatenate([f0, f1]))       # relative indices
    assert clouds.dtype == np.float64 and np.array_equal(clouds, np.concatenate([c0, c1]))


def test_driver_planning_with_mesh_conditions():
    from shapemol_amd.sampling import guidance_groups, plan_batches, plan_guidance
    (v0, f0, c0), (v1, f1, c1), _ = meshes()
    s = np.zeros((32, 3))
    md0, md1, pc = ((v0, f0), c0, "tree0"), ((v1, f1), c1, "tree1"), (c0, "tree", 0.25)
    kind, data = plan_guidance([(s, None, md0), (s, None), (s, pc, md1)])          # a mesh beside a cloud: the mesh guides
    assert kind == "mesh" and data[0] is md0 and data[1] is None and data[2] is md1
    plan = plan_batches(3, 5, 8)
    assert plan == [[(0, 0, 5), (1, 0, 3)], [(1, 3, 2), (2, 0, 5)]]
    key, groups = guidance_groups(kind, data, plan[0])
    assert key == "use_mesh_data" and groups == [(md0[0], c0, None, 5), (None, None, None, 3)]
    key, groups = guidance_groups(kind, data, plan[1])
    assert key == "use_mesh_data" and groups[0] == (None, None, None, 2) and groups[1][0] is md1[0] and groups[1][3] == 5
    assert guidance_groups(kind, data, [(1, 0, 3)]) == (None, None)                # a batch of unguided conditions only
    # clouds as before, nothing, and the refused mixture
    kind, data = plan_guidance([(s, pc), (s, None, None)])
    assert kind == "cloud" and guidance_groups(kind, data, [(0, 0, 2), (1, 0, 2)]) == ("use_pointcloud_data", [(c0, None, 0.25, 2), (None, None, None, 2)])
    assert plan_guidance([(s, None), (s, None, None)]) == (None, [None, None])
    with pytest.raises(ValueError, match="mix meshes and point clouds"):
        plan_guidance([(s, pc), (s, None, md0)])
    with pytest.raises(ValueError, match=r"conditions\[1\] must be"):
        plan_guidance([(s, pc), (s,)])
    # the driver refuses the mixture before any chain runs (no device needed)

    class Accelerated:
        _accelerated = True
    from shapemol_amd.sampling import sample_diffusion_ligand_multi
    with pytest.raises(ValueError, match="mix meshes and point clouds"):
        sample_diffusion_ligand_multi(Accelerated(), [(s, pc), (s, None, md0)], 2)
