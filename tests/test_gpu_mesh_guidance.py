"""Mesh shape guidance on the device (the reference's mesh_shape_guidance, models/molopt_score_model.py:742-775, and its use
inside sample_diffusion, :571-580) against the reference's fixtures (tests/golden/make_golden_mesh.py) and the test-local
oracle (tests/mesh_oracle.py).  Run on the GPU box:  pytest tests/test_gpu_mesh_guidance.py -m gpu"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mesh_oracle as M  # noqa: E402
from util import T, golden, hash_noise, hip_model, maxabs, record, synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POS_TOL = 1e-4      # coordinates of a chain (as the other chain parity tests)
FN_TOL = 1e-6       # the function alone: float64 arithmetic as numpy's, rounded once to float32


def _mesh():
    m = golden("mesh_fixture.npz")
    return m["verts"], m["faces"], m["cloud"]


def _data(verts=None):
    v, f, c = _mesh()
    return ((v if verts is None else verts, f), c, None)


class _TrimeshLike:
    def __init__(self, vertices, faces):
        self.vertices, self.faces = vertices, faces


def _moved(a, b):
    return (np.asarray(a) != np.asarray(b)).any(1)


def test_mesh_function_golden():
    """The two kernels on their own against the reference's function on the recorded draws: the same moved set, positions
    within 1e-6; in place; k / ratio ignored; the context-bound entry points give the same."""
    import shapemol_amd
    from shapemol_amd import _lib
    f = golden("mesh_guidance_fn.npz")
    verts, faces, cloud = _mesh()
    pos = T(f["pred"].copy(), DEV)
    out = shapemol_amd.mesh_shape_guidance(((_TrimeshLike(verts, faces)), cloud, None), pos, draws=T(f["draws"], DEV))
    assert out is pos
    got = out.cpu().numpy()
    err = maxabs(got, f["out"])
    record("mesh_function_golden", moved=int(_moved(f["out"], f["pred"]).sum()), max_err=err)
    assert np.array_equal(_moved(got, f["pred"]), _moved(f["out"], f["pred"]))
    assert err <= FN_TOL
    for k, ratio in ((5, 0.1), (1, 0.7)):
        again = shapemol_amd.mesh_shape_guidance(_data(), T(f["pred"].copy(), DEV), k, ratio, draws=T(f["draws"], DEV)).cpu().numpy()
        assert np.array_equal(again, got)
    # shapemol_set_mesh_guidance + shapemol_guide_points_mesh on a model's context
    m = hip_model()
    lib = _lib.load()
    ctx = m._context(torch.device(DEV))
    cf = np.ascontiguousarray(faces.astype(np.int32))
    vp = lambda a: a.ctypes.data_as(_lib.C.c_void_p)  # noqa: E731
    _lib.check(lib.shapemol_set_mesh_guidance(ctx, vp(verts), len(verts), vp(cf), len(cf), vp(cloud), len(cloud), 0, None), "set")
    try:
        p2 = T(f["pred"].copy(), DEV)
        d2 = T(f["draws"], DEV)
        _lib.check(lib.shapemol_guide_points_mesh(ctx, _lib.C.c_void_p(p2.data_ptr()), len(p2), _lib.C.c_void_p(d2.data_ptr()),
                                                  _lib.C.c_uint64(0), _lib.C.c_void_p(torch.cuda.current_stream().cuda_stream)), "guide")
        torch.cuda.synchronize()
        assert np.array_equal(p2.cpu().numpy(), got)
    finally:
        _lib.check(lib.shapemol_set_mesh_guidance(ctx, None, 0, None, 0, None, 0, 0, None), "unset")


def test_mesh_function_philox():
    """Device-drawn uniforms: deterministic per seed, np.random.seed reproduces a call, every moved atom satisfies the
    acceptance rule under the oracle, and every atom that is not moved is unmoved."""
    from shapemol_amd import mesh_shape_guidance
    f = golden("mesh_guidance_fn.npz")
    verts, faces, cloud = _mesh()
    pred = f["pred"]
    a = mesh_shape_guidance(_data(), T(pred.copy(), DEV), seed=5).cpu().numpy()
    b = mesh_shape_guidance(_data(), T(pred.copy(), DEV), seed=5).cpu().numpy()
    c = mesh_shape_guidance(_data(), T(pred.copy(), DEV), seed=6).cpu().numpy()
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    np.random.seed(3); x = mesh_shape_guidance(_data(), T(pred.copy(), DEV)).cpu().numpy()
    np.random.seed(3); y = mesh_shape_guidance(_data(), T(pred.copy(), DEV)).cpu().numpy()
    assert np.array_equal(x, y)
    tables = M.MeshTables(verts, faces)
    inside0 = M.contains_parity(tables, pred)
    d0 = M.nearest_dist(cloud, pred)
    outmesh = ~inside0 | (d0 < 0.2)
    for r in (a, c, x):
        mv = _moved(r, pred)
        assert mv.any() and not (mv & ~outmesh).any()               # only outmesh atoms move
        pts = r[mv].astype(np.float64)
        assert M.contains_parity(tables, pts).all() and (M.nearest_dist(cloud, pts) > 0.2 - 1e-6).all()


def test_mesh_function_at_size():
    """5.5k atoms (a B = 256 batch's worth, the spread of the chains' predictions plus far atoms) against the oracle with
    fixed draws: several LDS tiles of within-atoms, a within set across molecules."""
    from shapemol_amd import mesh_shape_guidance
    verts, faces, cloud = _mesh()
    n = 5500
    pred = synth.hash_normal((n, 3), 403, 5) * np.array([2.4, 1.6, 1.2])
    pred[::10] *= 4.0
    pred = pred.astype(np.float32)
    draws = synth.hash_normal((5, n), 404, 5)
    draws = (np.abs(draws) % 1.0).astype(np.float64)
    ref = M.mesh_shape_guidance(verts, faces, cloud, pred, draws)
    got = mesh_shape_guidance(_data(), T(pred.copy(), DEV), draws=T(draws, DEV)).cpu().numpy()
    err = maxabs(got, ref)
    record("mesh_function_at_size", n=n, moved=int(_moved(ref, pred).sum()), max_err=err)
    assert np.array_equal(_moved(got, pred), _moved(ref, pred))
    assert err <= FN_TOL


def _batch(c):
    B, S, seed = int(c["B"]), int(c["S"]), int(c["seed"])
    bb = synth.synthetic_batch(B, seed=seed)
    eps, u = hash_noise(len(bb["batch"]), S, seed)
    args = (T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1))
    return args, dict(num_steps=S, center_pos_mode="none", noise=(T(eps, DEV), T(u, DEV)))


def test_mesh_guided_chain_golden():
    """sample_diffusion(use_mesh_data=..., grad_step=990): 20 reverse steps, the first 9 guided, against the reference's chain
    (recorded draws), with and without the captured graph; an unguided chain afterwards -- also after a failing guided call --
    equals the unguided baseline bit for bit."""
    m = hip_model()
    c = golden("chain_mesh_guided_b4_s20.npz")
    args, kw = _batch(c)
    base = m.sample_diffusion(*args, **kw)
    for use_graph in (True, False):
        r = m.sample_diffusion(*args, **kw, use_graph=use_graph, use_mesh_data=_data(), grad_step=int(c["grad_step"]),
                               guide_draws=T(c["draws"], DEV))
        e_pos, e_cond = maxabs(r["pos"], c["pos"]), maxabs(torch.stack(r["pos_cond_traj"]), c["pos_cond_traj"])
        record("mesh_guided_chain_golden", use_graph=use_graph, pos_end=e_pos, pos_cond_traj=e_cond)
        assert np.array_equal(r["v"].cpu().numpy(), c["v"])
        assert np.array_equal(torch.stack(r["v_traj"]).numpy(), c["v_traj"])
        assert e_pos < POS_TOL and e_cond < POS_TOL
    r0 = m.sample_diffusion(*args, **kw)
    assert torch.equal(r0["pos"], base["pos"]) and maxabs(r0["pos"], c["pos"]) > 1e-3
    with pytest.raises(Exception):
        m.sample_diffusion(*args, **dict(kw, num_steps=2000), use_mesh_data=_data(), grad_step=int(c["grad_step"]))
    r1 = m.sample_diffusion(*args, **kw)
    assert torch.equal(r1["pos"], base["pos"])


def test_mesh_takes_precedence_over_pointcloud():
    m = hip_model()
    c = golden("chain_mesh_guided_b4_s20.npz")
    args, kw = _batch(c)
    _, _, cloud = _mesh()
    gk = dict(use_mesh_data=_data(), grad_step=int(c["grad_step"]), guide_draws=T(c["draws"], DEV))
    a = m.sample_diffusion(*args, **kw, **gk)
    b = m.sample_diffusion(*args, **kw, **gk, use_pointcloud_data=(cloud, None, 0.2))
    assert torch.equal(a["pos"], b["pos"]) and torch.equal(a["v"], b["v"])


def test_mesh_too_few_inside_raises_value_error():
    """A mesh that holds fewer than 3 atoms: ValueError (as the reference's KD-tree), from the function and from the chain;
    the context stays usable."""
    from shapemol_amd import mesh_shape_guidance
    m = hip_model()
    c = golden("chain_mesh_guided_b4_s20.npz")
    args, kw = _batch(c)
    base = m.sample_diffusion(*args, **kw)
    verts, _, _ = _mesh()
    far = verts + 100.0
    pred = T(golden("mesh_guidance_fn.npz")["pred"].copy(), DEV)
    before = pred.clone()
    with pytest.raises(ValueError):
        mesh_shape_guidance(_data(far), pred, seed=1)
    assert torch.equal(pred, before)
    for use_graph in (True, False):
        with pytest.raises(ValueError):
            m.sample_diffusion(*args, **kw, use_graph=use_graph, use_mesh_data=_data(far), grad_step=int(c["grad_step"]))
    r = m.sample_diffusion(*args, **kw)
    assert torch.equal(r["pos"], base["pos"])


def test_mesh_guidance_driver():
    """sample_diffusion_ligand(use_mesh_data=..., grad_step=...): the same molecules with pipeline 1 and 2, and more of the
    final atoms inside the mesh than in the unguided run with the same seed."""
    from shapemol_amd.sampling import sample_diffusion_ligand
    m = hip_model()
    verts, faces, cloud = _mesh()
    shape_emb = synth.synthetic_batch(1, seed=3)["shape"].reshape(-1, 3)

    def run(pipeline, mesh):
        torch.manual_seed(77)                                # the initial positions and atom types come from torch's generator
        return sample_diffusion_ligand(m, shape_emb, num_samples=6, batch_size=3, device=DEV, num_steps=1000, seed=5,
                                       sample_num_atoms="size", sample_func=lambda n: [14] * n, pipeline=pipeline,
                                       use_mesh_data=(_TrimeshLike(verts, faces), cloud, None) if mesh else None,
                                       use_mesh_gap=0.3, grad_step=0)
    a, b, u = run(1, True), run(2, True), run(2, False)
    for i in (0, 1):
        assert all(np.array_equal(x, y) for x, y in zip(a[i], b[i]))
    tables = M.MeshTables(verts, faces)
    frac_g = M.contains_parity(tables, np.concatenate(a[0])).mean()
    frac_u = M.contains_parity(tables, np.concatenate(u[0])).mean()
    record("mesh_guidance_driver", inside_guided=float(frac_g), inside_unguided=float(frac_u))
    print(f"fraction of final atoms inside the mesh: guided {frac_g:.3f}, unguided {frac_u:.3f}")
    assert frac_g > frac_u
