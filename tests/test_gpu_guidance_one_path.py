"""The single-cloud and single-mesh forms of shape guidance run as a set of ONE group that spans the batch (DESIGN.md sections 10,
12, 13).  Small cases of what that changes for them: the group's atoms come from a per-workgroup table without a batch vector
(N = 1, 15, 16, 17: a lone atom, a partly empty last workgroup, exactly one more workgroup), the LDS tile behind the cloud gets
the groups' 32-byte rounding (clouds of 199 and 511 points), and a set that spans "whatever batch comes" must follow a change
of the batch.  References: tests/mesh_oracle.py and the oracle's pointcloud_shape_guidance, which the grouped tests use too.
Run on the GPU box:  pytest tests/test_gpu_guidance_one_path.py -m gpu"""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_oracle as M
from mesh_multi_util import CHAINS, atom_ranges, chain_batch, meshes
from util import O, T, golden, hash_noise, hip_model, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 15, 16, 17)


def _moved(a, b):
    return (np.asarray(a) != np.asarray(b)).any(1)


def _same(got, ref, pred):
    """The existing function tests' comparison, at error 0: the same atoms moved, to the same float32 positions."""
    assert np.array_equal(_moved(got, pred), _moved(ref, pred))
    assert float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()) == 0.0


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _guide_points(entry, ctx, pos, draws):
    from shapemol_amd import _lib
    p, d = T(pos.copy(), DEV), T(np.ascontiguousarray(draws), DEV)
    _lib.check(entry(ctx, C.c_void_p(p.data_ptr()), len(p), C.c_void_p(d.data_ptr()), C.c_uint64(0),
                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), "guide")
    torch.cuda.synchronize()
    return p.cpu().numpy()


def _cloud_case():
    c = golden("chain_guided_multi_b6_s20.npz")
    return c["clouds"][c["cloud_off"][0]:c["cloud_off"][1]].copy(), float(c["radii"][0]), c["fn_pred"], c["draws"][0]


def _mesh_case():
    """Group 1 of the grouped mesh fixture (73 atoms of fn_pred, 512-point cloud) as a single mesh."""
    c = golden(CHAINS[0])
    verts, faces, cloud = meshes()[1]
    _, off = atom_ranges(chain_batch(c)["counts"], c["group_mols"])
    lo, hi = int(off[1]), int(off[2])
    return verts, np.ascontiguousarray(faces.astype(np.int32)), cloud, c["fn_pred"][lo:hi], c["draws"][0][:, lo:hi]


@pytest.mark.parametrize("n", SIZES)
def test_cloud_atom_counts(n):
    """pointcloud_shape_guidance and shapemol_set_guidance + shapemol_guide_points on the first n atoms of fn_pred (every one of
    them is pulled) against the oracle on the recorded draws."""
    import shapemol_amd
    from shapemol_amd import _lib
    cloud, radius, pred, draws = _cloud_case()
    pred, draws = pred[:n], np.ascontiguousarray(draws[:, :n])
    ref = np.asarray(O.pointcloud_shape_guidance(cloud, radius, pred.copy(), draws))
    assert _moved(ref, pred).sum() == n
    got = shapemol_amd.pointcloud_shape_guidance((cloud, None, radius), T(pred.copy(), DEV), draws=T(draws, DEV)).cpu().numpy()
    _same(got, ref, pred)
    lib, ctx = _lib.load(), hip_model()._context(torch.device(DEV))
    _lib.check(lib.shapemol_set_guidance(ctx, _vp(cloud), len(cloud), radius, 0, None), "set")
    try:
        _same(_guide_points(lib.shapemol_guide_points, ctx, pred, draws), ref, pred)
    finally:
        _lib.check(lib.shapemol_set_guidance(ctx, None, 0, 0.0, 0, None), "unset")


# slices of the group's fn_pred in which the oracle finds >= 3 within-atoms and pulls 3 atoms (checked on the CPU: 8 / 8 / 9
# within-atoms).  With one atom there cannot be three: the lone atom [1:2] is itself a within-atom, nothing is to be pulled and
# nothing moves (the oracle and the reference's KD-tree do not raise then); the lone atom [0:1] is not, and both raise.
@pytest.mark.parametrize("lo,n", [(1, 1), (0, 1), (0, 15), (0, 16), (0, 17)])
def test_mesh_atom_counts(lo, n):
    """mesh_shape_guidance and shapemol_set_mesh_guidance + shapemol_guide_points_mesh on n atoms against tests/mesh_oracle.py on
    the recorded draws."""
    import shapemol_amd
    from shapemol_amd import _lib
    verts, faces, cloud, pred, draws = _mesh_case()
    pred, draws = pred[lo:lo + n], np.ascontiguousarray(draws[:, lo:lo + n])
    data = ((verts, faces), cloud, None)
    lib, ctx = _lib.load(), hip_model()._context(torch.device(DEV))
    try:
        st = {}
        ref = M.mesh_shape_guidance(verts, faces, cloud, pred, draws, stats=st)
    except M.TooFewWithin:
        assert n == 1
        pos = T(pred.copy(), DEV)
        with pytest.raises(_lib.MeshGuidanceError):
            shapemol_amd.mesh_shape_guidance(data, pos, draws=T(draws, DEV))
        assert np.array_equal(pos.cpu().numpy(), pred)
        # the context-bound pair on the same atom: status flag 6 is raised and the position stays
        _lib.check(lib.shapemol_set_mesh_guidance(ctx, _vp(verts), len(verts), _vp(faces), len(faces), _vp(cloud), len(cloud), 0, None), "set")
        try:
            assert np.array_equal(_guide_points(lib.shapemol_guide_points_mesh, ctx, pred, draws), pred)
            flags = (C.c_int32 * 8)()
            assert lib.shapemol_status(ctx, flags) != 0 and flags[_lib.ST_MESH] == 1
            assert not any(flags[i] for i in range(8) if i != _lib.ST_MESH)
        finally:
            _lib.check(lib.shapemol_set_mesh_guidance(ctx, None, 0, None, 0, None, 0, 0, None), "unset")
        return
    assert (st["n_within"] >= 3 and _moved(ref, pred).sum() == 3) if n > 1 else (st["n_within"] == 1 and not _moved(ref, pred).any())
    got = shapemol_amd.mesh_shape_guidance(data, T(pred.copy(), DEV), draws=T(draws, DEV)).cpu().numpy()
    _same(got, ref, pred)
    _lib.check(lib.shapemol_set_mesh_guidance(ctx, _vp(verts), len(verts), _vp(faces), len(faces), _vp(cloud), len(cloud), 0, None), "set")
    try:
        _same(_guide_points(lib.shapemol_guide_points_mesh, ctx, pred, draws), ref, pred)
        flags = (C.c_int32 * 8)()
        assert lib.shapemol_status(ctx, flags) == 0 and not flags[_lib.ST_MESH]
    finally:
        _lib.check(lib.shapemol_set_mesh_guidance(ctx, None, 0, None, 0, None, 0, 0, None), "unset")


@pytest.mark.parametrize("points", (199, 511))
def test_single_mesh_with_odd_cloud_sizes(points):
    """A single-mesh call with a cloud of 199 / 511 points (24 P bytes is then no multiple of 32: the tile behind the cloud starts
    at the rounded-up offset) against the oracle, on all 73 atoms of the group."""
    import shapemol_amd
    verts, faces, cloud, pred, draws = _mesh_case()
    cloud = np.ascontiguousarray(cloud[:points])
    ref = M.mesh_shape_guidance(verts, faces, cloud, pred, draws)
    assert _moved(ref, pred).sum() > 25
    got = shapemol_amd.mesh_shape_guidance(((verts, faces), cloud, None), T(pred.copy(), DEV), draws=T(np.ascontiguousarray(draws), DEV)).cpu().numpy()
    _same(got, ref, pred)


@pytest.mark.parametrize("slot", (0, 1))
def test_a_refused_guided_chain_leaves_the_context_unguided(slot):
    """A tuple-form mesh chain that the library refuses AFTER its set (and the caller's draws pointer) has been installed --
    num_steps = T + 1 is an error return of shapemol_sample, before any launch -- takes the set out again: the same unguided
    chain before and after it is bit-equal on that context, and runs the same launch forms."""
    from shapemol_amd import _lib
    m = hip_model()
    bb = synth.synthetic_batch(2, seed=11)
    n, steps_max = len(bb["batch"]), int(m.num_timesteps)
    args = (T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(2, -1))
    plain = dict(num_steps=2, center_pos_mode="none", seed=9, _slot=slot)

    def forms():
        rec = np.zeros(8, np.int64)
        assert _lib.load().shapemol_debug_read(m._context(torch.device(DEV), slot), b"launch", _vp(rec), rec.nbytes) == rec.nbytes
        return rec.tolist()
    first = m.sample_diffusion(*args, **plain)
    first_forms = forms()
    verts, faces, cloud, _, _ = _mesh_case()
    draws = torch.zeros((steps_max + 1, 5, n), dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.ShapeMolLibraryError, match="num_steps out of range"):
        m.sample_diffusion(*args, num_steps=steps_max + 1, center_pos_mode="none", seed=9, _slot=slot, return_traj=False,
                           use_mesh_data=((verts, faces), cloud, None), guide_draws=draws)
    del draws
    again = m.sample_diffusion(*args, **plain)
    assert torch.equal(again["pos"], first["pos"]) and torch.equal(again["v"], first["v"])
    assert forms() == first_forms


def _chain_inputs(name, n_mols=None):
    """The fixture's batch, or its first n_mols molecules as a batch of their own (with their per-atom noise)."""
    c = golden(name)
    B, S = int(c["B"]), int(c["S"])
    bb = synth.synthetic_batch(B, seed=int(c["seed"]))
    eps, u = hash_noise(len(bb["batch"]), S, int(c["seed"]))
    if n_mols is not None:
        n = int(np.sum(bb["counts"][:n_mols]))
        bb = dict(init_pos=bb["init_pos"][:n], init_v=bb["init_v"][:n], batch=bb["batch"][:n], shape=bb["shape"][:n_mols])
        eps, u, B = np.ascontiguousarray(eps[:, :n]), np.ascontiguousarray(u[:, :n]), n_mols
    args = (T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1))
    return c, args, dict(num_steps=S, center_pos_mode="none", noise=(T(eps, DEV), T(u, DEV)), seed=9, grad_step=int(c["grad_step"]))


def _equal(a, b):
    return torch.equal(a["pos"], b["pos"]) and torch.equal(a["v"], b["v"]) and \
        torch.equal(torch.stack(a["pos_cond_traj"]), torch.stack(b["pos_cond_traj"]))


@pytest.mark.parametrize("kind", ("cloud", "mesh"))
def test_whole_batch_set_follows_the_batch(kind):
    """Stale sets: a tuple-form chain of B = 4 and then one of B = 2 on the same context equals the B = 2 chain of a fresh context
    (no n_mols check trips, no table of the earlier chain is reused).  The tuple form installs a one-group set per chain with
    n_mols = B, so that half covers the per-chain table only; the `whole` set -- one group that spans whatever batch comes -- is
    covered by the C ABI half, where shapemol_set_guidance / shapemol_set_mesh_guidance leave ONE set installed across both chains."""
    from shapemol_amd import _lib
    m = hip_model()
    if kind == "cloud":
        name = "chain_guided_b4_s20.npz"
        c = golden(name)
        cloud = np.ascontiguousarray(c["cloud"])
        guide = dict(use_pointcloud_data=(cloud, None, float(c["radius"])))
        install = lambda lib, ctx: lib.shapemol_set_guidance(ctx, _vp(cloud), len(cloud), float(c["radius"]), int(c["grad_step"]), None)      # noqa: E731
        clear = lambda lib, ctx: lib.shapemol_set_guidance(ctx, None, 0, 0.0, 0, None)      # noqa: E731
    else:
        name = "chain_mesh_guided_b4_s20.npz"
        c, mf = golden(name), golden("mesh_fixture.npz")
        verts, faces, cloud = mf["verts"], np.ascontiguousarray(mf["faces"].astype(np.int32)), mf["cloud"]
        guide = dict(use_mesh_data=((verts, faces), cloud, None))
        install = lambda lib, ctx: lib.shapemol_set_mesh_guidance(ctx, _vp(verts), len(verts), _vp(faces), len(faces), _vp(cloud), len(cloud),      # noqa: E731
                                                                  int(c["grad_step"]), None)
        clear = lambda lib, ctx: lib.shapemol_set_mesh_guidance(ctx, None, 0, None, 0, None, 0, 0, None)      # noqa: E731
    _, args4, kw4 = _chain_inputs(name)
    _, args2, kw2 = _chain_inputs(name, 2)
    a4 = m.sample_diffusion(*args4, **kw4, **guide)
    a2 = m.sample_diffusion(*args2, **kw2, **guide)                   # the same context, after B = 4
    fresh = m.sample_diffusion(*args2, **kw2, **guide, _slot=3)       # a context that has seen no other chain
    plain = m.sample_diffusion(*args2, **kw2)
    assert _equal(a2, fresh) and not torch.equal(a2["pos"], plain["pos"])
    # the C ABI: one installed set, two batch sizes, against the tuple form (device Philox draws on the same seed)
    lib, ctx = _lib.load(), m._context(torch.device(DEV))
    _lib.check(install(lib, ctx), "set")
    try:
        b4 = m.sample_diffusion(*args4, **{k: v for k, v in kw4.items() if k != "grad_step"})
        b2 = m.sample_diffusion(*args2, **{k: v for k, v in kw2.items() if k != "grad_step"})
    finally:
        _lib.check(clear(lib, ctx), "unset")
    assert _equal(b4, a4) and _equal(b2, a2)
    assert _equal(m.sample_diffusion(*args2, **kw2), plain)           # and nothing stays installed
