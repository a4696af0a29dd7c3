"""Molecular surfaces on the device (shapemol_amd/mol_surface.py, csrc/sm_mol_surface.h) against the float64 numpy oracle of the
same rule (tests/mol_surface_oracle.py).  Run on the GPU box:  pytest tests/test_gpu_mol_surface.py -m gpu

Every fixture is first checked on the host, through the oracle: min |fA|, |g| over the nodes >= 1e-9 and min |d - p| over the
erosion candidates >= 1e-9, so that no node's side depends on rounding -- a condition on the inputs, not a tolerance on the
kernels.  One kind of candidate is exempt and counted instead: an exact tie d == p where the spacing is a power of two and the
squared node offset a perfect square (p = 0.5, h = 0.25: the offset (2, 0, 0)); h sqrt(m) is then exact in any IEEE arithmetic,
g is exactly 0 on the device and in the oracle, and the rule puts g >= 0 outside.  The erosion cases the rule is tested at
(p = 0.5, h = 0.25 and the stencil boundary (p + h) / h integer) cannot avoid such ties.
With that the faces equal the oracle's exactly and the vertices agree within 1e-12 * max |coordinate|."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mesh_oracle as M  # noqa: E402
import mol_surface_oracle as O  # noqa: E402
from util import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHIFT = np.array([0.013, 0.027, 0.041])
LINE = (np.array([[0.0, 0.0, 0.0], [1.25, 0.25, 0.25], [2.5, 0.5, 0.5]]) + SHIFT, np.array([1.7, 1.5, 1.2]))
_cache = {}


def _oracle(c, r, p, h, scaling=1.0):
    """The oracle's mesh of a fixture (computed once), after the fixture's margins are asserted."""
    key = (np.asarray(c, np.float64).tobytes(), np.asarray(r, np.float64).tobytes(), p, h, scaling)
    if key not in _cache:
        v, f, fld = O.get_mesh(c, r, p, h, scaling)
        node, dp, ties = O.margins(fld, p * scaling, h)
        print(f"fixture: grid {fld['n'].tolist()}, {len(v)} vertices, {len(f)} faces, min |field| {node:.3e}, min |d - p| {dp:.3e}, exact ties {ties}")
        assert node >= 1e-9 and dp >= 1e-9
        _cache[key] = (v, f, fld, ties)
    return _cache[key]


def _device(mols, p, h, scaling=1.0, details=False):
    from shapemol_amd.mol_surface import get_mesh_batch
    return get_mesh_batch(mols, p, scaling, h, device=DEV, details=details)


def _same(got, want):
    (v, f), (wv, wf) = got, want[:2]
    assert f.dtype == np.int32 and v.dtype == np.float64
    assert f.shape == wf.shape and np.array_equal(f, wf)
    assert v.shape == wv.shape
    err = float(np.abs(v - wv).max())
    print(f"max vertex error {err:.3e}, bound {1e-12 * np.abs(wv).max():.3e}")
    assert err <= 1e-12 * np.abs(wv).max()


def test_one_atom_without_a_probe():
    """The smallest grid (19^3 at h = 0.25), p = 0: g = fA, no erosion kernel."""
    (c, r) = O.SPHERE
    want = _oracle(c, r, 0.0, 0.25)
    assert want[2]["n"].tolist() == [19, 19, 19]
    _same(_device([(c, r)], 0.0, 0.25)[0], want)


@pytest.mark.parametrize("p, ratio_is_integer", [(0.5, True), (0.75, True), (0.6, False)])
def test_erosion_across_tiles(p, ratio_is_integer):
    """Three atoms in a line, h = 0.25.  p = 0.5: a stencil of 3 nodes and a grid of 33 x 25 x 25 nodes, one more than a multiple
    of the 8-node erosion tile in every axis, the surface crossing tile faces in all of them.  p = 0.5 and 0.75 sit on the
    stencil-radius boundary ((p + h) / h = 3, 4); p = 0.6 has no exact tie."""
    from shapemol_amd import mol_surface as MS
    c, r = LINE
    h = 0.25
    want = _oracle(c, r, p, h)
    fld = want[2]
    assert (float((p + h) / h).is_integer()) == ratio_is_integer and O.stencil(p, h) == (3 if p == 0.5 else 4)
    assert (want[3] > 0) == ratio_is_integer
    if p == 0.5:
        assert MS.sizes().tile == O.TILE and all(int(n) % O.TILE == 1 for n in fld["n"])
        cut = (fld["g"][:-1] < 0) != (fld["g"][1:] < 0)                      # cut x-edges: some leave a tile, in every tile layer
        assert cut[O.TILE - 1::O.TILE].any() and ((fld["g"][:, :-1] < 0) != (fld["g"][:, 1:] < 0))[:, O.TILE - 1::O.TILE].any()
    _same(_device([(c, r)], p, h)[0], want)


def test_scan_boundaries():
    """One molecule whose 300763 nodes make 294 scan blocks -- more than the 256 the per-molecule scan takes per pass, so both the
    vertex and the triangle count cross a block boundary of both scan levels -- and one whose vertex and triangle counts (14
    and 24: one node inside) are both below one wave of 64."""
    from shapemol_amd import mol_surface as MS
    z = MS.sizes()
    assert (z.scan_block, z.scan_width) == (O.SCAN_BLOCK, 256)
    big = _oracle(*O.SPHERE, 0.0, 0.055)
    nodes = int(np.prod(big[2]["n"]))
    assert -(-nodes // z.scan_block) > z.scan_width and len(big[0]) > z.scan_block and len(big[1]) > z.scan_block
    small_mol = (np.array([[0.01, 0.02, 0.03]]), np.array([0.2]))
    small = _oracle(*small_mol, 0.0, 0.25)
    assert 0 < len(small[0]) < 64 and 0 < len(small[1]) < 64 and int(np.prod(small[2]["n"])) <= z.scan_block
    _same(_device([O.SPHERE], 0.0, 0.055)[0], big)
    _same(_device([small_mol], 0.0, 0.25)[0], small)


def _ragged():
    from shapemol_amd.mol_surface import radii_of
    bb = synth.synthetic_batch(4, seed=3)
    o = np.cumsum([0, 1, 2, 9, 27, 9])
    pos, types = bb["init_pos"].astype(np.float64), bb["init_v"]
    return [(pos[o[i]:o[i + 1]], radii_of(atom_types=types[o[i]:o[i + 1]])) for i in range(5)]


def test_ragged_batch_is_deterministic():
    """Molecules of 1, 2, 9, 27 and 9 atoms with Bondi radii by type, p = 0.5, h = 0.4: every molecule of the batch equals its
    own single call bit for bit, in any order of the batch, in two runs -- and the oracle."""
    mols, p, h = _ragged(), 0.5, 0.4
    batch = _device(mols, p, h)
    again = _device(mols, p, h)
    order = [3, 0, 4, 2, 1]
    shuffled = _device([mols[i] for i in order], p, h)
    for b, m in enumerate(mols):
        alone = _device([m], p, h)[0]
        for other in (batch[b], again[b], shuffled[order.index(b)]):
            assert np.array_equal(alone[0], other[0]) and np.array_equal(alone[1], other[1])
        _same(alone, _oracle(*m, p, h))
    assert len({len(v) for v, _ in batch}) == 5


def test_device_mesh_is_valid_on_its_own():
    """Without the oracle's mesh: closed and oriented, outward normals, every vertex inside the grid box, and the device's own
    node field, re-interpolated linearly at the vertices, is 0 within 1e-9."""
    mols, p, h = _ragged()[2:4], 0.5, 0.4
    meshes, info = _device(mols, p, h, details=True)
    assert set(info["stage_ms"]) == {"field", "erode", "count", "scan", "verts", "faces"}
    for b, (v, f) in enumerate(meshes):
        lo, n, g = info["lo"][b], info["dims"][b], info["field"][b]
        assert O.closed_and_oriented(f) and O.volume(v, f) > 0
        assert f.min() == 0 and f.max() == len(v) - 1
        assert (v >= lo).all() and (v <= lo + h * (n - 1)).all()
        assert (g[[0, 1, -2, -1]] >= 0).all() and (g[:, [0, 1, -2, -1]] >= 0).all() and (g[:, :, [0, 1, -2, -1]] >= 0).all()
        res = float(np.abs(O.interpolate(g, lo, h, v)).max())
        print(f"molecule {b}: {len(v)} vertices, max |g| at the vertices {res:.3e}")
        assert res <= 1e-9


def test_mesh_feeds_shape_data_and_mesh_guidance():
    """A 20-atom molecule's mesh, as returned, through shape_data.build_batch (whose first step is shapemol_sdata_check) and
    through mesh_shape_guidance: every atom centre is inside and stays, points r_max + p + 3h beyond the bounding box are
    outside and are pulled in, exactly as the guidance oracle moves them."""
    from shapemol_amd import mesh_shape_guidance
    from shapemol_amd.mol_surface import get_mesh, radii_of
    from shapemol_amd.shape_data import build_batch
    bb = synth.synthetic_batch(4, seed=3)
    pos, types = bb["init_pos"][:20].astype(np.float64), bb["init_v"][:20]
    r, p, h = radii_of(atom_types=types), 0.5, 0.4
    _oracle(pos, r, p, h)
    verts, faces = get_mesh(pos, radii=r, probe_radius=p, spacing=h, device=DEV)
    out = build_batch([(verts, faces)], 64, 16, device=DEV, seed=1)
    assert out["cloud"].shape == (1, 64, 3) and torch.isfinite(out["points"]).all() and int(out["counts"].sum()) == 48
    far = r.max() + p + 3 * h
    lo, hi = pos.min(0) - far, pos.max(0) + far
    outside = np.array([[lo[0], lo[1], lo[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], lo[2]], [hi[0], lo[1], hi[2]]])
    pred = np.concatenate([pos, outside]).astype(np.float32)
    cloud = np.full((4, 3), 1000.0)                                            # nowhere near: only containment decides
    tables = M.MeshTables(verts, faces)
    inside = M.contains_parity(tables, pred)
    assert inside[:20].all() and not inside[20:].any()
    draws = np.full((5, len(pred)), 0.95)
    want = M.mesh_shape_guidance(verts, faces, cloud, pred, draws, tables)
    got = mesh_shape_guidance(((verts, faces), cloud, None), torch.from_numpy(pred.copy()).to(DEV), draws=torch.from_numpy(draws).to(DEV)).cpu().numpy()
    assert np.array_equal(got[:20], pred[:20])                                 # reported inside: not touched
    assert (got[20:] != pred[20:]).any(1).all()                                # reported outside: pulled in
    assert np.abs(got - want).max() <= 1e-6
    assert M.contains_parity(tables, got[20:].astype(np.float64)).all()


def test_limits_are_errors_and_the_context_survives():
    from shapemol_amd.mol_surface import get_mesh_batch
    c, r = O.SPHERE
    before = _device([(c, r)], 0.0, 0.25)[0]
    with pytest.raises(ValueError, match=r"molecule 1: the grid exceeds 2097152 nodes"):
        get_mesh_batch([(c, r), (np.array([[0.0, 0.0, 0.0], [40.0, 40.0, 40.0]]), [1.7, 1.7])], 0.0, spacing=0.25, device=DEV)
    with pytest.raises(ValueError, match="molecule 1: no atoms"):
        get_mesh_batch([(c, r), (np.zeros((0, 3)), [])], 0.0, spacing=0.25, device=DEV)
    after = _device([(c, r)], 0.0, 0.25)[0]
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    _same(after, _oracle(c, r, 0.0, 0.25))


def test_c_abi_refused_batch_and_device_inputs():
    """shapemol_msurf_build itself, past the Python module's check: a refused batch (a grid over the cap; then a molecule without
    atoms) returns 1 with the documented message before any kernel runs and leaves nothing to copy; the same context then builds
    a valid batch whose centres and radii are DEVICE pointers (inputs_on_device = 1), equal to the host-input path bit for bit."""
    import ctypes as C
    from shapemol_amd import _lib
    lib = _lib.load()
    vp = lambda a: C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    ctx = C.c_void_p()
    _lib.check(lib.shapemol_msurf_create(0, C.byref(ctx)), "create")
    try:
        def build(off, cen, rad, on_device, p, h):
            counts = np.full((len(off) - 1, 2), -1, np.int32)
            rc = lib.shapemol_msurf_build(ctx, len(off) - 1, vp(off), vp(cen), vp(rad), on_device, p, h, 1.0, vp(counts), None, None, None, stream)
            return rc, counts

        def fetch(counts):
            nv, nf = int(counts[:, 0].sum()), int(counts[:, 1].sum())
            v, f = np.empty((nv, 3), np.float64), np.empty((nf, 3), np.int32)
            _lib.check(lib.shapemol_msurf_copy(ctx, 0, vp(v), 3 * nv, stream), "copy")
            _lib.check(lib.shapemol_msurf_copy(ctx, 1, vp(f), 3 * nf, stream), "copy")
            return v, f

        c, r = LINE
        off = np.array([0, 3], np.int64)
        rc, counts = build(off, np.ascontiguousarray(c), r, 0, 0.6, 0.25)
        assert rc == 0
        want = fetch(counts)
        # refused inside build: the second molecule's grid is over 128^3 nodes; then a molecule without atoms
        wide = np.concatenate([c, [[0.0, 0.0, 0.0], [40.0, 40.0, 40.0]]])
        rc, counts = build(np.array([0, 3, 5], np.int64), wide, np.concatenate([r, [1.7, 1.7]]), 0, 0.0, 0.25)
        assert rc == 1 and "molecule 1: the grid exceeds 2097152 nodes" in lib.shapemol_last_error().decode() and (counts == -1).all()
        dummy = np.empty(3, np.float64)
        assert lib.shapemol_msurf_copy(ctx, 0, vp(dummy), 3, stream) == 1                 # nothing from a refused build
        rc, counts = build(np.array([0, 3, 3], np.int64), np.ascontiguousarray(c), r, 0, 0.6, 0.25)
        assert rc == 1 and "molecule 1: no atoms" in lib.shapemol_last_error().decode()
        # the next batch on the same context, inputs on the device
        dc, dr = torch.from_numpy(np.ascontiguousarray(c)).to(DEV), torch.from_numpy(r).to(DEV)
        rc, counts = build(off, dc, dr, 1, 0.6, 0.25)
        assert rc == 0, lib.shapemol_last_error().decode()
        got = fetch(counts)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        _same(got, _oracle(c, r, 0.6, 0.25))
        # refused device inputs: offsets that do not start at 0
        rc, _ = build(np.array([1, 3], np.int64), dc, dr, 1, 0.6, 0.25)
        assert rc == 1
    finally:
        lib.shapemol_msurf_destroy(ctx)


def test_scaling():
    """scaling = 2 at spacing h gives twice the mesh of the unscaled call at h / 2."""
    c, r = LINE
    p, h = 0.6, 0.5
    scaled = _device([(c, r)], p, h, scaling=2.0)[0]
    plain = _device([(c, r)], p, h / 2)[0]
    assert np.array_equal(scaled[1], plain[1])
    assert np.abs(scaled[0] / 2 - plain[0]).max() <= 1e-12
    _same(scaled, _oracle(c, r, p, h, 2.0))
