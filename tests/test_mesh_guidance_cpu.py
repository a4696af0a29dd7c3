"""Mesh shape guidance without a GPU: the fixtures of tests/golden/make_golden_mesh.py are well formed, the test-local oracle
(tests/mesh_oracle.py) reproduces the reference's function from the recorded draws, its ray parity agrees with the winding
number, and the package and the C header expose the feature."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import mesh_oracle as M  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")


def _load(name):
    return np.load(os.path.join(GOLDEN, name))


def test_mesh_fixtures_well_formed():
    m = _load("mesh_fixture.npz")
    verts, faces, cloud = m["verts"], m["faces"], m["cloud"]
    assert verts.dtype == np.float64 and faces.dtype == np.int32 and cloud.shape == (512, 3)
    assert len(faces) >= 1000 and faces.min() >= 0 and faces.max() < len(verts)
    assert M.check_closed(faces)
    ext = verts.max(0) - verts.min(0)
    assert 8.0 < ext.max() < 12.0                                   # molecule size
    assert abs(M.winding_number(verts, faces, [[0.0, -1.5, 0.0]])[0] - 1.0) < 1e-9     # outward orientation
    f = _load("mesh_guidance_fn.npz")
    n = len(f["pred"])
    assert f["pred"].dtype == np.float32 and f["pred"].shape == (n, 3) and f["out"].shape == (n, 3) and f["draws"].shape == (5, n)
    c = _load("chain_mesh_guided_b4_s20.npz")
    S = int(c["S"])
    assert c["draws"].shape[:2] == (S, 5) and int(c["guided_steps"]) == 999 - int(c["grad_step"])
    for d in (f["draws"], c["draws"]):
        assert (d >= 0).all() and (d < 1).all()


def test_oracle_reproduces_reference_function():
    m, f = _load("mesh_fixture.npz"), _load("mesh_guidance_fn.npz")
    stats = {}
    out = M.mesh_shape_guidance(m["verts"], m["faces"], m["cloud"], f["pred"], f["draws"], stats=stats)
    assert np.array_equal(out, f["out"])
    # the sets the fixture must exercise
    acc = np.array(list(stats["accepted_at"].values()))
    assert stats["contained"].any() and (~stats["contained"]).any() and stats["near_cloud_inside"].any()
    assert (acc == 0).any() and (acc >= 1).any() and len(stats["never"])
    never = stats["never"]
    assert np.array_equal(out[never], f["pred"][never])              # never accepted: original position


def test_ray_parity_equals_winding_number_on_a_grid():
    m = _load("mesh_fixture.npz")
    verts, faces = m["verts"], m["faces"]
    lo, hi = verts.min(0) - 1.0, verts.max(0) + 1.0
    ax = [np.linspace(lo[k], hi[k], 23) + 0.0137 * (k + 1) for k in range(3)]
    pts = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    w = M.winding_number(verts, faces, pts)
    keep = np.abs(w - np.round(w)) < 1e-6                            # drop points on the surface (none expected)
    assert keep.mean() > 0.999
    par = M.contains_parity(M.MeshTables(verts, faces), pts[keep])
    assert np.array_equal(par, np.round(w[keep]) == 1)
    assert 0.05 < par.mean() < 0.6


def test_package_and_header_expose_mesh_guidance():
    import shapemol_amd
    from shapemol_amd import _lib, molopt_score_model
    assert shapemol_amd.mesh_shape_guidance is molopt_score_model.mesh_shape_guidance
    assert hasattr(molopt_score_model.ScorePosNet3D, "mesh_shape_guidance")
    assert issubclass(_lib.MeshGuidanceError, ValueError)
    header = open(os.path.join(ROOT, "include", "shapemol_hip.h")).read()
    declared = set(re.findall(r"\b(shapemol_[a-z_]+)\s*\(", header))
    new = {"shapemol_set_mesh_guidance", "shapemol_guide_points_mesh", "shapemol_mesh_guidance"}
    assert new <= declared and new <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 5
