"""The molecular-surface rule on the host: its numpy oracle (tests/mol_surface_oracle.py) against analytic
volumes and areas and against skimage's marching cubes, and the host side of shapemol_amd.mol_surface (argument checks, radius
table, no CPU path).  The measured convergence figures are in profiles/mol_surface/oracle_convergence.txt."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mol_surface_oracle as O  # noqa: E402


def test_kuhn_split_and_triangle_table():
    """Six positively oriented tetrahedra that tile the cell, every edge between a corner and one that holds its bits."""
    vol = 0.0
    for tet in O.KUHN:
        assert tet[0] == 0 and tet[3] == 7
        d = np.linalg.det(np.stack([O._corner(tet[i]) - O._corner(tet[0]) for i in (1, 2, 3)]))
        assert d > 0
        vol += d / 6
        for i in range(4):
            for j in range(i + 1, 4):
                a, b = min(tet[i], tet[j]), max(tet[i], tet[j])
                assert a & b == a and (a ^ b) in O.EDGE_CLASS
    assert abs(vol - 1.0) < 1e-12
    assert [len(t) for t in O.TRI] == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]


def test_sphere_is_closed_and_converges():
    """r = 1.7, p = 0: closed and oriented at h = 0.25; the volume and area errors fall as h halves (0.5, 0.25, 0.125)."""
    v, f, fld = O.get_mesh(*O.SPHERE, 0.0, 0.25)
    assert O.closed_and_oriented(f)
    assert O.volume(v, f) > 0                                   # normals point outwards
    assert (v >= fld["lo"]).all() and (v <= fld["lo"] + 0.25 * (fld["n"] - 1)).all()
    assert np.abs(O.interpolate(fld["g"], fld["lo"], 0.25, v[::17])).max() < 1e-12
    rows = O.convergence_table()
    for (h0, v0, a0), (h1, v1, a1) in zip(rows, rows[1:]):
        print(f"h {h0} -> {h1}: volume error {v0:.3e} -> {v1:.3e}, area error {a0:.3e} -> {a1:.3e}")
        assert v1 < v0 and a1 < a0


def test_two_spheres_with_a_probe_lie_between_the_unions():
    """p = 0.5: the eroded surface encloses more than the union of the van-der-Waals spheres and less than the union of the
    inflated ones (both analytic: two spherical caps)."""
    (c, r), p, h = O.TWO_SPHERES, 0.5, 0.25
    v, f, fld = O.get_mesh(c, r, p, h)
    assert O.closed_and_oriented(f)
    d = float(np.linalg.norm(c[1] - c[0]))
    lower, upper = O.sphere_union_volume(r[0], r[1], d), O.sphere_union_volume(r[0] + p, r[1] + p, d)
    vol = O.volume(v, f)
    print(f"vdw union {lower:.4f} < mesh {vol:.4f} < inflated union {upper:.4f}")
    assert lower < vol < upper


def test_empty_and_degenerate_fields():
    """A field without a crossing gives no faces; a node with g == 0 is outside and its cut edges meet at the node."""
    g = np.ones((4, 4, 4))
    v, f = O.triangulate(g, np.zeros(3), 1.0)
    assert len(v) == 0 and len(f) == 0 and not O.closed_and_oriented(f)
    g[1:3, 1:3, 1:3] = -1.0
    g[0, 1, 1] = 0.0
    v, f = O.triangulate(g, np.zeros(3), 1.0)
    assert O.closed_and_oriented(f) and O.volume(v, f) > 0


def test_against_skimage_marching_cubes():
    """Marching cubes of the same node field.  Both triangulations interpolate g linearly along grid edges, so each lies within
    an order-h^2 error of the smooth level set, of the size the oracle's own sphere error e(h) measures at that spacing
    (convergence_table: 1.1 % of the volume, 0.56 % of the area at h = 0.25).  Two such surfaces differ by at most 2 e(h); the
    margin is 4 e(h), a factor 2 for surfaces more curved than the sphere -- volume and area each against their own e(h).  On
    the sphere fixture skimage's mesh must also lie within that margin of the analytic values.  This margin is reasoned:
    skimage is not installed where this was written and the test has not run; profiles/mol_surface/skimage_comparison.txt says
    so, and the margin is to become twice the measured difference once it can be measured."""
    measure = pytest.importorskip("skimage.measure")
    for name, ((c, r), p, h) in O.SKIMAGE_FIXTURES.items():
        (_, ev, ea), = O.convergence_table((h,))
        v, f, fld = O.get_mesh(c, r, p, h)
        sv, sf, _, _ = measure.marching_cubes(fld["g"], level=0.0, spacing=(h, h, h))
        sv = sv + fld["lo"]
        vol, vol_s, ar, ar_s = O.volume(v, f), abs(O.volume(sv, sf)), O.area(v, f), O.area(sv, sf)
        print(f"{name}: volume {vol:.4f} vs {vol_s:.4f} (margin {4 * ev:.4f}), area {ar:.4f} vs {ar_s:.4f} (margin {4 * ea:.4f})")
        assert abs(vol - vol_s) / vol <= 4 * ev
        assert abs(ar - ar_s) / ar <= 4 * ea
        if name.startswith("sphere"):
            rr = float(r[0])
            assert abs(vol_s - 4 / 3 * np.pi * rr ** 3) / (4 / 3 * np.pi * rr ** 3) <= 4 * ev
            assert abs(ar_s - 4 * np.pi * rr * rr) / (4 * np.pi * rr * rr) <= 4 * ea


# ---- the package's host side ------------------------------------------------------------------------------------------------
def test_radius_table_covers_the_vocabularies():
    from shapemol_amd import mol_surface as MS
    assert [len(v) for v in (MS.VOCAB_ELEMENTS[k] for k in ("basic", "add_aromatic", "full"))] == [10, 15, 23]
    for mode, zs in MS.VOCAB_ELEMENTS.items():
        r = MS.radii_of(atom_types=np.arange(len(zs)), mode=mode)
        assert r.shape == (len(zs),) and (r >= 1.2).all() and (r <= 1.98).all()
    assert MS.radii_of(elements=[6, 1, 53]).tolist() == [1.70, 1.20, 1.98]
    with pytest.raises(ValueError):
        MS.radii_of(elements=[6, 34])
    with pytest.raises(ValueError):
        MS.radii_of(atom_types=[15], mode="add_aromatic")


def test_limits_match_the_library():
    """The oracle's copy of the constants against the library's own (the Python module keeps none)."""
    from shapemol_amd import mol_surface as MS
    z = MS.sizes()
    assert (O.MAX_NODES, O.MAX_ATOMS, O.MAX_STENCIL, O.TILE, O.SCAN_BLOCK) == (z.max_nodes, z.max_atoms, z.max_stencil, z.tile, z.scan_block)
    assert z.max_batch_nodes == 2 ** 26 and z.max_mols == 65535 and z.scan_width == 256
    assert 7 * z.max_nodes < 2 ** 31 and 12 * z.max_nodes < 2 ** 31             # int32 holds every vertex and face index
    assert (z.tile + 2 * z.max_stencil) ** 3 <= 64 * 1024 and 32 * z.max_atoms <= 64 * 1024      # the LDS behind two of the limits


def test_argument_validation_needs_no_device():
    from shapemol_amd.mol_surface import get_mesh, get_mesh_batch
    pos = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0]])
    ok = dict(radii=[1.7, 1.5], probe_radius=0.5, spacing=0.25)
    bad = [dict(ok, radii=[1.7, 0.0]), dict(ok, radii=[1.7, -1.0]), dict(ok, radii=[np.nan, 1.5]), dict(ok, probe_radius=-0.1),
           dict(ok, probe_radius=np.nan), dict(ok, spacing=0.0), dict(ok, spacing=np.nan), dict(ok, scaling=0.0), dict(ok, radii=[1.7]),
           dict(ok, spacing=0.01),                      # (4 + 0.04) / 0.01 nodes across: over 128^3
           dict(ok, probe_radius=5.0, spacing=0.25)]    # a stencil of 21 nodes
    for kw in bad:
        with pytest.raises(ValueError):
            get_mesh(pos, **kw)
    with pytest.raises(ValueError):
        get_mesh(np.array([[np.inf, 0.0, 0.0]]), radii=[1.7])
    with pytest.raises(ValueError, match="no atoms"):
        get_mesh_batch([(pos, [1.7, 1.5]), (np.zeros((0, 3)), [])], 0.5, spacing=0.25)
    with pytest.raises(ValueError, match="limit is 1024"):
        get_mesh(np.zeros((1025, 3)), radii=np.ones(1025), spacing=1.0)
    with pytest.raises(ValueError, match="128\\^3"):
        get_mesh(np.array([[0.0, 0, 0], [200.0, 200, 200]]), radii=[1.7, 1.7], spacing=1.0)
    with pytest.raises(ValueError):
        get_mesh(pos)                                   # neither radii nor elements
    with pytest.raises(ValueError):
        get_mesh_batch([])


def test_no_cpu_path():
    from shapemol_amd.mol_surface import get_mesh
    with pytest.raises(RuntimeError, match="no CPU path"):
        get_mesh(np.zeros((1, 3)), elements=[6], probe_radius=0.0, spacing=0.5, device="cpu")
