"""Test-local oracle of the shape-data builder (shapemol_amd/csrc/sm_shape_data.h) in numpy float64: for fed draws every stage
is restated operation for operation (same association, no fused multiply-adds), on the helpers of tests/mesh_oracle.py.

    host_tables   face areas 0.5 |(B - A) x (C - A)|, their sequential running sum, the vertex bounding box
    surface_cloud the face of every point by the cdf rule, pytorch3d's barycentric formula, rounded to float32
    candidates    ((u * ((hi - lo) + 2)) + lo) - 1
    centre        the float64 sum of the float32 cloud in the kernel's fixed order (256 strided partial sums, folded in halves)
    select        the first n_in inside and the first n_out outside candidates in candidate order
    build         all of it for one mesh
and the small closed meshes the tests use.
"""
import numpy as np

import mesh_oracle as M


def host_tables(verts, faces):
    verts, faces = np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    A, B, C = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    e1, e2 = B - A, C - A
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    area = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    cdf = np.add.accumulate(area)                      # sequential: cdf[k] = cdf[k - 1] + area[k]
    return dict(A=A, B=B, C=C, area=area, cdf=cdf, lo=verts.min(0), hi=verts.max(0))


def surface_cloud(tab, draws):
    """draws (P,3) -> (float32 cloud (P,3), face index (P,), float64 points, weights (P,3))."""
    draws = np.asarray(draws, dtype=np.float64)
    u0, u1, u2 = draws[:, 0], draws[:, 1], draws[:, 2]
    cdf = tab["cdf"]
    k = np.minimum(np.searchsorted(cdf, u0 * cdf[-1], side="right"), len(cdf) - 1)    # first k with cdf[k] > x
    s = np.sqrt(u1)
    w0, w1, w2 = 1.0 - s, s * (1.0 - u2), s * u2
    p = (w0[:, None] * tab["A"][k] + w1[:, None] * tab["B"][k]) + w2[:, None] * tab["C"][k]
    return p.astype(np.float32), k, p, np.stack([w0, w1, w2], 1)


def candidates(tab, draws):
    draws = np.asarray(draws, dtype=np.float64)
    return ((draws * ((tab["hi"] - tab["lo"]) + 2.0)) + tab["lo"]) - 1.0


def centre(cloud32):
    """float32 mean of the float32 cloud: thread t sums the points t, t + 256, ... in order, the partial sums fold in halves."""
    c = np.asarray(cloud32, dtype=np.float32).astype(np.float64)
    part = np.zeros((256, 3))
    for j in range(0, len(c), 256):
        rows = c[j:j + 256]
        part[:len(rows)] = part[:len(rows)] + rows
    s = 128
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return (part[0] / float(len(c))).astype(np.float32)


def select(flags, T):
    flags = np.asarray(flags, dtype=bool)
    tot_in = int(flags.sum())
    n_in = min(T // 2, tot_in)
    n_out = T - n_in
    idx_in, idx_out = np.where(flags)[0][:n_in], np.where(~flags)[0][:n_out]
    return np.concatenate([idx_in, idx_out]), n_in, n_out, (tot_in, len(flags) - tot_in)


def build(verts, faces, cloud_draws, query_draws=None, T=0, loss_type="signed_distance"):
    """One mesh.  `short` says that the outside candidates cannot fill their rows (the builder raises ValueError there)."""
    verts = np.asarray(verts, dtype=np.float64)
    tab = host_tables(verts, faces)
    cloud32, face_idx, _, _ = surface_cloud(tab, cloud_draws)
    off = centre(cloud32)
    off64 = off.astype(np.float64)
    out = dict(cloud32=cloud32, face_idx=face_idx, centres=off, cloud=cloud32 - off,
               bounds=np.stack([(tab["lo"] - off64).astype(np.float32), (tab["hi"] - off64).astype(np.float32)], 1))
    if T:
        cand = candidates(tab, query_draws)
        flags = M.contains_parity(M.MeshTables(verts, faces), cand)
        dist = M.nearest_dist(cloud32.astype(np.float64), cand)
        sel, n_in, n_out, counts = select(flags, T)
        sign = np.concatenate([np.ones(n_in), -np.ones(len(sel) - n_in)])
        if loss_type == "occupancy":
            values = (sign > 0).astype(np.float32)
        else:
            values = (sign * dist[sel]).astype(np.float32)
        out.update(cand=cand, flags=flags, dist=dist, sel=sel, n_in=n_in, n_out=n_out, counts=counts, short=counts[1] < n_out,
                   points=(cand[sel] - off64).astype(np.float32), values=values)
    return out


# ---- meshes ------------------------------------------------------------------------------------------------------------
def tetrahedron(edge=0.5, centre_at=(0.3, -0.2, 0.1)):
    s = edge / (2.0 * np.sqrt(2.0))
    v = s * np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) + np.asarray(centre_at)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)
    return v, _outward(v, f)


def box(size, lo=(0.0, 0.0, 0.0)):
    """Axis-aligned cube of edge `size`, 12 faces."""
    c = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)]) * size + np.asarray(lo)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.int32)
    return c, _outward(c, f)


def pillbox(height=1e-6):
    """A closed mesh of 4 faces of which face 0 holds half the area (to ~ height^2): a big triangle with an apex barely above
    its centroid."""
    v = np.array([[0.0, 0.0, 0.0], [6.0, 0.0, 0.0], [0.0, 6.0, 0.0], [2.0, 2.0, height]])
    f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int32)
    return v, _outward(v, f)


def _outward(v, f):
    c = v.mean(0)
    f = f.copy()
    for i, (a, b, d) in enumerate(f):
        n = np.cross(v[b] - v[a], v[d] - v[a])
        if np.dot(n, v[a] - c) < 0:
            f[i] = (a, d, b)
    return f


# sphere_union_mesh parameters (r1, r2, distance of the centres, h) whose face counts lie just below, at and just above the
# 512-face tile of the classify kernel (kMeshFaceTile); found by a scan on the CPU, asserted by the tests
TILE_PARAMS = {508: (0.87, 0.89, 1.12, 0.498), 512: (0.92, 0.71, 0.93, 0.443), 520: (0.82, 0.87, 0.76, 0.446)}
_tile_cache = {}


def tile_mesh(n_faces):
    if n_faces not in _tile_cache:
        r1, r2, d, h = TILE_PARAMS[n_faces]
        _tile_cache[n_faces] = M.sphere_union_mesh([(0.1, 0.2, -0.1), (0.1 + d, 0.25, 0.05)], [r1, r2], h)
    return _tile_cache[n_faces]


def draws(shape, seed):
    """Uniforms in [0, 1) with 53 random bits, as the fed tables hold them."""
    return np.random.RandomState(seed).random_sample(shape)


def u_mesh():
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_fixture.npz"))
    return g["verts"], g["faces"]


# ---- the fed-draw cases of tests/test_gpu_shape_data.py (the CPU suite checks the oracle on the same) ----------------------
# name -> (mesh names, P, T, loss type, shapes that reuse the draws of an earlier shape {shape: earlier shape})
FED_CASES = {
    "tetra": (["tetra"], 17, 341, "signed_distance", {}),                 # few candidates inside: n_in < T // 2
    "tile508": (["tile508"], 1, 2, "signed_distance", {}),
    "tile512": (["tile512"], 16, 5, "signed_distance", {}),
    "tile512_big": (["tile512"], 2048, 128, "signed_distance", {}),       # the cloud limit: the classify kernel's largest LDS (64 KB)
    "tile520": (["tile520"], 17, 341, "signed_distance", {}),
    "umesh": (["umesh"], 512, 341, "signed_distance", {}),
    "umesh_occupancy": (["umesh"], 16, 5, "occupancy", {}),
    "batch3": (["tile508", "umesh", "tetra"], 17, 341, "signed_distance", {}),          # three face counts: the CSR offsets
    "batch3_twice": (["tile520", "tetra", "tile520"], 16, 5, "signed_distance", {2: 0}),   # the two copies give identical rows
}
_case_cache = {}


def named_mesh(name):
    if name == "tetra":
        return tetrahedron()
    if name == "umesh":
        return u_mesh()
    if name.startswith("tile"):
        return tile_mesh(int(name[4:]))
    raise KeyError(name)


def fed_case(name):
    """(meshes, P, T, loss type, cloud_draws (B,P,3), query_draws (B,3T,3), [oracle result per shape]); computed once."""
    if name not in _case_cache:
        names, P, T, loss, same = FED_CASES[name]
        seed = 1000 + sorted(FED_CASES).index(name)
        meshes = [named_mesh(n) for n in names]
        cd, qd = draws((len(meshes), P, 3), seed), draws((len(meshes), 3 * T, 3), seed + 500)
        for b, src in same.items():
            cd[b], qd[b] = cd[src], qd[src]
        res = [build(v, f, cd[b], qd[b], T, loss) for b, (v, f) in enumerate(meshes)]
        for r in (cd, qd):
            r.setflags(write=False)
        _case_cache[name] = (meshes, P, T, loss, cd, qd, res)
    return _case_cache[name]


def short_case():
    """The error path: [tetrahedron, 40 A cube], T = 341.  (40 / 42)^3 = 0.86 of the cube's candidates fall inside, about 0.41 T
    outside, and its outside rows need at least T / 2.  -> (meshes, P, T, cloud_draws, query_draws)"""
    meshes = [tetrahedron(), box(40.0)]
    return meshes, 16, 341, draws((2, 16, 3), 1), draws((2, 3 * 341, 3), 2)


WINDING_MARGIN, WINDING_SKIP_CAP = 0.4, 0.02


def winding_check(verts, faces, points, flags):
    """(fraction of points outside the margin |winding - 0.5| > 0.4, all the others agree with `flags`)."""
    w = winding_number(verts, faces, points)
    clear = np.abs(w - 0.5) > WINDING_MARGIN
    return float((~clear).mean()), bool(np.array_equal(np.asarray(flags, dtype=bool)[clear], (w > 0.5)[clear]))


winding_number = M.winding_number
