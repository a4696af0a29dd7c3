"""Test-local oracle of mesh shape guidance (the reference's mesh_shape_guidance, models/molopt_score_model.py:742-775) in
numpy float64, and the triangle meshes the fixtures use.

* ``contains_parity``: ray parity with exactly the rule of shapemol_amd/csrc/sm_mesh.h (same projection, same edge functions
  in canonical vertex order, same zero rule, same operation order, no fused multiply-adds).
* ``winding_number``: the generalized winding number (sum of the solid angles of the faces / 4 pi, Van Oosterom & Strackee),
  an independent containment test: the fixtures hold only points where both agree with a margin.
* ``mesh_shape_guidance``: the reference's function restated on these tests and brute-force float64 searches.
* ``sphere_union_mesh``: a closed, consistently oriented triangle mesh of a union of spheres by marching tetrahedra.
"""
import numpy as np

ROT = np.array([[0.8, -0.6, 0.0], [0.36, 0.48, -0.8], [0.48, 0.64, 0.6]])   # sm_mesh.h kMeshRot


def project(p):
    p = np.asarray(p, dtype=np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return [(ROT[r, 0] * x + ROT[r, 1] * y) + ROT[r, 2] * z for r in range(3)]


class MeshTables:
    """Projected faces as the device image holds them."""

    def __init__(self, verts, faces):
        faces = np.asarray(faces, dtype=np.int64)
        u, v, w = project(verts)
        self.u, self.v, self.w = u[faces], v[faces], w[faces]                   # (F, 3) each
        self.canon = np.stack([faces[:, k] < faces[:, (k + 1) % 3] for k in range(3)], 1)
        self.box = (self.u.min(1), self.u.max(1), self.v.min(1), self.v.max(1))
        self.bounds = (self.u.min(), self.u.max(), self.v.min(), self.v.max(), self.w.max())


def contains_parity(tables, points, chunk=256):
    """Odd number of crossings of the ray along +w (sm_mesh.h's mesh_contains) for every point."""
    t = tables
    qu, qv, qw = project(points)
    out = np.zeros(len(qu), dtype=bool)
    b = t.bounds
    cand = np.where((qu >= b[0]) & (qu <= b[1]) & (qv >= b[2]) & (qv <= b[3]) & (qw <= b[4]))[0]
    for s in range(0, len(cand), chunk):
        idx = cand[s:s + chunk]
        pu, pv, pw = qu[idx, None], qv[idx, None], qw[idx, None]
        inbox = (pu >= t.box[0]) & (pu <= t.box[1]) & (pv >= t.box[2]) & (pv <= t.box[3])
        pi, fi = np.nonzero(inbox)
        pu, pv, pw = qu[idx][pi], qv[idx][pi], qw[idx][pi]
        e, pos = [], []
        for k in range(3):
            a, c = k, (k + 1) % 3
            cn = t.canon[fi, k]
            lo = np.where(cn, a, c)
            hi = np.where(cn, c, a)
            ulo, uhi = t.u[fi, lo], t.u[fi, hi]
            vlo, vhi = t.v[fi, lo], t.v[fi, hi]
            ec = (uhi - ulo) * (pv - vlo) - (vhi - vlo) * (pu - ulo)
            p = ec >= 0.0
            pos.append(np.where(cn, p, ~p))
            e.append(np.where(cn, ec, -ec))
        same = (pos[0] == pos[1]) & (pos[1] == pos[2])
        d = (e[1] * (t.w[fi, 0] - pw) + e[2] * (t.w[fi, 1] - pw)) + e[0] * (t.w[fi, 2] - pw)
        cross = same & np.where(pos[0], d > 0.0, d < 0.0)
        cnt = np.bincount(pi, weights=cross.astype(np.float64), minlength=len(idx)).astype(np.int64)
        out[idx] = (cnt & 1) == 1
    return out


def winding_number(verts, faces, points, chunk=128):
    verts, faces = np.asarray(verts, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    A, B, Cc = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    points = np.asarray(points, dtype=np.float64)
    out = np.empty(len(points))
    for s in range(0, len(points), chunk):
        q = points[s:s + chunk, None, :]
        a, b, c = A[None] - q, B[None] - q, Cc[None] - q
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
        det = np.einsum("pfi,pfi->pf", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("pfi,pfi->pf", a, b) * lc + np.einsum("pfi,pfi->pf", b, c) * la + np.einsum("pfi,pfi->pf", c, a) * lb
        out[s:s + chunk] = 2.0 * np.arctan2(det, den).sum(1) / (4.0 * np.pi)
    return out


def nearest_dist(cloud, points):
    """Distance to the nearest cloud point, computed as sklearn's KD-tree does (sqrt of ((dx^2 + dy^2) + dz^2))."""
    cloud, points = np.asarray(cloud, dtype=np.float64), np.asarray(points, dtype=np.float64)
    best = np.full(len(points), np.inf)
    for s in range(0, len(cloud), 256):
        c = cloud[None, s:s + 256]
        dx, dy, dz = (points[:, None, k] - c[..., k] for k in range(3))
        best = np.minimum(best, ((dx * dx + dy * dy) + dz * dz).min(1))
    return np.sqrt(best)


def knn3(anchor, points):
    """Indices (into `anchor`) of the 3 nearest anchors of every point, ascending distance, ties to the lower index; and the
    squared distances of the 4 nearest (for the tie checks)."""
    anchor = np.asarray(anchor, dtype=np.float64)
    points = np.asarray(points, dtype=np.float64)
    dx, dy, dz = (points[:, None, k] - anchor[None, :, k] for k in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz
    order = np.lexsort((np.broadcast_to(np.arange(len(anchor)), d2.shape), d2), axis=1)[:, :4]
    return order[:, :3], np.take_along_axis(d2, order, 1)


class TooFewWithin(ValueError):
    pass


def mesh_shape_guidance(verts, faces, cloud, pred, draws, tables=None, stats=None):
    """The reference's function (float32 (N,3) `pred`, uniforms `draws` (5,N) by atom) -> float32 (N,3).  `stats`, if a dict,
    receives the sets the fixtures must exercise."""
    t = tables or MeshTables(verts, faces)
    pred = np.asarray(pred, dtype=np.float32)
    contained = contains_parity(t, pred)
    d = nearest_dist(cloud, pred)
    within = pred[contained & (d > 0.4)]
    out_idx = np.where(~contained | (d < 0.2))[0]
    if len(within) == 0 or (len(within) < 3 and len(out_idx)):
        raise TooFewWithin("fewer than 3 within-mesh atoms")
    res = pred.copy()
    pts = pred[out_idx]
    accepted_at = {}
    j = 0
    while len(out_idx) and j < 5:
        nb, _ = knn3(within, pts)
        w = within[nb]                                            # (M, 3, 3) float32
        mean = ((w[:, 0] + w[:, 1]) + w[:, 2]) / np.float32(3)
        direction = pts - mean                                    # float32 in the first iteration, float64 after
        scalar = draws[j, out_idx][:, None] * 0.8 + 0.2
        new = pts - scalar * direction
        ok = contains_parity(t, new) & (nearest_dist(cloud, new) > 0.2)
        res[out_idx[ok]] = new[ok].astype(np.float32)
        for a in out_idx[ok]:
            accepted_at[int(a)] = j
        out_idx, pts = out_idx[~ok], new[~ok]
        j += 1
    if stats is not None:
        stats.update(contained=contained, near_cloud_inside=contained & (d < 0.2), accepted_at=accepted_at,
                     never=out_idx, n_within=len(within))
    return res


# ---- meshes ------------------------------------------------------------------------------------------------------------
_TETS = [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]    # Freudenthal: 6 tets per cube
# cube corner c = 4 * dx + 2 * dy + dz


def marching_tetrahedra(field, origin, h):
    """Zero level set of the grid function `field` (negative inside, positive on the boundary of the grid) -> (verts, faces),
    every triangle oriented with its normal towards increasing field (outwards)."""
    nx, ny, nz = field.shape
    f = field.ravel()
    gid = np.arange(nx * ny * nz).reshape(nx, ny, nz)
    base = gid[:-1, :-1, :-1].ravel()
    corner = np.array([((c >> 2) & 1) * ny * nz + ((c >> 1) & 1) * nz + (c & 1) for c in range(8)])
    tets = np.concatenate([base[:, None] + corner[list(t)][None, :] for t in _TETS])
    inside = f[tets] < 0
    cnt = inside.sum(1)
    tets = tets[(cnt > 0) & (cnt < 4)]
    coords = lambda g: origin + h * np.stack(np.unravel_index(g, (nx, ny, nz)), -1)   # noqa: E731
    vid, verts, faces = {}, [], []

    def edge_vertex(a, b):
        key = (min(a, b), max(a, b))
        if key not in vid:
            fa, fb = f[a], f[b]
            vid[key] = len(verts)
            verts.append(coords(a) + (fa / (fa - fb)) * (coords(b) - coords(a)))
        return vid[key]

    for tet in tets:
        ins = [g for g in tet if f[g] < 0]
        outs = [g for g in tet if f[g] >= 0]
        if len(ins) == 1 or len(ins) == 3:
            lone, others = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
            tris = [[edge_vertex(lone, o) for o in others]]
        else:
            a, b = ins
            c, d = outs
            p = [edge_vertex(a, c), edge_vertex(a, d), edge_vertex(b, d), edge_vertex(b, c)]
            tris = [[p[0], p[1], p[2]], [p[0], p[2], p[3]]]
        cin = np.mean([coords(g) for g in ins], 0)
        cout = np.mean([coords(g) for g in outs], 0)
        for tri in tris:
            P = [verts[i] for i in tri]
            n = np.cross(P[1] - P[0], P[2] - P[0])
            faces.append(tri if np.dot(n, cout - cin) > 0 else tri[::-1])
    return np.array(verts), np.array(faces, dtype=np.int32)


def sphere_union_mesh(centres, radii, h, seed=0):
    centres, radii = np.asarray(centres, dtype=np.float64), np.asarray(radii, dtype=np.float64)
    lo = (centres - radii[:, None]).min(0) - 2 * h
    hi = (centres + radii[:, None]).max(0) + 2 * h
    n = np.ceil((hi - lo) / h).astype(int) + 1
    g = lo + h * np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), -1)
    field = (np.linalg.norm(g[..., None, :] - centres, axis=-1) - radii).min(-1)
    rng = np.random.RandomState(seed)
    field = field + rng.uniform(-1e-7, 1e-7, field.shape)          # no grid value exactly on the surface
    field[field == 0] = 1e-9
    return marching_tetrahedra(field, lo, h)


def check_closed(faces):
    """Every undirected edge in exactly two faces, every directed edge in one (closed, consistently oriented)."""
    faces = np.asarray(faces, dtype=np.int64)
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    und = np.sort(d, 1)
    _, cu = np.unique(und, axis=0, return_counts=True)
    _, cd = np.unique(d, axis=0, return_counts=True)
    return bool((cu == 2).all() and (cd == 1).all())


def sample_surface(verts, faces, n, seed):
    """n points on the surface, area-weighted (as pytorch3d's sample_points_from_meshes)."""
    verts, faces = np.asarray(verts), np.asarray(faces)
    A, B, Cc = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(B - A, Cc - A), axis=1)
    rng = np.random.RandomState(seed)
    fi = rng.choice(len(faces), n, p=area / area.sum())
    r1, r2 = np.sqrt(rng.random_sample(n)), rng.random_sample(n)
    return (1 - r1)[:, None] * A[fi] + (r1 * (1 - r2))[:, None] * B[fi] + (r1 * r2)[:, None] * Cc[fi]


# the fixture mesh: a U of spheres (non-convex, about 10 A across); the gap of the U is outside
FIXTURE_CENTRES = [(-3.0, -1.5, 0.0), (-1.5, -1.5, 0.3), (0.0, -1.5, 0.0), (1.5, -1.5, -0.3), (3.0, -1.5, 0.0),
                   (-3.0, 0.0, 0.2), (-3.0, 1.5, 0.0), (3.0, 0.0, -0.2), (3.0, 1.5, 0.0), (0.0, -1.0, 1.4)]
FIXTURE_RADII = [1.6, 1.5, 1.6, 1.5, 1.6, 1.5, 1.6, 1.5, 1.6, 1.2]
