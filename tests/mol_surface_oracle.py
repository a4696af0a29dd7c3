"""Float64 numpy restatement of the molecular-surface rule of DESIGN.md section 20 (csrc/sm_mol_surface.h), operation for
operation: the grid, the inflated field fA, the probe erosion g, marching tetrahedra on the six Kuhn tetrahedra of every cell,
vertices in (node linear index, edge class) order and faces in (cell linear index, tetrahedron, triangle) order.  Nodes are
numbered with the LAST axis fastest: node (a, b, c) of an (nx, ny, nz) grid has linear index (a * ny + b) * nz + c.

Also the checks the tests share: closed and consistently oriented, enclosed volume (divergence theorem), area, and the margins
min |field| over the nodes and min |d - p| over the erosion candidates that tell whether a node's side can depend on rounding.
"""
import itertools

import numpy as np

# corner k of a cell sits at the lower node + (k & 1, k >> 1 & 1, k >> 2 & 1); an edge's class follows from the bits in which
# its two corners differ: the three axes, the three face diagonals, the body diagonal
EDGE_UPPER = (1, 2, 4, 3, 5, 6, 7)                       # class -> corner at the edge's upper end (its lower end is corner 0)
EDGE_CLASS = {d: k for k, d in enumerate(EDGE_UPPER)}
MAX_NODES = 128 ** 3                                     # kMsurfMaxNodes
MAX_ATOMS = 1024                                         # kMsurfMaxAtoms
MAX_STENCIL = 16                                         # kMsurfMaxStencil
SCAN_BLOCK = 1024                                        # kMsurfScanBlock
TILE = 8                                                 # kMsurfTile


def _corner(k):
    return np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1], np.float64)


def kuhn_tets():
    """The six tetrahedra 0 -> e_i -> e_i + e_j -> 7 of a cell, one per order (i, j, k) of the axes in lexicographic order, each
    with its two middle corners swapped where needed so that det(v1 - v0, v2 - v0, v3 - v0) > 0."""
    tets = []
    for perm in itertools.permutations(range(3)):
        v = [0, 1 << perm[0], (1 << perm[0]) | (1 << perm[1]), 7]
        if np.linalg.det(np.stack([_corner(v[i]) - _corner(v[0]) for i in (1, 2, 3)])) < 0:
            v[1], v[2] = v[2], v[1]
        tets.append(tuple(v))
    return tuple(tets)


def _even(p):
    return sum(p[i] > p[j] for i in range(4) for j in range(i + 1, 4)) % 2 == 0


def tri_table():
    """For a positively oriented tetrahedron and the set of its corners with g < 0 (bit i of the case: corner i inside): the
    triangles, each three edges (i, j) of the tetrahedron, normals pointing from g < 0 to g >= 0.
    One corner a inside, (a, b, c, d) an even permutation: (ab, ac, ad); one corner a outside: (ab, ad, ac); two corners a < b
    inside, (a, b, c, d) even: the quadrilateral ac, ad, bd, bc as (ac, ad, bd) and (ac, bd, bc)."""
    table = []
    for case in range(16):
        inside = [i for i in range(4) if case >> i & 1]
        outside = [i for i in range(4) if not case >> i & 1]
        tris = []
        if len(inside) in (1, 3):
            a = inside[0] if len(inside) == 1 else outside[0]
            rest = [i for i in range(4) if i != a]
            b, c, d = next(p for p in itertools.permutations(rest) if _even((a,) + p))
            tris = [((a, b), (a, c), (a, d))] if len(inside) == 1 else [((a, b), (a, d), (a, c))]
        elif len(inside) == 2:
            a, b = inside
            c, d = next(p for p in itertools.permutations(outside) if _even((a, b) + p))
            tris = [((a, c), (a, d), (b, d)), ((a, c), (b, d), (b, c))]
        # the orientation, checked on the unit tetrahedron with every vertex at its edge's midpoint
        ref = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
        for tri in tris:
            q = [(ref[i] + ref[j]) / 2 for i, j in tri]
            assert np.dot(np.cross(q[1] - q[0], q[2] - q[0]), ref[outside].mean(0) - ref[inside].mean(0)) > 0, (case, tri)
        table.append(tuple(tris))
    return tuple(table)


KUHN = kuhn_tets()
TRI = tri_table()


def grid(centres, radii, p, h):
    """(lo (3,), n (3,) int) of the rule's grid."""
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    rmax = float(np.max(np.asarray(radii, np.float64)))
    lo = np.empty(3)
    n = np.empty(3, np.int64)
    for k in range(3):
        lo[k] = (c[:, k].min() - (rmax + p)) - 2.0 * h
        n[k] = int(np.ceil(((((c[:, k].max() + rmax) + p) + 2.0 * h) - lo[k]) / h)) + 1
    return lo, n


def node_coords(lo, n, h):
    ax = [lo[k] + h * np.arange(n[k], dtype=np.float64) for k in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1)


def inflated_field(centres, radii, p, lo, n, h):
    x = node_coords(lo, n, h)
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    r = np.asarray(radii, np.float64)
    f = np.full(x.shape[:3], np.inf)
    for i in range(len(c)):
        d = x - c[i]
        f = np.minimum(f, np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) - (r[i] + p))
    return f


def stencil(p, h):
    return int(np.ceil((p + h) / h))


def erosion_m(outside, R):
    """Per node the smallest squared node offset di^2 + dj^2 + dk^2 to a node of `outside` within R nodes each way (a large
    number where there is none)."""
    big = 3 * R * R + 1
    m = np.full(outside.shape, big, np.int64)
    nx, ny, nz = outside.shape
    pad = np.zeros((nx + 2 * R, ny + 2 * R, nz + 2 * R), bool)
    pad[R:R + nx, R:R + ny, R:R + nz] = outside
    for di in range(-R, R + 1):
        for dj in range(-R, R + 1):
            for dk in range(-R, R + 1):
                s = di * di + dj * dj + dk * dk
                hit = pad[R + di:R + di + nx, R + dj:R + dj + ny, R + dk:R + dk + nz]
                m = np.where(hit & (s < m), s, m)
    return m, big


def field(centres, radii, p, h):
    """dict(lo, n, fA, g, m): the grid, both fields, and the erosion's squared offsets (None when p == 0)."""
    lo, n = grid(centres, radii, p, h)
    fA = inflated_field(centres, radii, p, lo, n, h)
    if p == 0:
        return dict(lo=lo, n=n, fA=fA, g=fA, m=None)
    R = stencil(p, h)
    m, big = erosion_m(fA >= 0, R)
    d = h * np.sqrt(m.astype(np.float64))
    d = np.where(m == big, p + h, d)
    g = p - np.minimum(d, p + h)
    return dict(lo=lo, n=n, fA=fA, g=g, m=np.where(m == big, -1, m))


def margins(fld, p, h):
    """(min |fA| and |g| over the nodes, min |d - p| over the erosion candidates that are no exact tie, number of exact ties).
    A candidate is every node's nearest-outside distance d = h sqrt(m).  An exact tie is d == p bit for bit with m a perfect
    square and h a power of two: then h sqrt(m) is exact in any IEEE arithmetic and the node's side (g = 0: outside) does not
    depend on rounding either."""
    node = float(min(np.abs(fld["fA"]).min(), np.abs(fld["g"]).min() if p == 0 else np.inf))
    if p == 0:
        return node, np.inf, 0
    m = fld["m"][fld["m"] >= 0]
    ms = np.unique(m)
    d = h * np.sqrt(ms.astype(np.float64))
    root = np.rint(np.sqrt(ms.astype(np.float64))).astype(np.int64)
    exact = (d == p) & (root * root == ms) & (np.frexp(h)[0] == 0.5)
    free = np.abs(d[~exact] - p)
    return node, float(free.min()) if free.size else np.inf, int(np.isin(m, ms[exact]).sum())


def triangulate(g, lo, h):
    """(verts (V,3) float64, faces (F,3) int32) of the zero level of the node field g."""
    g = np.asarray(g, np.float64)
    nx, ny, nz = g.shape
    inside = g < 0
    lin = np.arange(nx * ny * nz, dtype=np.int64).reshape(nx, ny, nz)
    off = [tuple(int(v) for v in _corner(k)) for k in range(8)]

    def shifted(a, o, fill):
        out = np.full(a.shape, fill, a.dtype)
        out[:nx - o[0], :ny - o[1], :nz - o[2]] = a[o[0]:, o[1]:, o[2]:]
        return out

    # vertices: per node the cut edges among its seven classes
    cut = np.zeros((nx, ny, nz, 7), bool)
    t = np.zeros((nx, ny, nz, 7))
    for k, up in enumerate(EDGE_UPPER):
        o = off[up]
        exists = np.zeros((nx, ny, nz), bool)
        exists[:nx - o[0], :ny - o[1], :nz - o[2]] = True
        g1 = shifted(g, o, 1.0)
        cut[..., k] = exists & (inside != (g1 < 0))
        with np.errstate(divide="ignore", invalid="ignore"):
            t[..., k] = np.where(cut[..., k], g / (g - g1), 0.0)
    flat = cut.reshape(-1, 7)
    vid = (np.cumsum(flat.reshape(-1)) - flat.reshape(-1)).reshape(-1, 7)          # exclusive scan in (node, class) order
    x0 = node_coords(lo, (nx, ny, nz), h).reshape(-1, 3)
    node_ix, cls = np.nonzero(flat)
    th = t.reshape(-1, 7)[node_ix, cls] * h
    verts = x0[node_ix].copy()
    for k in range(3):
        on = np.array([off[EDGE_UPPER[c]][k] for c in range(7)], bool)[cls]
        verts[on, k] = x0[node_ix[on], k] + th[on]
    # faces: per cell, tetrahedron, triangle
    cell = np.zeros((nx, ny, nz), bool)
    cell[:nx - 1, :ny - 1, :nz - 1] = True
    cells = np.nonzero(cell.reshape(-1))[0]
    corner_lin = np.stack([shifted(lin, off[k], -1).reshape(-1)[cells] for k in range(8)], 1)       # (cells, 8)
    corner_in = np.stack([shifted(inside, off[k], False).reshape(-1)[cells] for k in range(8)], 1)
    rows = []                                                # (cell position, tet, tri, v0, v1, v2)
    for ti, tet in enumerate(KUHN):
        case = sum(corner_in[:, tet[i]].astype(np.int64) << i for i in range(4))
        for cs in range(1, 15):
            sel = np.nonzero(case == cs)[0]
            if not sel.size:
                continue
            for tri_i, tri in enumerate(TRI[cs]):
                ids = []
                for (i, j) in tri:
                    a, b = min(tet[i], tet[j]), max(tet[i], tet[j])
                    assert a & b == a
                    ids.append(vid[corner_lin[sel, a], EDGE_CLASS[a ^ b]])
                rows.append(np.stack([sel, np.full(len(sel), ti), np.full(len(sel), tri_i)] + ids, 1))
    if rows:
        rows = np.concatenate(rows)
        rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
        faces = rows[:, 3:].astype(np.int32)
    else:
        faces = np.zeros((0, 3), np.int32)
    return verts, faces


def get_mesh(centres, radii, p, h, scaling=1.0):
    """(verts, faces, field dict) of one molecule under the rule; `scaling` multiplies centres, radii and the probe radius."""
    c = np.asarray(centres, np.float64).reshape(-1, 3) * scaling
    r = np.asarray(radii, np.float64) * scaling
    fld = field(c, r, p * scaling, h)
    v, f = triangulate(fld["g"], fld["lo"], h)
    return v, f, fld


# ---- checks ---------------------------------------------------------------------------------------------------------------------
def closed_and_oriented(faces):
    """Every undirected edge is shared by exactly two faces, which run through it in opposite directions."""
    f = np.asarray(faces, np.int64)
    if len(f) == 0:
        return False
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    if (e[:, 0] == e[:, 1]).any():
        return False
    big = int(f.max()) + 1
    directed = e[:, 0] * big + e[:, 1]
    if len(np.unique(directed)) != len(directed):
        return False                                        # a directed edge twice: two faces run the same way
    reverse = e[:, 1] * big + e[:, 0]
    return bool(np.array_equal(np.sort(directed), np.sort(reverse)))


def volume(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def area(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)


def interpolate(g, lo, h, pts):
    """g re-interpolated linearly inside the Kuhn tetrahedron that holds each point (the interpolant marching tetrahedra cuts)."""
    g = np.asarray(g, np.float64)
    u = (np.asarray(pts, np.float64) - lo) / h
    base = np.clip(np.floor(u).astype(np.int64), 0, np.array(g.shape) - 2)
    fr = u - base
    out = np.empty(len(u))
    for q in range(len(u)):
        order = np.argsort(-fr[q], kind="stable")              # the largest fraction first: the path 0 -> e_i -> e_i + e_j -> 7
        a = base[q].copy()
        val = g[tuple(a)]
        for k in order:
            b = a.copy()
            b[k] += 1
            val += fr[q, k] * (g[tuple(b)] - g[tuple(a)])
            a = b
        out[q] = val
    return out


def sphere_union_volume(r1, r2, d):
    """Volume of the union of two spheres whose centres are d apart."""
    v = 4.0 / 3.0 * np.pi * (r1 ** 3 + r2 ** 3)
    if d >= r1 + r2:
        return v
    if d <= abs(r1 - r2):
        return 4.0 / 3.0 * np.pi * max(r1, r2) ** 3
    lens = np.pi * (r1 + r2 - d) ** 2 * (d * d + 2 * d * (r1 + r2) - 3 * (r1 - r2) ** 2) / (12 * d)
    return v - lens


# ---- fixtures and the table of profiles/mol_surface/oracle_convergence.txt ----------------------------------------------------
SPHERE = (np.array([[0.1, 0.2, 0.3]]), np.array([1.7]))
TWO_SPHERES = (np.array([[0.0, 0.0, 0.0], [2.6, 0.0, 0.0]]), np.array([1.7, 1.5]))
THREE_ATOMS = (np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [3.0, 0.1, 0.0]]), np.array([1.7, 1.5, 1.2]))
SKIMAGE_FIXTURES = {"sphere_p0_h0.25": (SPHERE, 0.0, 0.25), "two_spheres_p0.6_h0.25": (TWO_SPHERES, 0.6, 0.25),
                    "three_atoms_p0.7_h0.2": (THREE_ATOMS, 0.7, 0.2)}


def convergence_table(hs=(0.5, 0.25, 0.125)):
    """[(h, relative volume error, relative area error)] of the sphere r = 1.7, p = 0."""
    r = float(SPHERE[1][0])
    rows = []
    for h in hs:
        v, f, _ = get_mesh(*SPHERE, 0.0, h)
        rows.append((h, abs(volume(v, f) - 4 / 3 * np.pi * r ** 3) / (4 / 3 * np.pi * r ** 3), abs(area(v, f) - 4 * np.pi * r * r) / (4 * np.pi * r * r)))
    return rows
