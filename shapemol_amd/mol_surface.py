"""Molecular surface meshes on the device, from atom coordinates and radii.

``get_mesh`` takes the place of the reference's (utils/shape.py:153-162), which hands an RDKit molecule to oddt's
``generate_surface_marching_cubes``; here the molecule is given as arrays and a batch of molecules goes through six kernels
(csrc/sm_mol_surface.h).  The surface rule is this package's own, not oddt's: a float64 grid field of
the spheres inflated by the probe, eroded by the probe over grid nodes, cut by marching tetrahedra; every mesh is closed,
consistently oriented (normals outwards) and identical from run to run.  How far it lies from oddt's surface has not been
measured: oddt is not available to this project.

Radii: given, or looked up by element in ``VDW_RADII`` -- Bondi's van-der-Waals radii (J. Phys. Chem. 68 (1964) 441) for the
elements of the three atom vocabularies (``basic``, ``add_aromatic``, ``full``: H C N O F P S Cl Br I).  The table is this
package's choice; oddt takes its radii from its own atom typing.

Limits (``ValueError`` before any kernel runs): 1..1024 atoms per molecule, at most 128^3 grid nodes per molecule and 2^26 per
call, ``ceil((probe_radius * scaling + spacing) / spacing) <= 16``.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._native import DeviceContexts, hip_device, host, ptr, stream_ptr

# Bondi (1964), Angstrom, by atomic number
VDW_RADII = {1: 1.20, 6: 1.70, 7: 1.55, 8: 1.52, 9: 1.47, 15: 1.80, 16: 1.80, 17: 1.75, 35: 1.85, 53: 1.98}
# atomic number of every atom-type index of the three vocabularies (utils/transforms.py:11-66 of the reference)
VOCAB_ELEMENTS = {
    "basic": (1, 6, 7, 8, 9, 15, 16, 17, 35, 53),
    "add_aromatic": (1, 6, 6, 7, 7, 8, 8, 9, 15, 15, 16, 16, 17, 35, 53),
    "full": (1, 6, 6, 6, 6, 7, 7, 7, 7, 8, 8, 8, 9, 15, 15, 15, 15, 16, 16, 16, 16, 16, 17),
}
STAGES = ("field", "erode", "count", "scan", "verts", "faces")
Sizes = collections.namedtuple("Sizes", "max_nodes max_batch_nodes max_atoms max_stencil tile scan_block max_mols scan_width")


def sizes():
    """The library's limits and block sizes (shapemol_msurf_sizes; the constants of csrc/sm_mol_surface.h): grid nodes per
    molecule and per call, atoms per molecule, erosion stencil, erosion tile edge, nodes per scan block, molecules per call,
    scan blocks per pass of the per-molecule scan."""
    out = (C.c_int64 * 8)()
    _lib.load().shapemol_msurf_sizes(out, 8)
    return Sizes(*out)


def radii_of(elements=None, atom_types=None, mode="add_aromatic"):
    """Bondi radii (float64) of atoms given by atomic number, or by atom-type index of the vocabulary ``mode``."""
    if (elements is None) == (atom_types is None):
        raise ValueError("give either elements (atomic numbers) or atom_types")
    if elements is None:
        if mode not in VOCAB_ELEMENTS:
            raise ValueError(f"unknown atom vocabulary {mode!r}")
        table = np.asarray(VOCAB_ELEMENTS[mode])
        idx = host(atom_types).astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= len(table)):
            raise ValueError(f"an atom type lies outside the {len(table)} types of {mode!r}")
        elements = table[idx]
    z = host(elements).astype(np.int64).reshape(-1)
    missing = sorted(set(z.tolist()) - set(VDW_RADII))
    if missing:
        raise ValueError(f"no van-der-Waals radius for atomic number(s) {missing}; give radii")
    return np.array([VDW_RADII[int(k)] for k in z], np.float64)


def _pack(mols):
    """[(pos (N,3), radii (N,)), ...] -> host arrays (atom_off int64, centres float64, radii float64)."""
    off, cs, rs = [0], [], []
    for b, (pos, rad) in enumerate(mols):
        c = host(pos).astype(np.float64).reshape(-1, 3)
        r = host(rad).astype(np.float64).reshape(-1)
        if len(r) != len(c):
            raise ValueError(f"molecular surface: molecule {b}: {len(c)} positions and {len(r)} radii")
        cs.append(c)
        rs.append(r)
        off.append(off[-1] + len(c))
    cat = lambda xs, shape: np.ascontiguousarray(np.concatenate(xs)) if off[-1] else np.zeros(shape, np.float64)  # noqa: E731
    return np.asarray(off, np.int64), cat(cs, (1, 3)), cat(rs, (1,))


_contexts = DeviceContexts("shapemol_msurf_create", "shapemol_msurf_destroy")


def _device(device):
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    return hip_device(device, "molecular surfaces are built on a HIP device")


def get_mesh_batch(mols, probe_radius=1.4, scaling=1.0, spacing=None, *, device=None, details=False):
    """Meshes of a list of molecules in one launch sequence.  A molecule is ``(pos, radii)`` or a dict with ``pos`` and
    ``radii`` or ``elements`` (atomic numbers).  Returns a list of ``(verts (V,3) float64, faces (F,3) int32)`` numpy arrays --
    what ``shape_data.build_batch`` and ``use_mesh_data=(mesh, point_clouds, kdtree)`` take as they are.  Centres, radii and the
    probe radius are multiplied by ``scaling`` as the reference's argument does, the vertices stay in those scaled units, and
    ``spacing`` is the grid spacing in them (default 1, i.e. 1 / scaling Angstrom: oddt's unit grid).
    ``details=True`` adds a dict: ``lo (B,3)``, ``dims (B,3)`` of the grids, ``stage_ms`` per kernel stage and ``field``, the
    node field g of every molecule as an (nx, ny, nz) array."""
    pairs = []
    for m in mols:
        if isinstance(m, dict):
            rad = m["radii"] if m.get("radii") is not None else radii_of(elements=m["elements"])
            m = (m["pos"], rad)
        pairs.append(m)
    if not pairs:
        raise ValueError("molecular surface: no molecule given")
    off, cen, rad = _pack(pairs)
    h = 1.0 if spacing is None else float(spacing)
    lib = _lib.load()
    B = len(pairs)
    if lib.shapemol_msurf_check(B, ptr(off), ptr(cen), ptr(rad), float(probe_radius), h, float(scaling)):
        raise ValueError(lib.shapemol_last_error().decode())
    device = _device(device)
    counts = np.zeros((B, 2), np.int32)
    lo, dims, ms = np.zeros((B, 3), np.float64), np.zeros((B, 3), np.int32), np.zeros(6, np.float64)
    ctx = _contexts.of(device)
    with torch.cuda.device(device):
        stream = stream_ptr(device)
        _lib.check(lib.shapemol_msurf_build(ctx, B, ptr(off), ptr(cen), ptr(rad), 0, float(probe_radius), h, float(scaling), ptr(counts),
                                            ptr(lo), ptr(dims), ptr(ms) if details else None, stream), "shapemol_msurf_build")
        nv, nf = int(counts[:, 0].sum()), int(counts[:, 1].sum())
        verts, faces = np.empty((nv, 3), np.float64), np.empty((nf, 3), np.int32)
        _lib.check(lib.shapemol_msurf_copy(ctx, 0, ptr(verts), 3 * nv, stream), "shapemol_msurf_copy")
        _lib.check(lib.shapemol_msurf_copy(ctx, 1, ptr(faces), 3 * nf, stream), "shapemol_msurf_copy")
        field = None
        if details:
            field = np.empty(int(dims.astype(np.int64).prod(1).sum()), np.float64)
            _lib.check(lib.shapemol_msurf_copy(ctx, 2, ptr(field), field.size, stream), "shapemol_msurf_copy")
    vo, fo = np.concatenate([[0], np.cumsum(counts[:, 0])]), np.concatenate([[0], np.cumsum(counts[:, 1])])
    meshes = [(verts[vo[b]:vo[b + 1]].copy(), faces[fo[b]:fo[b + 1]].copy()) for b in range(B)]
    if not details:
        return meshes
    no = np.concatenate([[0], np.cumsum(dims.astype(np.int64).prod(1))])
    return meshes, dict(lo=lo, dims=dims, stage_ms=dict(zip(STAGES, ms.tolist())),
                        field=[field[no[b]:no[b + 1]].reshape(tuple(dims[b])) for b in range(B)])


def get_mesh(pos, radii=None, elements=None, probe_radius=1.4, scaling=1.0, spacing=None, *, device=None):
    """``get_mesh(mol, probe_radius=...)`` of the reference with the molecule as arrays: ``pos (N,3)`` and either ``radii (N,)``
    or ``elements (N,)`` (atomic numbers; Bondi radii).  Returns ``(verts, faces)``; see ``get_mesh_batch``."""
    if radii is None:
        if elements is None:
            raise ValueError("molecular surface: give radii or elements")
        radii = radii_of(elements=elements)
    return get_mesh_batch([(pos, radii)], probe_radius, scaling, spacing, device=device)[0]
