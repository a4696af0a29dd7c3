"""Guidance of a reverse chain on the host side: the parsers that turn the reference's arguments into the arrays the library's
setters take, the plan of one ``sample_diffusion`` call (``_resolve_chain`` -> ``ChainPlan``), the one owner of what a chain
installs into its library context (``_ChainSettings``), and the stand-alone ``pointcloud_shape_guidance`` /
``mesh_shape_guidance`` of the reference's module surface (re-exported by ``molopt_score_model``).
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._native import _check_device_tensor, ptr, stream_ptr


def _field_decoder(shape_AE):
    """The device ``DecoderInner`` behind ``sample_diffusion(shape_AE=...)``."""
    from .shape_autoencoder import DecoderInner, PointCloud_AE
    if shape_AE is None:
        raise ValueError("use_grad=True needs shape_AE: a shapemol_amd.shape_autoencoder.PointCloud_AE or DecoderInner")
    if isinstance(shape_AE, PointCloud_AE):
        return shape_AE.generator
    if isinstance(shape_AE, DecoderInner):
        return shape_AE
    raise TypeError(f"shape_AE is a {type(shape_AE).__module__}.{type(shape_AE).__name__}: gradient shape guidance runs on the device "
                    "auto-encoder -- load its state dict into shapemol_amd.shape_autoencoder.PointCloud_AE and pass that")


def pointcloud_shape_guidance(use_pointcloud_data, pred_ligand_pos, k=3, ratio=0.2, *, draws=None, seed=None):
    """``pointcloud_shape_guidance`` of the reference (module level there too, ``models/molopt_score_model.py:699-740``) as
    one device kernel: atoms of ``pred_ligand_pos`` (N,3) whose ``k`` = 3 nearest cloud points are on average farther than
    ``radius`` are pulled towards their mean by ``u * (0.8 - ratio) + ratio``, up to five times; the tensor is updated in
    place and returned.  ``use_pointcloud_data = (point_clouds, kdtree, radius)`` as there (the KD-tree is not used:
    brute-force float64 search on the device).
    Extensions (keyword-only): ``draws`` (5,N) float64 device tensor = the uniform of every (iteration, atom) (parity
    mode); otherwise device Philox keyed by ``seed`` (default: drawn from numpy's global generator, which the reference's
    function draws its uniforms from)."""
    if k != 3:
        raise NotImplementedError("the device kernel searches the reference's default k = 3 nearest cloud points")
    pos, _, cloud, gd, seed = _standalone_inputs(pred_ligand_pos, draws, seed, lambda: _cloud_array(use_pointcloud_data[0]))
    if pos.shape[0] == 0:
        return pred_ligand_pos
    with torch.cuda.device(pos.device):
        rc = _lib.load().shapemol_pointcloud_guidance(ptr(cloud), cloud.shape[0], float(use_pointcloud_data[2]),
                                                      float(ratio), ptr(pos), pos.shape[0], ptr(gd), C.c_uint64(seed), stream_ptr(pos.device))
    _lib.check(rc, "shapemol_pointcloud_guidance")
    return pred_ligand_pos


def _cfg_groups(entries, bounds, n_mols):
    """The list form of classifier-free guidance, ``[(guide_stren, n_mols), ...]`` with ``bounds`` (B,3,2), (3,2) or None, as the
    arrays shapemol_set_cfg_groups takes: molecule offsets (G+1) int64, strengths (G) float64 and boxes (G,3,2) float64 or None
    (each group's box is the row of its first molecule; a group without molecules gets a NaN row: no clamp).  Host logic only."""
    if not entries:
        raise ValueError("guide_stren: the list of groups is empty")
    off, stren = [0], []
    for i, e in enumerate(entries):
        if not isinstance(e, (tuple, list)) or len(e) != 2:
            raise ValueError(f"guide_stren[{i}] must be (guide_stren, n_mols)")
        w, cnt = float(e[0]), int(e[1])
        if cnt < 0:
            raise ValueError(f"guide_stren[{i}]: n_mols must be >= 0")
        if not np.isfinite(w):
            raise ValueError(f"guide_stren[{i}]: the guidance strength must be finite")
        stren.append(w)
        off.append(off[-1] + cnt)
    if off[-1] != n_mols:
        raise ValueError(f"guide_stren: the groups hold {off[-1]} molecules, the batch has {n_mols}")
    if len(stren) > _lib.CFG_MAX_GROUPS:
        raise ValueError(f"guide_stren: {len(stren)} groups, a chain takes at most {_lib.CFG_MAX_GROUPS}")
    boxes = None
    if bounds is not None:
        bx = bounds.detach().cpu().numpy() if isinstance(bounds, torch.Tensor) else np.asarray(bounds)
        bx = np.asarray(bx, dtype=np.float64)
        if bx.shape == (3, 2):
            boxes = np.ascontiguousarray(np.broadcast_to(bx, (len(stren), 3, 2)))
        elif bx.shape == (n_mols, 3, 2):
            boxes = np.full((len(stren), 3, 2), np.nan)
            for g in range(len(stren)):
                if off[g + 1] > off[g]:
                    boxes[g] = bx[off[g]]
        else:
            raise ValueError("bounds must be a (B, 3, 2) or (3, 2) box")
    return np.asarray(off, dtype=np.int64), np.asarray(stren, dtype=np.float64), boxes


def _guidance_groups(entries, n_mols):
    """``[(point_clouds or None, kdtree, radius, n_mols), ...]`` -> (mol_off (G+1,) int64, clouds (sum P_g, 3) float64, cloud_off
    (G+1,) int64, radii (G,) float64), host arrays for ``shapemol_set_guidance_groups``.  The groups' molecule counts must sum to
    ``n_mols``.  Host logic only: the clouds' sizes and the radii are checked by the library, which names the offending group."""
    if len(entries) == 0:
        raise ValueError("use_pointcloud_data: the list of groups is empty")
    counts, clouds, radii = [], [], []
    for g, e in enumerate(entries):
        if not isinstance(e, (tuple, list)) or len(e) != 4:
            raise ValueError(f"use_pointcloud_data[{g}] must be (point_clouds, kdtree, radius, n_mols)")
        cnt = int(e[3])
        if cnt < 0:
            raise ValueError(f"use_pointcloud_data[{g}]: n_mols < 0")
        counts.append(cnt)
        clouds.append(np.zeros((0, 3)) if e[0] is None else np.asarray(e[0], dtype=np.float64).reshape(-1, 3))
        radii.append(1.0 if e[0] is None else float(e[2]))          # an unguided group's radius is not used
    if sum(counts) != n_mols:
        raise ValueError(f"use_pointcloud_data: the groups hold {sum(counts)} molecules, the batch has {n_mols}")
    mol_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cloud_off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    return mol_off, np.ascontiguousarray(np.concatenate(clouds)), cloud_off, np.asarray(radii, dtype=np.float64)


def _mesh_guidance_groups(entries, n_mols):
    """``[(mesh or None, point_clouds, kdtree, n_mols), ...]`` -> (mol_off, verts (sum V_g, 3) float64, vert_off, faces (sum F_g, 3)
    int32 with indices relative to the group's own vertices, face_off, clouds (sum P_g, 3) float64, cloud_off), offsets (G+1,)
    int64: host arrays for ``shapemol_set_mesh_guidance_groups``.  The groups' molecule counts must sum to ``n_mols``.  Host logic
    only; the library checks the meshes and clouds again and names the offending group."""
    if len(entries) == 0:
        raise ValueError("use_mesh_data: the list of groups is empty")
    counts, verts, faces, clouds = [], [], [], []
    for g, e in enumerate(entries):
        if not isinstance(e, (tuple, list)) or len(e) != 4:
            raise ValueError(f"use_mesh_data[{g}] must be (mesh, point_clouds, kdtree, n_mols)")
        cnt = int(e[3])
        if cnt < 0:
            raise ValueError(f"use_mesh_data[{g}]: n_mols < 0")
        counts.append(cnt)
        v, f, c = (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32), np.zeros((0, 3))) if e[0] is None else _mesh_arrays(tuple(e[:3]))
        verts.append(v), faces.append(f), clouds.append(c)
    if sum(counts) != n_mols:
        raise ValueError(f"use_mesh_data: the groups hold {sum(counts)} molecules, the batch has {n_mols}")
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)        # noqa: E731
    return (np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), np.ascontiguousarray(np.concatenate(verts)), off(verts),
            np.ascontiguousarray(np.concatenate(faces).astype(np.int32)), off(faces), np.ascontiguousarray(np.concatenate(clouds)),
            off(clouds))


def _mesh_groups_error(lib, ctx, n_groups):
    """The MeshGuidanceError of a chain / pass with mesh groups: names the groups that were left unguided and in how many steps
    (``.group_steps``: (G,) int32, from the library's per-group count)."""
    steps = np.zeros(n_groups, dtype=np.int32)
    got = lib.shapemol_debug_read(ctx, b"mesh_group_flags", ptr(steps), steps.nbytes)
    bad = np.nonzero(steps)[0] if got == steps.nbytes else []
    which = ", ".join(f"group {g} in {int(steps[g])} step(s)" for g in bad[:16]) + (" ..." if len(bad) > 16 else "")
    err = _lib.MeshGuidanceError(
        "mesh shape guidance per group of molecules: " + (which or "a group") + " had fewer than 3 atoms inside its mesh and > 0.4 "
        "from its cloud (none at all, or fewer than 3 while atoms are to be pulled) and was left unguided there; the reference "
        "raises ValueError from its KD-tree here.  The other groups were guided; the chain's result is not returned")
    err.group_steps = steps if got == steps.nbytes else None
    return err


def _cloud_array(points):
    return np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))


def _one_group(kind, data, n_mols):
    """The tuple form ``(mesh, point_clouds, kdtree)`` / ``(point_clouds, kdtree, radius)`` as the payload of a set of ONE group
    that spans the batch: the only place where the reference's form becomes the form the library runs.  The tuple's own argument
    checks (and their texts) come first.  What the library itself rejects (a cloud of fewer than 3 or more than 2048 points, a
    radius <= 0, a face that repeats a vertex, a non-finite vertex) is then reported by the groups setter, as "group 0"."""
    if kind == "mesh_groups":
        verts, faces, cloud = _mesh_arrays(data)
        return _mesh_guidance_groups([((verts, faces), cloud, None, n_mols)], n_mols)
    return _guidance_groups([(_cloud_array(data[0]), None, float(data[2]), n_mols)], n_mols)


# setter of each kind of guidance, and the arguments that take the guidance out of the context again
_GUIDANCE = {"mesh_groups": ("shapemol_set_mesh_guidance_groups", (0, None, None, None, None, None, None, None, 0, None)),
             "groups": ("shapemol_set_guidance_groups", (0, None, None, None, None, 0, None))}


def _install_guidance(lib, ctx, kind, payload, grad_step, gd):
    """payload -- "mesh_groups": _mesh_guidance_groups' arrays; "groups": _guidance_groups' arrays."""
    if kind == "mesh_groups":
        mol_off, verts, vert_off, faces, face_off, clouds, cloud_off = payload
        opt = lambda a: ptr(a) if len(a) else None      # noqa: E731
        args = (len(mol_off) - 1, ptr(mol_off), opt(verts), ptr(vert_off), opt(faces), ptr(face_off), opt(clouds), ptr(cloud_off))
    else:
        mol_off, clouds, cloud_off, radii = payload
        args = (len(radii), ptr(mol_off), ptr(clouds) if len(clouds) else None, ptr(cloud_off), ptr(radii))
    _lib.check(getattr(lib, _GUIDANCE[kind][0])(ctx, *args, int(grad_step), ptr(gd)), _GUIDANCE[kind][0])


def _clear_guidance(lib, ctx, kind):
    name, off = _GUIDANCE[kind]
    _lib.check(getattr(lib, name)(ctx, *off), name)


def _standalone_inputs(pred_ligand_pos, draws, seed, payload, batch_ligand=None):
    """Shared head of the stand-alone guidance functions, in the order their errors are raised: the (N, 3) tensor updated in place,
    the batch vector (groups only), ``payload()``'s host arrays, the (5, N) draws, the default seed (numpy's global generator)."""
    pos = _check_device_tensor("pred_ligand_pos", pred_ligand_pos, torch.float32)
    if pos.data_ptr() != pred_ligand_pos.data_ptr() or pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError("pred_ligand_pos must be a contiguous (N, 3) tensor (it is updated in place)")
    batch = None if batch_ligand is None else _check_device_tensor("batch_ligand", batch_ligand, torch.int64)
    arrays = payload()
    gd = None if draws is None else _check_device_tensor("draws", draws, torch.float64)
    bad_draws = gd is not None and tuple(gd.shape) != (5, pos.shape[0])
    if bad_draws or (batch is not None and batch.shape != (pos.shape[0],)):
        raise ValueError("draws must be (5, N) float64" if batch is None else "batch_ligand must be (N,) and draws (5, N) float64")
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 62, dtype=np.int64)) if gd is None else 0
    return pos, batch, arrays, gd, seed


def _mesh_arrays(use_mesh_data):
    """(mesh, point_clouds, kdtree) -> contiguous (V,3) float64 vertices, (F,3) int32 faces, (P,3) float64 cloud.  The mesh is
    duck-typed: ``.vertices`` / ``.faces`` (a ``trimesh.Trimesh``) or a ``(vertices, faces)`` pair."""
    if not isinstance(use_mesh_data, (tuple, list)) or len(use_mesh_data) != 3:
        raise NotImplementedError("use_mesh_data must be (mesh, point_clouds, kdtree), as the reference's sampling script builds it")
    mesh, cloud = use_mesh_data[0], use_mesh_data[1]
    if hasattr(mesh, "vertices") and hasattr(mesh, "faces"):
        verts, faces = mesh.vertices, mesh.faces
    elif isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        verts, faces = mesh
    else:
        raise NotImplementedError(f"a mesh of type {type(mesh).__name__}: give one with .vertices / .faces or a (vertices, faces) pair")
    verts = np.ascontiguousarray(np.asarray(verts, dtype=np.float64))
    faces = np.asarray(faces)
    if verts.ndim != 2 or verts.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3 or len(faces) == 0:
        raise ValueError("the mesh must have (V, 3) vertices and (F >= 1, 3) faces")
    if faces.min() < 0 or faces.max() >= len(verts):
        raise ValueError("a face names a vertex outside [0, V)")
    faces = np.ascontiguousarray(faces.astype(np.int32))
    cloud = cloud.detach().cpu().numpy() if isinstance(cloud, torch.Tensor) else cloud
    return verts, faces, _cloud_array(cloud)


def mesh_shape_guidance(use_mesh_data, pred_ligand_pos, k=3, ratio=0.5, *, draws=None, seed=None):
    """``mesh_shape_guidance`` of the reference (``models/molopt_score_model.py:742-775``) as two device kernels: the atoms of
    ``pred_ligand_pos`` (N,3) inside the mesh and > 0.4 from the cloud anchor the pull; every atom outside the mesh or < 0.2
    from the cloud moves away from the mean of its 3 nearest anchors by ``u * 0.8 + 0.2`` and is accepted once inside the mesh
    and > 0.2 from the cloud, up to five times; atoms never accepted keep their position.  The tensor is updated in place and
    returned.  ``use_mesh_data = (mesh, point_clouds, kdtree)`` as there; the mesh is anything with ``.vertices`` / ``.faces``
    or a ``(vertices, faces)`` pair, the KD-tree is not used (brute-force float64 searches on the device), and ``k`` / ``ratio``
    are ignored, as the reference ignores them.  Containment is the parity of a fixed ray (``csrc/sm_mesh.h``), not trimesh's
    code.  Raises ``ValueError`` (``_lib.MeshGuidanceError``) when fewer than 3 atoms are inside, as the reference's KD-tree.
    Extensions (keyword-only): ``draws`` (5,N) float64 device tensor = the uniform of every (iteration, atom) (parity mode);
    otherwise device Philox keyed by ``seed`` (default: drawn from numpy's global generator)."""
    del k, ratio                 # the reference hard-codes 3 neighbours and the fraction u * 0.8 + 0.2
    pos, _, (verts, faces, cloud), gd, seed = _standalone_inputs(pred_ligand_pos, draws, seed, lambda: _mesh_arrays(use_mesh_data))
    if pos.shape[0] == 0:
        raise _lib.MeshGuidanceError("mesh shape guidance: no atoms inside the mesh (the reference's KDTree of none raises)")
    flag = C.c_int32(0)
    with torch.cuda.device(pos.device):
        rc = _lib.load().shapemol_mesh_guidance(ptr(verts), verts.shape[0], ptr(faces), faces.shape[0], ptr(cloud), cloud.shape[0],
                                                ptr(pos), pos.shape[0], ptr(gd), C.c_uint64(seed), C.byref(flag), stream_ptr(pos.device))
    if rc and flag.value:
        raise _lib.MeshGuidanceError(_lib.load().shapemol_last_error().decode())
    _lib.check(rc, "shapemol_mesh_guidance")
    return pred_ligand_pos


# ---------------------------------------------------------------------------------------------------------- one chain's settings
@dataclass
class ChainPlan:
    """What ``sample_diffusion``'s arguments decide before a tensor is looked at (``_resolve_chain``)."""
    kind: str                    # None / "groups" / "mesh_groups" (the names of _GUIDANCE's rows) / "field" / "cfg"
    payload: tuple               # the cloud / mesh set's host arrays; of a tuple-form set once one_group() knows the batch
    data: object                 # use_mesh_data / use_pointcloud_data of the kind that won
    n_mesh_groups: int           # mesh groups of a list-form chain (their unguided steps go into a MeshGuidanceError)
    cfg_groups: tuple            # _cfg_groups' arrays, or None: the scalar form (guide_stren, cfg_box)
    guide_stren: float
    cfg_p: float
    cfg_box: np.ndarray
    threshold_type: str
    field_dec: object
    grad_lr: float
    grad_step: int
    first_step: int
    num_steps: int
    center_pos_mode: str

    def one_group(self, n_mols):
        if self.payload is None:
            self.payload = _one_group(self.kind, self.data, n_mols)


def _resolve_chain(model, ligand_shape, threshold_type, threshold_args, num_steps, center_pos_mode, use_grad, grad_lr, shape_AE,
                   use_mesh_data, use_pointcloud_data, grad_step, guide_stren, bounds, first_step):
    """``sample_diffusion``'s arguments -> ChainPlan.  Host logic only: no library call, no device allocation; the argument errors
    that need no device tensor are raised here."""
    # gradient shape guidance: behind a mesh and a point cloud in the reference's if / elif, so with either it is not looked at
    field_dec = None
    if use_grad and use_mesh_data is None and use_pointcloud_data is None:
        field_dec = _field_decoder(shape_AE)
        grad_lr = float(grad_lr)
        if not np.isfinite(grad_lr):
            raise ValueError(f"grad_lr must be finite, got {grad_lr}")
    groups = mesh_groups = None
    if isinstance(use_pointcloud_data, list):
        if isinstance(use_mesh_data, list):
            raise NotImplementedError("mesh groups and point-cloud groups in one chain are not supported: give one kind of list")
        if use_mesh_data is not None:
            raise NotImplementedError("mesh guidance takes one mesh per chain")
        groups = _guidance_groups(use_pointcloud_data, int(ligand_shape.shape[0]))
    elif isinstance(use_mesh_data, list):        # (with a single point cloud beside: the mesh wins, the reference's if / elif)
        mesh_groups = _mesh_guidance_groups(use_mesh_data, int(ligand_shape.shape[0]))
    cfg_groups = None
    if isinstance(guide_stren, list):
        cfg_groups = _cfg_groups(guide_stren, bounds, int(ligand_shape.shape[0]))
        if model.cond_mask_prob == 0:
            assert not cfg_groups[1].any()
        guide_stren = float(np.abs(cfg_groups[1]).max()) if cfg_groups[1].any() else 0.0      # (> 0: some group is guided)
    elif model.cond_mask_prob == 0:
        assert guide_stren == 0
    # classifier-free guidance: the reference's branch order (:561-642) -- mesh, point cloud, then CFG
    cfg = use_mesh_data is None and use_pointcloud_data is None and field_dec is None and (model.cond_mask_prob or 0) > 0 and guide_stren > 0.0
    cfg_p, cfg_box = 0.0, None
    if cfg:
        if threshold_type not in _lib.CFG_THRESHOLDS:
            raise ValueError("undefined thresholding strategy: expect one of (reference_threshold, dynamic_threshold, rescale, none) "
                             + "but get %s" % (threshold_type))
        if threshold_type is not None:
            cfg_p = float((threshold_args or {}).get("p", _lib.CFG_DEFAULT_P[threshold_type]))
        if threshold_type == "dynamic_threshold" and not 0.0 <= cfg_p <= 1.0:
            raise RuntimeError(f"quantile() q must be in the range [0, 1] but got {cfg_p}")     # torch.quantile's check
        if bounds is not None and cfg_groups is None:
            bx = bounds.detach().cpu().numpy() if isinstance(bounds, torch.Tensor) else np.asarray(bounds)
            bx = np.asarray(bx, dtype=np.float64)
            if bx.ndim == 3:
                bx = bx[0]               # the box of molecule 0 clamps every atom, as the reference's bounds[0]
            if bx.shape != (3, 2):
                raise ValueError("bounds must be a (B, 3, 2) or (3, 2) box")
            cfg_box = np.ascontiguousarray(bx)
    if center_pos_mode not in (None, "none", "center"):
        raise NotImplementedError(center_pos_mode)       # as center_pos() of the reference (:52-60)
    if num_steps is None:
        num_steps = model.num_timesteps
    print('sample center pos mode: ', center_pos_mode)
    # the kind of set the chain installs (the names of _GUIDANCE's two rows); the mesh wins, as the reference's if / elif
    kind = "mesh_groups" if use_mesh_data is not None else "groups" if use_pointcloud_data is not None else \
        "field" if field_dec is not None else "cfg" if cfg else None
    payload, data = (mesh_groups, use_mesh_data) if kind == "mesh_groups" else (groups, use_pointcloud_data)
    return ChainPlan(kind, payload, data, len(mesh_groups[0]) - 1 if isinstance(use_mesh_data, list) else 0, cfg_groups, guide_stren,
                     cfg_p, cfg_box, threshold_type, field_dec, grad_lr, grad_step, first_step, num_steps, center_pos_mode)


class _ChainSettings:
    """Everything one chain installs into its library context, and the only code that takes it out again.

    ``install`` issues the setters in a fixed order: the cloud / mesh set (with the caller-owned draws pointer), ``first_step``,
    the classifier-free settings (groups or scalars), the field decoder.  Removal has two halves, because the library reads the
    settings at two times:
      * ``clear_enqueued``: ``first_step``, the classifier-free settings and the field decoder are read only while
        ``shapemol_sample`` enqueues the chain, so they go as soon as it has returned (return codes ignored);
      * ``clear_finished``: the cloud / mesh set's device data and the draws are read by the running chain, so the device is
        synchronised first and the set cleared then -- from the chain handle's ``result()`` or ``abandon()``.
    Both halves are idempotent, and each clears exactly what ``install`` got as far as handing to a setter (a setter that failed
    included: its clearing call is harmless), nothing else -- a set that somebody installed through the C ABI stays.

    THE RULE for callers: between the first setter call and the ``try`` whose handlers run both halves no statement can raise.
    So everything that can fail without the library -- the trajectory buffers, the outputs, the chain handle -- is made first,
    and ``install`` itself is called inside that ``try``."""

    def __init__(self, plan, bufs, gd):
        self.plan, self.bufs, self.gd = plan, bufs, gd
        self._enqueued = []          # (setter, clearing arguments) owed by clear_enqueued, in install order
        self._set = None             # the kind of the cloud / mesh set owed by clear_finished

    def _setter(self, lib, ctx, name, args, off):
        self._enqueued.append((name, off))
        _lib.check(getattr(lib, name)(ctx, *args), name)

    def install(self, lib, ctx, dev):
        p = self.plan
        uncond = (ptr(self.bufs.get("pos_uncond_traj")), ptr(self.bufs.get("v_uncond_traj")))
        if p.kind in _GUIDANCE:
            self._set = p.kind
            _install_guidance(lib, ctx, p.kind, p.payload, p.grad_step, self.gd)
        if p.first_step:
            self._setter(lib, ctx, "shapemol_set_option", (b"first_step", int(p.first_step)), (b"first_step", 0))
        if p.kind == "cfg" and p.cfg_groups is not None:        # (the rows stay in device memory for the chain in flight)
            off, stren, boxes = p.cfg_groups
            self._setter(lib, ctx, "shapemol_set_cfg_groups", (len(stren), ptr(off), ptr(stren), _lib.CFG_THRESHOLDS[p.threshold_type],
                                                               p.cfg_p, ptr(boxes), *uncond), (0, None, None, 0, 0.0, None, None, None))
        elif p.kind == "cfg":
            self._setter(lib, ctx, "shapemol_set_cfg", (float(p.guide_stren), _lib.CFG_THRESHOLDS[p.threshold_type], p.cfg_p,
                                                        ptr(p.cfg_box), *uncond), (0.0, 0, 0.0, None, None, None))
        if p.kind == "field":
            self._setter(lib, ctx, "shapemol_set_field_guidance", (p.field_dec._context(dev), p.grad_lr, int(p.grad_step)), (None, 0.0, 0))

    def clear_enqueued(self, lib, ctx):
        while self._enqueued:
            name, off = self._enqueued.pop(0)
            getattr(lib, name)(ctx, *off)

    def clear_finished(self, lib, ctx, dev):
        if self._set:
            kind, self._set = self._set, None
            torch.cuda.synchronize(dev)
            _clear_guidance(lib, ctx, kind)
