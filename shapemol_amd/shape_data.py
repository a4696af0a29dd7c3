"""Batches for the shape auto-encoder, built on the device from molecule meshes.

``ShapeData`` / ``collate_fn`` take the place of the reference's (datasets/shape_data.py:106-187, ``shape_type == 'point_cloud'``)
and ``get_pointAE_shape_emb`` of the reference's (utils/shape.py:240-284), starting from meshes.  The reference samples the
surface cloud with pytorch3d, tests ``3 * num_samples`` random points with ``trimesh.contains`` and measures them with an sklearn
KD-tree, per mesh on the host; here a batch of meshes goes through four kernels (csrc/sm_shape_data.h).  Containment is this
package's ray parity (the rule of mesh guidance), not trimesh's, and meshes are not checked for closedness, as the reference
does not check them either.  Limits: ``point_cloud_samples <= 2048``, int32 face indices.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._native import LOSS_TYPES, DeviceContexts, get, hip_device, host, ptr, stream_ptr

MAX_CLOUD = 2048       # kSdataMaxCloud (csrc/sm_shape_data.h)


def _pack_meshes(meshes):
    """[(verts (V,3), faces (F,3)), ...] -> host CSR arrays (vert_off, verts float64, face_off, faces int32)."""
    if len(meshes) == 0:
        raise ValueError("shape data: no mesh given")
    verts, faces, vo, fo = [], [], [0], [0]
    for b, m in enumerate(meshes):
        if not isinstance(m, (tuple, list)) or len(m) != 2:
            m = (m.vertices, m.faces)          # a trimesh-like object
        v = host(m[0], np.float64).reshape(-1, 3)
        f = host(m[1], None).reshape(-1, 3)
        if f.dtype != np.int32:
            f = f.astype(np.int64)
            if f.size and (f.min() < -2 ** 31 or f.max() >= 2 ** 31):
                raise ValueError(f"shape data: shape {b}: a face index does not fit int32")
            f = f.astype(np.int32)
        verts.append(v)
        faces.append(f)
        vo.append(vo[-1] + len(v))
        fo.append(fo[-1] + len(f))
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs), dtype=dt) if sum(len(x) for x in xs) else np.zeros((1, 3), dt)  # noqa: E731
    return np.asarray(vo, np.int64), cat(verts, np.float64), np.asarray(fo, np.int64), cat(faces, np.int32)


def _check(packed, n_cloud, n_samples, loss_code):
    """The library's argument checks (host only): ValueError with its message."""
    vo, v, fo, f = packed
    lib = _lib.load()
    if lib.shapemol_sdata_check(len(vo) - 1, ptr(vo), ptr(v), ptr(fo), ptr(f), int(n_cloud), int(n_samples), loss_code):
        raise ValueError(lib.shapemol_last_error().decode())


_contexts = DeviceContexts("shapemol_sdata_create", "shapemol_sdata_destroy")


def _chunk_seed(seed, chunk):
    """A seed of its own for every build of one call (splitmix64 of the pair), so that calls with neighbouring seeds share no stream."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (chunk + 1)) & (2 ** 64 - 1)
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
    return z ^ (z >> 31)


def _device(device):
    return hip_device(device, "shape data is built on a HIP device")


def _draws(t, shape, device, name):
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.array(t, dtype=np.float64))       # (a copy: the caller's array may be read-only)
    t = torch.as_tensor(t).to(device=device, dtype=torch.float64).contiguous()
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
    return t


def build_batch(meshes, n_cloud, n_samples, loss_type="signed_distance", *, device, seed=None, cloud_draws=None, query_draws=None,
                debug=False):
    """The kernels' call: dict of device tensors ``cloud (B,P,3)``, ``centres (B,3)``, ``bounds (B,3,2)`` and, with
    ``n_samples > 0``, ``points (B,T,3)``, ``values (B,T)`` and the host array ``counts (B,2)`` of (inside, outside) candidates;
    ``debug`` adds ``face_idx (B,P)``, ``flags (B,3T)``, ``sel (B,T)`` (int32).  ``n_samples == 0``: no query points."""
    if loss_type not in LOSS_TYPES:
        raise ValueError(f"loss_type must be 'signed_distance' or 'occupancy', got {loss_type!r}")
    packed = _pack_meshes(meshes)
    n_cloud, n_samples = int(n_cloud), int(n_samples)
    _check(packed, n_cloud, n_samples, LOSS_TYPES[loss_type])
    device = _device(device)
    B, P, T = len(meshes), n_cloud, n_samples
    cloud_draws = _draws(cloud_draws, (B, P, 3), device, "cloud_draws")
    query_draws = _draws(query_draws, (B, 3 * T, 3), device, "query_draws") if T else None
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    f32 = dict(dtype=torch.float32, device=device)
    i32 = dict(dtype=torch.int32, device=device)
    out = dict(cloud=torch.empty((B, P, 3), **f32), centres=torch.empty((B, 3), **f32), bounds=torch.empty((B, 3, 2), **f32))
    counts = np.zeros((B, 2), np.int32)
    if T:
        out.update(points=torch.zeros((B, T, 3), **f32), values=torch.zeros((B, T), **f32))
    if debug:
        out["face_idx"] = torch.empty((B, P), **i32)
        if T:
            out.update(flags=torch.empty((B, 3 * T), **i32), sel=torch.full((B, T), -1, **i32))
    vo, v, fo, f = packed
    lib, ctx = _lib.load(), _contexts.of(device)
    with torch.cuda.device(device):
        rc = lib.shapemol_sdata_build(
            ctx, B, ptr(vo), ptr(v), ptr(fo), ptr(f), P, T, LOSS_TYPES[loss_type], ptr(cloud_draws), ptr(query_draws),
            C.c_uint64(int(seed) & (2 ** 64 - 1)), ptr(out["cloud"]), ptr(out.get("points")), ptr(out.get("values")), ptr(out["centres"]),
            ptr(out["bounds"]), ptr(counts) if T else None, ptr(out.get("face_idx")), ptr(out.get("flags")), ptr(out.get("sel")),
            stream_ptr(device))
    if T:
        out["counts"] = counts
    if rc == 2:
        err = ValueError(lib.shapemol_last_error().decode())
        err.counts = counts
        raise err
    _lib.check(rc, "shapemol_sdata_build")
    return out


class ShapeData:
    """``ShapeData(batch_data, config)`` of the reference for ``config.shape_type == 'point_cloud'``: ``batch_data`` is a list of
    dicts with ``'mesh': (verts, faces)`` (numpy arrays or tensors); ``config`` (attribute object or dict) has ``shape_type``,
    ``point_cloud_samples``, ``num_samples`` and ``loss_type``.  Attributes: ``point_cloud (B,P,3)``, ``points (B,T,3)``,
    ``values (B,T)`` -- float32 tensors on ``device``, centred on the cloud's mean --, ``mesh`` (the list as given) and the extras
    ``centres (B,3)``, ``bounds (B,3,2)`` (device) and ``counts (B,2)`` (numpy: inside / outside candidates per shape).

    ``seed`` keys the device's Philox draws (``None``: one from torch's CPU generator); ``cloud_draws (B,P,3)`` /
    ``query_draws (B,3T,3)`` feed the uniforms instead (float64).  A shape whose candidates hold too few outside points to fill
    ``num_samples`` rows raises ValueError naming it (the reference's ``torch.stack`` fails there)."""

    def __init__(self, batch_data, config, *, device, seed=None, cloud_draws=None, query_draws=None):
        shape_type = get(config, "shape_type")
        if shape_type == "voxel":
            raise NotImplementedError("ShapeData: shape_type 'voxel' has no device implementation; the shipped models use 'point_cloud'")
        if shape_type != "point_cloud":
            raise ValueError(f"ShapeData: unknown shape_type {shape_type!r}")
        n_samples = int(get(config, "num_samples"))
        if n_samples < 2:
            raise ValueError(f"ShapeData: num_samples must be >= 2, got {n_samples}")
        meshes = [d["mesh"] for d in batch_data]
        out = build_batch(meshes, get(config, "point_cloud_samples"), n_samples, get(config, "loss_type"), device=device, seed=seed,
                          cloud_draws=cloud_draws, query_draws=query_draws)
        self._store = {"points": out["points"], "values": out["values"], "point_cloud": out["cloud"], "mesh": meshes,
                       "centres": out["centres"], "bounds": out["bounds"], "counts": out["counts"]}

    def to(self, device):
        device = torch.device(device)
        for k, v in self._store.items():
            if isinstance(v, torch.Tensor) and v.device != device:
                self._store[k] = v.to(device)
        return self

    def __getattr__(self, key):
        if key == "_store":
            raise AttributeError(key)
        try:
            return self._store[key]
        except KeyError:
            raise AttributeError(key) from None

    def __getstate__(self):
        return self.__dict__

    def __setstate__(self, mapping):
        for key, value in mapping.items():
            self.__dict__[key] = value


def collate_fn(batch_data, config, **kw):
    """``DataLoader(collate_fn=partial(collate_fn, config=config.data, device=...))``."""
    return ShapeData(batch_data, config, **kw)


def get_pointAE_shape_emb(meshes, model, point_cloud_samples, *, batch_size=32, seed=None, cloud_draws=None, device=None):
    """The reference's function from meshes on (``get_mesh`` needs oddt and stays with the caller): ``(zs, batch_bounds,
    batch_point_clouds, batch_point_cloud_centers)`` with ``zs = model.encoder(clouds)`` (``model``: this package's
    ``PointCloud_AE``, or a ``VN_DGCNN_Encoder``), clouds ``(B,1,P,3)`` centred, bounds ``(B,3,2)`` centred, centres ``(B,3)``;
    all device tensors.  ``batch_size`` meshes per build; ``cloud_draws (B,P,3)`` feeds the uniforms.  No query points are built."""
    encoder = getattr(model, "encoder", model)
    if device is None:
        device = next(encoder.parameters()).device
    device = _device(device)
    if seed is None and cloud_draws is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    clouds, centres, bounds = [], [], []
    for i in range(0, len(meshes), batch_size):
        part = meshes[i:i + batch_size]
        draws = None if cloud_draws is None else cloud_draws[i:i + batch_size]
        # (the Philox key holds the shape's index in ITS build: every build gets a seed of its own)
        out = build_batch(part, point_cloud_samples, 0, device=device, seed=_chunk_seed(seed or 0, i // batch_size), cloud_draws=draws)
        clouds.append(out["cloud"][:, None])
        centres.append(out["centres"])
        bounds.append(out["bounds"])
    if not clouds:
        raise ValueError("get_pointAE_shape_emb: no mesh given")
    batch_point_clouds = torch.cat(clouds, 0)
    with torch.no_grad():
        zs = encoder(batch_point_clouds)
    return zs, torch.cat(bounds, 0), batch_point_clouds, torch.cat(centres, 0)
