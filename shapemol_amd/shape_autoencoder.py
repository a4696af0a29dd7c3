"""Drop-in for the reference's shape auto-encoder ``PointCloud_AE`` and its decoder ``DecoderInner``
(``models/shape_pointcloud_modelAE.py:21-150``): the implicit field -- signed distance or occupancy -- that a shape latent
``z (Z, 3)`` encodes, evaluated at query points.  ``utils/shape.py:226-238`` builds the auto-encoder and the sampling script
passes it on as ``shape_AE``.

``DecoderInner`` has the reference's constructor arguments and forward contract (``p (B, T, 3), z (B, Z, 3) -> (B, T)``; ReLU
activations: ``PointCloud_AE`` never sets ``leaky``).  State-dict keys follow the reference for ``z_in``, ``fc_in`` and
``fc_out``; the residual blocks are registered here as ``blocks.{i}.fc_0.*`` / ``fc_1.*`` -- in the reference they live in a
plain Python list, so they are neither saved in ``se_model.pt`` nor moved by ``.to()``: loading that checkpoint
with ``strict=False`` leaves them at their initial values, exactly as the reference leaves them at random initial values.
All arithmetic runs in libshapemol_hip.so (``shapemol_sd_*`` / ``shapemol_field_*``, hand-written HIP); there is no CPU path.
Inference has one derivative, the field's gradient with respect to the query points (``decode_grad``, ``decode_atoms_grad``, the
autograd function ``field`` and the guidance pass ``guide_atoms`` built on it).  Training goes through ``DecoderInner.train_field``
(dense form only): the field as an autograd function differentiable in ``p``, ``z`` and every decoder parameter, whose backward is
one deterministic library call (``shapemol_field_train``); ``PointCloud_AE.get_generator_train_loss`` is the reference's training
loss on it, with the latent a constant when it comes from the encoder; ``PointCloud_AE.get_autoencoder_train_loss`` is the same
loss through ``VN_DGCNN_Encoder.encode_train``, differentiable in every encoder and generator parameter.
Once a module has a context, changed parameters that live on the context's device are repacked there by a kernel
(``shapemol_field_load_weights``) -- an optimiser step costs no host packing and no new context.
A module owns one library context whose per-shape workspace every call rewrites: calls of one module on different streams must
be ordered by the caller (events or a synchronise); the first call with more shapes than any before it synchronises the device.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._native import LOSS_TYPES, get, hip_device, ptr, stream_ptr
from .shape_encoder import VN_DGCNN_Encoder

__all__ = ["DecoderInner", "PointCloud_AE"]


class _VNLinear(nn.Module):
    """Parameter container with the reference's names (models/shape_vn_layers.py:VNLinear)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.map_to_feat = nn.Linear(cin, cout, bias=False)


class _ResnetBlockFC(nn.Module):
    """Parameter container of models/shape_vn_layers.py:210-252 with size_in == size_out (no shortcut); fc_1.weight starts at
    zero, as there."""

    def __init__(self, size):
        super().__init__()
        self.fc_0 = nn.Linear(size, size)
        self.fc_1 = nn.Linear(size, size)
        nn.init.zeros_(self.fc_1.weight)


class DecoderInner(nn.Module):
    def __init__(self, dim=3, z_dim=128, hidden_size=128, layer_num=4, loss_type="occupancy"):
        super().__init__()
        if dim != 3:
            raise ValueError("DecoderInner: dim must be 3")
        self.z_dim, self.hidden_size, self.layer_num, self.loss_type = z_dim, hidden_size, layer_num, loss_type
        self.z_in = _VNLinear(z_dim, z_dim)
        self.fc_in = nn.Linear(2 * z_dim + 1, hidden_size)
        self.blocks = nn.ModuleList([_ResnetBlockFC(hidden_size) for _ in range(layer_num)])
        self.fc_out = nn.Linear(hidden_size, 1)
        self._ctx, self._key = None, None

    def _params(self):
        """The parameters in the library's weight order."""
        parts = [self.z_in.map_to_feat.weight, self.fc_in.weight, self.fc_in.bias]
        for b in self.blocks:
            parts += [b.fc_0.weight, b.fc_0.bias, b.fc_1.weight, b.fc_1.bias]
        return parts + [self.fc_out.weight, self.fc_out.bias]

    def _pack(self):
        """The host's flat float32 vector of ``_params()``."""
        return np.concatenate([p.detach().cpu().numpy().astype(np.float32).reshape(-1) for p in self._params()])

    @staticmethod
    def _flat(params):
        """One flat float32 vector of ``params`` on their device (what ``_load_weights`` takes)."""
        return torch.cat([p.detach().to(torch.float32).reshape(-1) for p in params])

    def _load_weights(self, ctx, flat, device):
        """Repack the context's weights from one flat float32 device vector in ``_pack`` order (a kernel on the current stream)."""
        with torch.cuda.device(device):
            rc = _lib.load().shapemol_field_load_weights(ctx, ptr(flat), flat.numel(), stream_ptr(device))
        _lib.check(rc, "shapemol_field_load_weights")

    def _context(self, device):
        device = hip_device(device)      # ('cuda' and 'cuda:<current>' are one context)
        key = (str(device), self.loss_type) + tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._ctx is not None and key == self._key:
            return self._ctx
        if self._ctx is not None and key[:2] == self._key[:2] and all(p.device == device for p in self.parameters()):
            # the same context, new values (an optimiser step, load_state_dict): repacked on the device
            self._load_weights(self._ctx, self._flat(self._params()), device)
            self._key = key
            return self._ctx
        lib = _lib.load()
        self._release()
        w = self._pack()
        ctx = C.c_void_p()
        # (as in the reference, every loss_type but 'occupancy' is a signed distance: no sigmoid)
        _lib.check(lib.shapemol_sd_create(self.hidden_size, self.z_dim, self.layer_num, LOSS_TYPES.get(self.loss_type, 0), ptr(w), w.size,
                                          device.index, C.byref(ctx)), "shapemol_sd_create")
        self._ctx, self._key = ctx, key
        return ctx

    def _release(self):
        if getattr(self, "_ctx", None) is not None:
            _lib.load().shapemol_sd_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def tile(self, device):
        """Points a workgroup of the decode kernel takes per iteration (shapemol_sd_tile)."""
        with torch.cuda.device(device):
            return int(_lib.load().shapemol_sd_tile(self._context(device)))

    # ---- diagnostics (tests/test_gpu_shape_decoder.py) ----
    _DEBUG = {"z_inv": 0, "G": 1, "c": 2}

    def debug_read(self, device, name, n_shapes):
        """The per-shape prologue of the last decode on `device` as a numpy array (shapemol_sd_debug_read): z_inv (B, Z),
        G (B, H, 3), c (B, H) of fc_in(feature) = w_0 |p|^2 + G p + c."""
        shape = {"z_inv": (n_shapes, self.z_dim), "G": (n_shapes, self.hidden_size, 3), "c": (n_shapes, self.hidden_size)}[name]
        a = np.empty(shape, np.float32)
        _lib.check(_lib.load().shapemol_sd_debug_read(self._context(device), self._DEBUG[name], ptr(a), a.nbytes),
                   "shapemol_sd_debug_read")
        return a

    def grad_tile(self, device):
        """Points a workgroup of the value-and-gradient kernel takes per iteration (shapemol_field_grad_tile)."""
        with torch.cuda.device(device):
            return int(_lib.load().shapemol_field_grad_tile(self._context(device)))

    def _launch(self, p, shape_of, per_shape, z, with_grad):
        """shapemol_sd_decode, or with ``with_grad`` shapemol_field_decode_grad, on the current stream -> (out, grad or None)."""
        dev = p.device
        n, b = p.shape[0], z.shape[0]
        out = torch.empty((n,), dtype=torch.float32, device=dev)
        grad = torch.empty((n, 3), dtype=torch.float32, device=dev) if with_grad else None
        name = "shapemol_field_decode_grad" if with_grad else "shapemol_sd_decode"
        with torch.cuda.device(dev):
            args = [self._context(dev), ptr(p), ptr(shape_of), n, per_shape, ptr(z), b, ptr(out)] + ([ptr(grad)] if with_grad else [])
            rc = getattr(_lib.load(), name)(*args, stream_ptr(dev))
        _lib.check(rc, name)
        return out, grad

    def _decode_grad(self, p, shape_of, per_shape, z):
        return self._launch(p, shape_of, per_shape, z, True)

    def _decode(self, p, shape_of, per_shape, z):
        return self._launch(p, shape_of, per_shape, z, False)[0]

    def _latent(self, z, dev):
        if not isinstance(z, torch.Tensor) or not z.is_cuda:
            raise RuntimeError("z must be a tensor on a HIP device (shapemol_amd has no CPU path)")
        if z.device != dev:
            raise RuntimeError(f"z is on {z.device}, the points are on {dev}")
        z = z.reshape(z.shape[0], -1, 3).to(torch.float32).contiguous()
        if z.shape[1] != self.z_dim:
            raise ValueError(f"z has {z.shape[1]} latent vectors per shape, the decoder was built for z_dim = {self.z_dim}")
        return z

    def _dense(self, p, z):
        """Checked arguments of the dense forms: (x (B T, 3) float32 contiguous, z (B, Z, 3), B, T)."""
        if not isinstance(p, torch.Tensor) or not p.is_cuda:
            raise RuntimeError("p must be a tensor on a HIP device (shapemol_amd has no CPU path)")
        if p.dim() != 3 or p.shape[2] != 3:
            raise ValueError(f"p must be (B, T, 3), got {tuple(p.shape)}")
        z = self._latent(z, p.device)
        if z.shape[0] != p.shape[0]:
            raise ValueError(f"p has {p.shape[0]} shapes, z has {z.shape[0]}")
        b, t = p.shape[0], p.shape[1]
        return p.detach().to(torch.float32).contiguous().view(b * t, 3), z, b, t

    def _atoms(self, pos, batch, z):
        """Checked arguments of the per-atom forms: (pos (N, 3) float32 contiguous, batch (N,) integer, z (B, Z, 3))."""
        if not isinstance(pos, torch.Tensor) or not pos.is_cuda or not isinstance(batch, torch.Tensor) or not batch.is_cuda:
            raise RuntimeError("pos and batch must be tensors on a HIP device (shapemol_amd has no CPU path)")
        if pos.dim() != 2 or pos.shape[1] != 3 or batch.dim() != 1 or batch.shape[0] != pos.shape[0]:
            raise ValueError(f"pos must be (N, 3) and batch (N,), got {tuple(pos.shape)} and {tuple(batch.shape)}")
        if batch.dtype.is_floating_point or batch.dtype == torch.bool:
            raise ValueError("batch must be an integer tensor")
        z = self._latent(z, pos.device)
        n, b = pos.shape[0], z.shape[0]
        if n and bool(((batch < 0) | (batch >= b)).any()):
            raise ValueError(f"batch must lie in [0, {b}) (the number of shapes in z); got values from {int(batch.min())} to {int(batch.max())}")
        return pos.detach().to(torch.float32).contiguous(), batch, z

    @torch.no_grad()
    def forward(self, p, z, c=None, **kwargs):
        """p (B, T, 3), z (B, Z, 3) (or (B, 3 Z)) float32 device tensors -> (B, T): the field of shape b at its T points.
        1 <= B <= 65535 and B * T < 2^31, else ShapeMolLibraryError before any launch; T == 0 gives an empty tensor."""
        x, z, b, t = self._dense(p, z)
        return self._decode(x, None, t, z).view(b, t)

    @torch.no_grad()
    def decode_atoms(self, pos, batch, z):
        """The field of shape batch[i] at pos[i]: pos (N, 3) float32, batch (N,) integer in [0, B) in any order, z (B, Z, 3)
        -> (N,).  The natural use: the signed distance or occupancy of every generated atom under its molecule's shape
        condition.  An entry of batch outside [0, B) raises ValueError (checked with device ops before the call)."""
        pos, batch, z = self._atoms(pos, batch, z)
        return self._decode(pos, batch.to(torch.int32).contiguous(), 0, z)

    @torch.no_grad()
    def decode_grad(self, p, z):
        """``forward`` and its gradient with respect to the points in one kernel: -> (out (B, T), grad (B, T, 3) = d out / d p).
        ``out`` equals ``forward(p, z)`` bit for bit.  The gradient of a ReLU network is piecewise constant: it is the one of
        the linear piece the float32 evaluation lands in (mask = input > 0)."""
        x, z, b, t = self._dense(p, z)
        out, grad = self._decode_grad(x, None, t, z)
        return out.view(b, t), grad.view(b, t, 3)

    @torch.no_grad()
    def decode_atoms_grad(self, pos, batch, z):
        """``decode_atoms`` and its gradient: -> (out (N,), grad (N, 3)): per atom the signed distance (or occupancy) under its
        molecule's shape condition and the direction in which it grows."""
        pos, batch, z = self._atoms(pos, batch, z)
        return self._decode_grad(pos, batch.to(torch.int32).contiguous(), 0, z)

    @torch.no_grad()
    def guide_atoms(self, pos, batch, z, grad_lr):
        """One pass of the reference's gradient shape guidance (``models/molopt_score_model.py:592-615``) as one kernel: with
        ``d`` the field of shape ``batch[i]`` at atom i and ``T`` the atom count of its molecule,
        ``p' = p - grad_lr * (min(d, 0.5) - 0.5) * (1[d < 0.5] / T) * grad_p d``; atoms with ``d >= 0.5`` stay.  ``batch`` must be
        sorted (``ValueError`` otherwise).  Returns a new tensor; ``pos`` is left untouched."""
        pos, batch, z = self._atoms(pos, batch, z)
        grad_lr = float(grad_lr)
        if not np.isfinite(grad_lr):
            raise ValueError(f"grad_lr must be finite, got {grad_lr}")
        n = pos.shape[0]
        if n > 1 and bool((batch[1:] < batch[:-1]).any()):
            raise ValueError("batch must be sorted (atoms of a molecule are contiguous)")
        out = pos.clone()
        batch = batch.to(torch.int64).contiguous()
        dev = pos.device
        with torch.cuda.device(dev):
            rc = _lib.load().shapemol_field_guide(self._context(dev), ptr(out), ptr(batch), n, ptr(z), z.shape[0], grad_lr,
                                               stream_ptr(dev))
        _lib.check(rc, "shapemol_field_guide")
        return out

    def field(self, p, z):
        """``forward`` as a ``torch.autograd.Function`` differentiable in ``p`` only: p (B, T, 3) -> (B, T), whose backward is
        ``grad_out[..., None] * grad`` with the gradient the forward kernel saved.  For guidance rules written in torch.  A ``z``
        that requires grad, or a second derivative, raises ``RuntimeError``."""
        if isinstance(z, torch.Tensor) and z.requires_grad:
            raise RuntimeError("DecoderInner.field is differentiable in p only: z must not require grad")
        return _Field.apply(p, z, self)

    def train_tile(self, device):
        """Points a workgroup of the training kernel takes per iteration (shapemol_field_train_tile); a chunk is a multiple."""
        with torch.cuda.device(device):
            return int(_lib.load().shapemol_field_train_tile(self._context(device)))

    def train_field(self, p, z, chunk_points=0):
        """``forward`` as a ``torch.autograd.Function`` differentiable in ``p``, ``z`` and every decoder parameter (``z_in``,
        ``fc_in``, every block, ``fc_out``): p (B, T, 3), z (B, Z, 3) -> (B, T), equal to ``forward(p, z)`` bit for bit.  The
        forward loads the parameters' current device values into the context and evaluates the field; the backward runs the
        forward again inside the training call (the operands a weight gradient needs live in a workspace bounded by
        ``chunk_points``, 0 = the library's default, so they cannot be kept from one call to the next) and returns every
        gradient from that one call, deterministically.  Once differentiable.  The parameters must live on p's device."""
        x, zz, b, t = self._dense(p, z)
        dev = p.device
        params = self._params()
        if any(q.device != dev for q in params):
            raise RuntimeError(f"the decoder's parameters must be on {dev}, where the points are (shapemol_amd has no CPU path)")
        if not isinstance(z, torch.Tensor) or z.dtype != torch.float32 or p.dtype != torch.float32:
            raise ValueError("train_field takes float32 p and z")
        return _TrainField.apply(p, z, self, int(chunk_points), *params)


class _Field(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, z, dec):
        out, grad = dec.decode_grad(p, z)
        ctx.save_for_backward(grad)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable      # (a second derivative raises: the gradient is piecewise constant)
    def backward(ctx, grad_out):
        grad, = ctx.saved_tensors
        return grad_out.unsqueeze(-1) * grad, None, None


class _TrainField(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, z, dec, chunk_points, *params):
        x, zz, b, t = dec._dense(p, z)
        flat = dec._flat(params)
        dec._context(p.device)                             # (repacks by itself when a parameter changed)
        ctx.dec, ctx.dims, ctx.chunk = dec, (b, t), chunk_points
        ctx.shapes = [q.shape for q in params]
        ctx.z_shape = z.shape
        ctx.save_for_backward(x, zz, flat)
        ctx.weights_key = dec._key
        return dec._decode(x, None, t, zz).view(b, t)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, zz, flat = ctx.saved_tensors
        dec, (b, t) = ctx.dec, ctx.dims
        dev = x.device
        handle = dec._context(dev)
        if dec._key != ctx.weights_key:                    # the module's parameters moved on since the forward: this graph's values
            dec._load_weights(handle, flat, dev)
            dec._key = dec._key[:2] + (None,)              # (and the next call repacks the current ones)
        up = grad_out.detach().to(torch.float32).contiguous()
        gp = torch.empty((b * t, 3), dtype=torch.float32, device=dev)
        gz = torch.empty_like(zz)
        gw = torch.empty_like(flat)
        with torch.cuda.device(dev):
            rc = _lib.load().shapemol_field_train(handle, ptr(x), b, t, ptr(zz), ptr(up), None, ptr(gp), ptr(gz), ptr(gw), ctx.chunk,
                                                  stream_ptr(dev))
        _lib.check(rc, "shapemol_field_train")
        grads, o = [], 0
        for shp in ctx.shapes:
            n = int(np.prod(shp))
            grads.append(gw[o:o + n].view(shp))
            o += n
        return (gp.view(b, t, 3), gz.view(ctx.z_shape), None, None, *grads)


class PointCloud_AE(nn.Module):
    """``PointCloud_AE(config)`` of the reference: ``.encoder`` (the device ``VN_DGCNN_Encoder``) and ``.generator`` (the device
    ``DecoderInner``), built from ``config.{encoder, hidden_dim, latent_dim, layer_num, num_k, point_dim, loss_type}``
    (``ckpt['config'].model`` of ``se_model.pt``; an attribute object or a dict)."""

    def __init__(self, config):
        super().__init__()
        enc = get(config, "encoder")
        if enc == "VN_Resnet":
            raise NotImplementedError("PointCloud_AE: the VN_Resnet encoder has no device implementation; the shipped model uses VN_DGCNN")
        if enc != "VN_DGCNN":
            raise ValueError(f"PointCloud_AE: unknown encoder {enc!r}")
        hidden, latent, layers = get(config, "hidden_dim"), get(config, "latent_dim"), get(config, "layer_num")
        self.encoder = VN_DGCNN_Encoder(hidden, latent, layers, get(config, "num_k"))
        self.generator = DecoderInner(get(config, "point_dim"), latent, hidden, layers, get(config, "loss_type"))
        self.loss_type = get(config, "loss_type")

    @torch.no_grad()
    def forward(self, inputs, z_vector, point_coord, is_training=False):
        """(latent, field) with the reference's call contract: a given cloud batch ``inputs (B, 1, N, 3)`` is encoded and takes the
        place of ``z_vector``; the field is evaluated where both a latent and ``point_coord (B, T, 3)`` exist and is ``None``
        otherwise.  ``is_training`` always encodes and always decodes (there is no backward through ``z`` or the weights)."""
        if is_training or inputs is not None:
            latent = self.encoder(inputs)
        else:
            latent = z_vector
        if is_training or (latent is not None and point_coord is not None):
            return latent, self.generator(point_coord, latent)
        return latent, None

    @torch.no_grad()
    def get_val_loss(self, point_clouds, sample_points, sample_values):
        """Validation triple of clouds ``(B, N, 3)`` against ``sample_values (B, T)`` at ``sample_points (B, T, 3)``: the mean
        squared error of the field, the fraction of points whose thresholded field (> 0.5) equals the sample value, and that
        fraction among the occupied samples (value 1) alone; three 0-d device tensors."""
        field = self.forward(point_clouds[:, None], None, sample_points)[1]
        mse = (field - sample_values).square().mean()
        hit = (field > 0.5).to(sample_values.dtype) == sample_values
        occupied = sample_values == 1
        n_occupied = int(occupied.sum())                     # a host count, as the reference divides by one (same rounding)
        return mse, hit.sum() / hit.numel(), (hit & occupied).sum() / n_occupied

    def get_train_loss(self, point_clouds, sample_points, sample_values):
        raise NotImplementedError("PointCloud_AE.get_train_loss keeps refusing (the name stays bound to the frozen encoder): "
                                  "get_autoencoder_train_loss is the same loss with gradients for the encoder and the generator; "
                                  "get_generator_train_loss trains the generator (and a given latent) on the same loss")

    def get_autoencoder_train_loss(self, point_clouds, sample_points, sample_values):
        """The reference's ``get_train_loss`` (``models/shape_pointcloud_modelAE.py:146-150``): ``encode_train`` of ``point_clouds (B, N, 3)``,
        ``generator.train_field`` at ``sample_points (B, T, 3)``, ``mean((net_out - sample_values) ** 2)``.  Differentiable in every
        parameter of the encoder and of the generator; the clouds and the sample points are data."""
        latent = self.encoder.encode_train(point_clouds[:, None])
        net_out = self.generator.train_field(sample_points, latent)
        return torch.mean((net_out - sample_values) ** 2)

    def get_generator_train_loss(self, point_clouds, sample_points, sample_values, z_vector=None):
        """The reference's ``get_train_loss`` formula, ``mean((net_out - sample_values) ** 2)``, differentiable in the generator's
        parameters and in a given ``z_vector`` (B, Z, 3).  Without ``z_vector`` the latent is the device encoder's of
        ``point_clouds (B, N, 3)``, under ``no_grad``: the encoder receives no gradient.  For the generator's parameters the
        gradient is the one the reference's ``loss.backward()`` gives."""
        if z_vector is None:
            with torch.no_grad():
                z_vector = self.encoder(point_clouds[:, None])
        net_out = self.generator.train_field(sample_points, z_vector)
        return torch.mean((net_out - sample_values) ** 2)
