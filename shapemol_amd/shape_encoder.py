"""Drop-in for the encoder half of the reference's shape auto-encoder: ``VN_DGCNN_Encoder``
(``models/shape_pointcloud_modelAE.py:207-255``), the module that turns a molecule's surface point cloud into the
``shape_emb`` (32, 3) the diffusion model is conditioned on (``utils/shape.py:240-283``).

Same constructor arguments and forward contract (``input (B, 1, N, 3) -> (B, latent_dim, 3)``).  State-dict keys follow
the reference for ``conv_pos`` and ``conv_c``; the DGCNN blocks are registered here as ``blocks.{i}.*`` -- in the
reference they live in a plain Python list, so they are neither saved in ``se_model.pt`` nor moved by ``.to()``
(SURVEY.md F5): loading that checkpoint with ``strict=False`` leaves them at their initial values, exactly as the
reference leaves them at random initial values.  Batch-norm uses batch statistics, as the reference's auto-encoder does
(it is never switched to eval mode, ``utils/shape.py:226-238``); ``forward`` carries the running statistics without updating them.
All arithmetic runs in libshapemol_hip.so (``shapemol_se_*``, hand-written HIP); there is no CPU path.
``forward`` is frozen (``no_grad``).  Training goes through ``encode_train``: the same latent as one autograd function whose
backward is one deterministic library call (``shapemol_se_train_backward``) that fills the gradient of every parameter; the points
receive none.  Once a module has a context, changed parameters that live on the context's device are repacked there by a kernel
(``shapemol_se_load_weights``) -- an optimiser step costs no host packing and no new context.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._native import hip_device, ptr, stream_ptr

__all__ = ["VN_DGCNN_Encoder"]


class _VNLinearLeakyReLU(nn.Module):
    """Parameter container with the reference's names (models/shape_vn_layers.py:95-124)."""

    def __init__(self, cin, cout, share_nonlinearity=False):
        super().__init__()
        self.map_to_feat = nn.Linear(cin, cout, bias=False)
        self.batchnorm = nn.Module()
        self.batchnorm.bn = nn.BatchNorm1d(cout)          # parameter / buffer names as BatchNorm1d / BatchNorm2d alike
        self.map_to_dir = nn.Linear(cin, 1 if share_nonlinearity else cout, bias=False)


class VN_DGCNN_Encoder(nn.Module):
    def __init__(self, hidden_dim, latent_dim, layer_num, num_k):
        super().__init__()
        self.hidden_dim, self.latent_dim, self.layer_num, self.num_k = hidden_dim, latent_dim, layer_num, num_k
        self.conv_pos = _VNLinearLeakyReLU(2, hidden_dim)
        self.blocks = nn.ModuleList([_VNLinearLeakyReLU(2 * hidden_dim, hidden_dim) for _ in range(layer_num)])
        self.conv_c = _VNLinearLeakyReLU(layer_num * hidden_dim, latent_dim, share_nonlinearity=True)
        self._ctx, self._key = None, None

    def _stages(self):
        return [self.conv_pos, *self.blocks, self.conv_c]

    def _params(self):
        """The parameters in the library's weight order."""
        parts = []
        for m in self._stages():
            parts += [m.map_to_feat.weight, m.batchnorm.bn.weight, m.batchnorm.bn.bias, m.map_to_dir.weight]
        return parts

    def _pack(self):
        return np.concatenate([p.detach().cpu().numpy().astype(np.float32).reshape(-1) for p in self._params()])

    @staticmethod
    def _flat(params):
        """One flat float32 vector of ``params`` on their device (what ``_load_weights`` takes)."""
        return torch.cat([p.detach().to(torch.float32).reshape(-1) for p in params])

    def _load_weights(self, ctx, flat, device):
        """Repack the context's weights from one flat float32 device vector in ``_pack`` order (a kernel on the current stream)."""
        with torch.cuda.device(device):
            rc = _lib.load().shapemol_se_load_weights(ctx, ptr(flat), flat.numel(), stream_ptr(device))
        _lib.check(rc, "shapemol_se_load_weights")

    def _context(self, device):
        device = hip_device(device)      # ('cuda' and 'cuda:<current>' are one context)
        key = (str(device),) + tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._ctx is not None and key == self._key:
            return self._ctx
        if self._ctx is not None and key[0] == self._key[0] and all(p.device == device for p in self.parameters()):
            # the same context, new values (an optimiser step, load_state_dict): repacked on the device
            self._load_weights(self._ctx, self._flat(self._params()), device)
            self._key = key
            return self._ctx
        lib = _lib.load()
        self._release()
        w = self._pack()
        ctx = C.c_void_p()
        _lib.check(lib.shapemol_se_create(self.hidden_dim, self.latent_dim, self.layer_num, self.num_k, ptr(w), w.size, device.index,
                                          C.byref(ctx)), "shapemol_se_create")
        self._ctx, self._key = ctx, key
        return ctx

    def _release(self):
        if getattr(self, "_ctx", None) is not None:
            _lib.load().shapemol_se_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def max_points(self, device):
        """Largest N the library accepts on `device` (shapemol_se_max_points)."""
        with torch.cuda.device(device):
            return int(_lib.load().shapemol_se_max_points(self._context(device)))

    # ---- diagnostics (tests/test_gpu_shape_encoder.py) ----
    _DEBUG = {"idx": (0, np.int32), "h0": (1, np.float32), "hcat": (2, np.float32), "y": (3, np.float32), "xx": (4, np.float32),
              "pd": (5, np.float32)}

    def debug_stop_after(self, device, n_blocks):
        """Following forwards return after block `n_blocks` (0: after conv_pos; -1: full encode again), leaving the output unset."""
        _lib.check(_lib.load().shapemol_se_debug_stop_after(self._context(device), n_blocks), "shapemol_se_debug_stop_after")

    def debug_read(self, device, name, n_total):
        """Workspace buffer `name` of the last forward on `device` (n_total = B * N points of it) as a numpy array
        (shapemol_se_debug_read): idx (P, k), h0 (P, C, 3), hcat (P, L, C, 3), y (P, 4C, 3), xx (P,), pd (P, latent + 1, 3)."""
        code, dt = self._DEBUG[name]
        C_, L, LAT = self.hidden_dim, self.layer_num, self.latent_dim
        shape = {"idx": (n_total, self.num_k), "h0": (n_total, C_, 3), "hcat": (n_total, L, C_, 3), "y": (n_total, 4 * C_, 3), "xx": (n_total,),
                 "pd": (n_total, LAT + 1, 3)}[name]
        a = np.empty(shape, dt)
        _lib.check(_lib.load().shapemol_se_debug_read(self._context(device), code, ptr(a), a.nbytes),
                   "shapemol_se_debug_read")
        return a

    @torch.no_grad()
    def forward(self, input):
        """input (B, 1, N, 3) (or (B, N, 3)) float32 device tensor -> latent (B, latent_dim, 3).

        1 <= B <= 65535, B * N <= 2^24, and N a multiple of 16 in [32, ``max_points(device)``]: the kNN needs N >= num_k = 20 and
        keeps the 16 x N distances of a row block in LDS, so the largest N is the device's dynamic LDS per workgroup / 64 bytes
        (2560 where a workgroup can have 160 KiB).  Anything else raises ShapeMolLibraryError before any launch."""
        if not isinstance(input, torch.Tensor) or not input.is_cuda:
            raise RuntimeError("input must be a tensor on a HIP device (shapemol_amd has no CPU path)")
        x = input.reshape(input.shape[0], -1, 3).to(torch.float32).contiguous()
        b, n = x.shape[0], x.shape[1]
        dev = x.device
        out = torch.empty((b, self.latent_dim, 3), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.load().shapemol_se_encode(self._context(dev), ptr(x), b, n, ptr(out), stream_ptr(dev))
        _lib.check(rc, "shapemol_se_encode")
        return out

    # ---- training ----
    def _workspace(self, handle, b, n, dev):
        size = int(_lib.load().shapemol_se_train_workspace(handle, b, n))
        return torch.empty((max(size, 1),), dtype=torch.uint8, device=dev)

    def _train_forward(self, x, workspace=None):
        """x (B, N, 3) float32 contiguous on the device -> (latent (B, latent_dim, 3), saved): ``shapemol_se_train_forward``.  ``saved``
        holds what the backward needs, in tensors of its own: idx (L + 1, P, 20) int32, h0 (P, C, 3), hcat (P, L, C, 3),
        stats (L + 2, 2, 256) float64 (batch mean and biased variance per stage and channel), pd (P, latent + 1, 3).  In training mode
        the running statistics of the L + 2 batch norms move as ``nn.BatchNorm`` moves them."""
        b, n = x.shape[0], x.shape[1]
        dev, P, C_, L, LAT = x.device, b * n, self.hidden_dim, self.layer_num, self.latent_dim
        handle = self._context(dev)
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)      # noqa: E731
        saved = dict(x=x, dims=(b, n), idx=new((L + 1, P, self.num_k), torch.int32), h0=new((P, C_, 3), torch.float32),
                     hcat=new((P, L, C_, 3), torch.float32), stats=new((L + 2, 2, 256), torch.float64), pd=new((P, LAT + 1, 3), torch.float32))
        out = new((b, LAT, 3), torch.float32)
        with torch.cuda.device(dev):
            ws = self._workspace(handle, b, n, dev) if workspace is None else workspace
            rc = _lib.load().shapemol_se_train_forward(handle, ptr(x), b, n, ptr(saved["idx"]), ptr(saved["h0"]), ptr(saved["hcat"]), ptr(saved["stats"]),
                                                       ptr(saved["pd"]), ptr(out), ptr(ws), ws.numel(), stream_ptr(dev))
        _lib.check(rc, "shapemol_se_train_forward")
        if self.training:
            self._update_running(saved["stats"], P)
        return out, saved

    @torch.no_grad()
    def _update_running(self, stats, n_points):
        """``nn.BatchNorm1d/2d`` in training mode: momentum 0.1, the unbiased batch variance; B N k samples per channel for the edge
        stages, B N for conv_c."""
        stages = self._stages()
        for i, m in enumerate(stages):
            bn = m.batchnorm.bn
            count = n_points * (self.num_k if i + 1 < len(stages) else 1)
            nch = bn.running_mean.numel()
            mean, var = stats[i, 0, :nch], stats[i, 1, :nch] * (count / max(count - 1, 1))
            bn.running_mean.mul_(1 - bn.momentum).add_(bn.momentum * mean.to(bn.running_mean))
            bn.running_var.mul_(1 - bn.momentum).add_(bn.momentum * var.to(bn.running_var))
            bn.num_batches_tracked += 1

    def _train_backward(self, saved, grad_out=None, grad_hcat=None, workspace=None, handle=None, masks=None):
        """The flat gradient vector (``_pack`` order) of ``shapemol_se_train_backward`` from ``saved`` and the latent's gradient
        ``grad_out`` (B, latent_dim, 3) -- or, with conv_c skipped, from ``grad_hcat`` (P, L, C, 3), the gradient at conv_c's input.
        ``handle``: the context to run on as it is (the autograd node passes one it has loaded with its graph's weights); without it
        the module's context with the current parameters.  ``masks``: an int32 tensor (L + 2, P, 256) that receives the leaky-ReLU
        branches taken (diagnostic, see the header)."""
        x, (b, n) = saved["x"], saved["dims"]
        dev = x.device
        if handle is None:
            handle = self._context(dev)
        up = None if grad_out is None else grad_out.detach().to(torch.float32).contiguous()
        uh = None if grad_hcat is None else grad_hcat.detach().to(torch.float32).contiguous()
        gw = torch.empty((sum(p.numel() for p in self._params()),), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ws = self._workspace(handle, b, n, dev) if workspace is None else workspace
            rc = _lib.load().shapemol_se_train_backward(handle, ptr(x), b, n, ptr(saved["idx"]), ptr(saved["h0"]), ptr(saved["hcat"]), ptr(saved["stats"]),
                                                        ptr(saved["pd"]), None if up is None else ptr(up), None if uh is None else ptr(uh), ptr(gw),
                                                        ptr(masks), ptr(ws), ws.numel(), stream_ptr(dev))
        _lib.check(rc, "shapemol_se_train_backward")
        return gw

    def encode_train(self, input):
        """``forward`` as a ``torch.autograd.Function`` differentiable in every parameter (``map_to_feat.weight``, ``batchnorm.bn.weight``,
        ``batchnorm.bn.bias`` and ``map_to_dir.weight`` of ``conv_pos``, every block and ``conv_c``): input (B, 1, N, 3) or (B, N, 3)
        with ``forward``'s limits -> latent (B, latent_dim, 3).  The clouds are data: no gradient flows to ``input`` (one that requires
        grad raises ``RuntimeError``), and none through the neighbour lists.  The batch statistics are summed in a fixed order, so the
        latent and every gradient are bit-identical from run to run; the latent equals ``forward``'s up to that summation order.  In
        training mode the running statistics are updated.  Once differentiable.  The parameters must live on the input's device."""
        if not isinstance(input, torch.Tensor) or not input.is_cuda:
            raise RuntimeError("input must be a tensor on a HIP device (shapemol_amd has no CPU path)")
        if input.requires_grad:
            raise RuntimeError("VN_DGCNN_Encoder.encode_train gives no gradient to the points: input must not require grad")
        params = self._params()
        if any(q.device != input.device for q in params):
            raise RuntimeError(f"the encoder's parameters must be on {input.device}, where the points are (shapemol_amd has no CPU path)")
        x = input.reshape(input.shape[0], -1, 3).to(torch.float32).contiguous()
        return _EncodeTrain.apply(x, self, *params)


class _EncodeTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, enc, *params):
        flat = enc._flat(params)
        out, saved = enc._train_forward(x)                 # (its _context repacks by itself when a parameter changed)
        ctx.enc, ctx.saved, ctx.flat, ctx.weights_key = enc, saved, flat, enc._key
        ctx.shapes = [q.shape for q in params]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        enc, dev = ctx.enc, ctx.saved["x"].device
        handle = enc._context(dev)
        if enc._key != ctx.weights_key:                    # the module's parameters moved on since the forward: this graph's values
            enc._load_weights(handle, ctx.flat, dev)
            enc._key = (enc._key[0], None)                 # (and the next call repacks the current ones)
        gw = enc._train_backward(ctx.saved, grad_out=grad_out, handle=handle)      # (on the handle as loaded: no second _context)
        grads, o = [], 0
        for shp in ctx.shapes:
            n = int(np.prod(shp))
            grads.append(gw[o:o + n].view(shp))
            o += n
        return (None, None, *grads)
