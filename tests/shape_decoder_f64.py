"""The shape decoder recomposed in torch on the CPU, in float64 and float32 (tests/test_shape_decoder_cpu.py,
tests/test_gpu_shape_decoder.py): the prologue (z_dir, z_inv), fc_in in the reference's concatenated form
[ |p|^2 , p.z_0 .. p.z_{Z-1} , z_inv ], the residual blocks x + fc_1(relu(fc_0(relu(x)))) and the head fc_out(relu(x)) with the
sigmoid of loss_type 'occupancy' (reference: models/shape_pointcloud_modelAE.py:69-103, models/shape_vn_layers.py:243-252).

Points are given ragged -- p (N, 3) with a shape index per point -- so that one function serves the dense (B, T, 3) form (index
= point // T) and decode_atoms.  The gate is precision.bound: eH <= 4 e32 + 16 * 2^-24 on max-normalised errors.

`fault` evaluates a deliberately wrong decoder (the negative controls of the CPU tests):
    other_shape   G and c (the latent) of the next shape            swap_fc    fc_0 and fc_1 of every block exchanged
    no_last_relu  fc_out(x) instead of fc_out(relu(x))              no_pp      the |p|^2 column dropped
    sigmoid       the sigmoid applied whatever the loss type         f16x2      both operands of every Linear rounded to two fp16 pieces
"""
import os

import numpy as np
import torch

from precision import U, bound, f16x2, rel_err          # the project's gate: eH <= 4 e32 + 16 u on max-normalised errors
from shapemol_amd import synth

F64, F32 = torch.float64, torch.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shape_decoder.npz")
FAULTS = ("other_shape", "swap_fc", "no_last_relu", "no_pp", "sigmoid", "f16x2")


def gate(res, r32, r64):
    """(eH, e32, passed) of a result against the float64 value, e32 from a float32 evaluation (the reference's own where a
    fixture holds one)."""
    eh, e32 = rel_err(res, r64), rel_err(r32, r64)
    return eh, e32, eh <= bound(e32)


def state_dict(layers=4, latent=32, hidden=128, seed=19, fc1_zero=False, small_fc0=False):
    """{key: float32 tensor} of synth.shape_decoder_state_dict.  fc1_zero: every fc_1.weight zero, the reference's
    initialisation (only the bias path of a block's second Linear is left).  small_fc0: fc_0 (weight and bias) of every block
    times 2^-6 and fc_1.weight times 2^6 -- ReLU is positively homogeneous, so the decoder is the same function and every
    float32 / float64 result the same to the bit, but fc_0's weights fall below 2^-9, where a two-piece fp16 operand is
    only within 2^-25 absolute."""
    sd = {k: torch.from_numpy(v) for k, v in synth.shape_decoder_state_dict(hidden, latent, layers, seed).items()}
    for i in range(layers):
        if fc1_zero:
            sd[f"blocks.{i}.fc_1.weight"] = torch.zeros_like(sd[f"blocks.{i}.fc_1.weight"])
        if small_fc0:
            sd[f"blocks.{i}.fc_0.weight"] = sd[f"blocks.{i}.fc_0.weight"] * 2.0 ** -6
            sd[f"blocks.{i}.fc_0.bias"] = sd[f"blocks.{i}.fc_0.bias"] * 2.0 ** -6
            sd[f"blocks.{i}.fc_1.weight"] = sd[f"blocks.{i}.fc_1.weight"] * 2.0 ** 6
    return sd


def inputs(B, counts, latent, seed, p_scale=1.0, z_scale=0.5):
    """(p (N, 3), shape_of (N,) int64, z (B, latent, 3)) float32: hash-normal points and latents; counts[b] points of shape b
    (an int: the same for every shape)."""
    counts = [counts] * B if isinstance(counts, int) else list(counts)
    n = int(sum(counts))
    p = torch.from_numpy((synth.hash_normal((n, 3), 611, seed) * np.float32(p_scale)).astype(np.float32))
    z = torch.from_numpy((synth.hash_normal((B, latent, 3), 612, seed) * np.float32(z_scale)).astype(np.float32))
    shape_of = torch.repeat_interleave(torch.arange(B), torch.tensor(counts))
    return p, shape_of, z


def decode(sd, p, shape_of, z, layers, loss_type, dtype=F64, form="concat", fault=None, taps=False):
    """dict(out (N,), z_inv (B, Z), G (B, H, 3), c (B, H)) in `dtype`; with taps also relu_in, the 2 layers + 1 inputs (N, H) of the ReLUs.
    form 'concat': fc_in on the concatenated feature, as the reference; 'factored': w_0 |p|^2 + G p + c, as the device."""
    assert fault is None or fault in FAULTS, fault
    op = f16x2 if fault == "f16x2" else (lambda t: t)
    W = {k: v.to(dtype) for k, v in sd.items()}
    p, z = p.to(dtype), z.to(dtype)
    Z = z.shape[1]

    def lin(x, w, b=None):
        y = op(x) @ op(w).T
        return y if b is None else y + b

    z_dir = torch.einsum("mk,bkx->bmx", op(W["z_in.map_to_feat.weight"]), op(z))
    z_inv = (z * z_dir).sum(-1)                                              # (B, Z)
    w_in, b_in = W["fc_in.weight"], W["fc_in.bias"]
    w0, wz, wi = w_in[:, 0], w_in[:, 1:1 + Z], w_in[:, 1 + Z:]
    G = torch.einsum("hm,bmx->bhx", op(wz), op(z))                            # (B, H, 3)
    c = lin(z_inv, wi, b_in)                                                 # (B, H)
    s = (shape_of + 1) % z.shape[0] if fault == "other_shape" else shape_of
    pp = (p * p).sum(-1, keepdim=True)
    if fault == "no_pp":
        pp = torch.zeros_like(pp)
    if form == "concat":
        feat = torch.cat([pp, torch.einsum("nx,nmx->nm", p, z[s]), z_inv[s]], dim=1)
        x = lin(feat, w_in, b_in)
    else:
        x = pp * w0[None, :] + torch.einsum("nhx,nx->nh", G[s], p) + c[s]
    relu_in = [x]
    a0, a1 = ("fc_1", "fc_0") if fault == "swap_fc" else ("fc_0", "fc_1")
    for i in range(layers):
        net = lin(torch.relu(x), W[f"blocks.{i}.{a0}.weight"], W[f"blocks.{i}.{a0}.bias"])
        relu_in.append(net if taps else None)
        x = x + lin(torch.relu(net), W[f"blocks.{i}.{a1}.weight"], W[f"blocks.{i}.{a1}.bias"])
        relu_in.append(x if taps else None)
    out = lin(x if fault == "no_last_relu" else torch.relu(x), W["fc_out.weight"], W["fc_out.bias"]).squeeze(-1)
    if loss_type == "occupancy" or fault == "sigmoid":
        out = torch.sigmoid(out)
    return dict(out=out, z_inv=z_inv, G=G, c=c, **({'relu_in': relu_in} if taps else {}))


def val_loss(net_out, sample_values):
    """(loss, acc, rec) of PointCloud_AE.get_val_loss (models/shape_pointcloud_modelAE.py:134-144) from its network output."""
    loss = torch.mean((net_out - sample_values) ** 2)
    pred = (net_out > 0.5).long()
    acc = torch.sum(pred == sample_values) / (pred.size(0) * pred.size(1))
    occ = sample_values == 1
    rec = torch.sum(pred[occ] == sample_values[occ]) / int(occ.sum())
    return loss, acc, rec
