"""The shape decoder's gradient with respect to the query points and the gradient shape guidance built on it, on the CPU in
float64 and float32 (tests/test_shape_decoder_grad_cpu.py, tests/test_gpu_field_guidance.py).

The value is tests/shape_decoder_f64.decode (differentiable torch); the gradient is autograd's of out.sum() with respect to p.

Fragile points.  A ReLU network's gradient is piecewise constant: where a ReLU input v of a point is nearly 0, float32 and
float64 may land on different linear pieces and their gradients differ by a whole column of a weight matrix -- which is no
error of either.  A point is FRAGILE in a case when some ReLU input of its float64 evaluation has |v| < 2^-18 max|v|, the
max over that ReLU input across the case.  2^-18 = 3.8e-6 lies above what the forward gate 4 e32 + 16 * 2^-24 lets a
pre-activation be off by (about 2e-6), so a decoder that passes the forward gate cannot flip a mask outside the set.
Fragile points are left out of the gradient gate (their device values must be finite); a case of 16 or more points may lose
at most 1/8 of them, a smaller case none (cap_ok) -- asserted from the float64 data alone.

The gate is the project's: eH <= 4 e32 + 16 * 2^-24, on the three components together, max-normalised over the kept points.

`device_form` recomposes the gradient as the kernel does (sm_shape_dec_grad.h): factored fc_in, masks m = (v > 0), transposed
products last block to first, grad = 2 p (w0 . g) + G^T g.  Its `fault` and guide's are the negative controls.
"""
import numpy as np
import torch

import shape_decoder_f64 as D
from precision import bound, rel_err
from util import O, T, hash_noise, oracle_model, synth

F64, F32 = D.F64, D.F32
FRAGILE = 2.0 ** -18
GRAD_FAULTS = ("no_2pw0", "no_last_mask", "other_shape", "no_sigmoid_slope")
GUIDE_FAULTS = ("no_count", "no_indicator")
GOLDEN = D.GOLDEN.replace("shape_decoder.npz", "field_guidance.npz")


def value_grad(sd, p, shape_of, z, layers, loss_type, dtype=F64):
    """(out (N,), grad (N, 3), relu_in [2 L + 1] of (N, H)) in `dtype`: autograd through shape_decoder_f64.decode."""
    q = p.detach().to(dtype).clone().requires_grad_(True)
    r = D.decode(sd, q, shape_of, z, layers, loss_type, dtype, taps=True)
    g, = torch.autograd.grad(r["out"].sum(), q)
    return r["out"].detach(), g, [t.detach() for t in r["relu_in"]]


def fragile(relu_in, margin=FRAGILE):
    """(N,) bool from the float64 ReLU inputs of a case."""
    bad = torch.zeros(relu_in[0].shape[0], dtype=torch.bool)
    for v in relu_in:
        bad |= (v.abs() < margin * v.abs().max()).any(dim=1)
    return bad


def cap_ok(frag):
    n = int(frag.numel())
    return int(frag.sum()) * 8 <= n if n >= 16 else not bool(frag.any())


def reference(sd, p, shape_of, z, layers, loss_type):
    """dict of the float64 and float32 values and gradients of a case, its fragile set and `keep` = ~fragile."""
    o64, g64, taps = value_grad(sd, p, shape_of, z, layers, loss_type, F64)
    o32, g32, _ = value_grad(sd, p, shape_of, z, layers, loss_type, F32)
    frag = fragile(taps)
    return dict(out64=o64, grad64=g64, out32=o32, grad32=g32, fragile=frag, keep=~frag, relu_in=taps)


def prefix(ref, n):
    """reference() of the first n points of a case: the same values, the fragile set from the maxima over those n points."""
    sub = {k: v[:n] for k, v in ref.items() if k != "relu_in"}
    sub["relu_in"] = [t[:n] for t in ref["relu_in"]]
    sub["fragile"] = fragile(sub["relu_in"])
    sub["keep"] = ~sub["fragile"]
    return sub


def tail_case(cus, tile=None):
    """(p, shape_of, z, totals) of the launch-tail test on a device of `cus` compute units: both shapes inside every tile."""
    tile = tile or DECODE_TILE
    full = 2 * cus * tile + 1
    p, _, z = D.inputs(2, [full, 0], 32, 7)
    s = torch.from_numpy((np.arange(full) * 7 // 5) % 2)
    return p, s, z, (cus * tile - 1, cus * tile, cus * tile + 1, 2 * cus * tile + 1)


def grad_gate(res, ref):
    """(eH, e32, passed) of a gradient (N, 3) against a reference() on its kept points."""
    k = ref["keep"]
    res = torch.as_tensor(res)
    eh, e32 = rel_err(res[k].numpy(), ref["grad64"][k].numpy()), rel_err(ref["grad32"][k].numpy(), ref["grad64"][k].numpy())
    return eh, e32, eh <= bound(e32)


def guide(p, out, grad, shape_of, n_shapes, grad_lr, fault=None):
    """The reference's update (models/molopt_score_model.py:592-615) from a value and a gradient of any dtype:
    p' = p - grad_lr (min(d, 0.5) - 0.5) (1[d < 0.5] / T_j) grad."""
    assert fault is None or fault in GUIDE_FAULTS, fault
    cnt = torch.bincount(shape_of, minlength=n_shapes).clamp(min=1).to(out.dtype)[shape_of]
    if fault == "no_count":
        cnt = torch.ones_like(cnt)
    e = out.clamp(max=0.5) - 0.5
    ind = torch.ones_like(out) if fault == "no_indicator" else (out < 0.5).to(out.dtype)
    if fault == "no_indicator":
        e = out - 0.5
    return p.to(out.dtype) - grad_lr * (e * ind / cnt)[:, None] * grad


def guide_reference_loop(sd, p, shape_of, z, layers, loss_type, grad_lr, dtype=F64):
    """The update exactly as the reference's block takes it: per molecule, autograd of mean(clip(d, max=0.5) - 0.5)."""
    out = p.detach().to(dtype).clone()
    for j in range(z.shape[0]):
        idx = torch.where(shape_of == j)[0]
        if idx.numel() == 0:
            continue
        q = out[idx].clone().requires_grad_(True)
        d = D.decode(sd, q, torch.zeros(idx.numel(), dtype=torch.int64), z[j:j + 1], layers, loss_type, dtype)["out"]
        d = torch.clip(d, max=0.5) - 0.5
        m = d.mean()
        if float(m.detach()) == 0.0:
            continue
        g, = torch.autograd.grad(m, q)
        out[idx] = out[idx] - grad_lr * d.detach()[:, None] * g
    return out


def device_form(sd, p, shape_of, z, layers, loss_type, dtype=F32, fault=None):
    """(out, grad) by reverse mode in the device's form, every operation in `dtype`."""
    assert fault is None or fault in GRAD_FAULTS, fault
    W = {k: v.to(dtype) for k, v in sd.items()}
    p, z = p.to(dtype), z.to(dtype)
    Z = z.shape[1]
    z_dir = torch.einsum("mk,bkx->bmx", W["z_in.map_to_feat.weight"], z)
    z_inv = (z * z_dir).sum(-1)
    w_in = W["fc_in.weight"]
    w0, wz, wi = w_in[:, 0], w_in[:, 1:1 + Z], w_in[:, 1 + Z:]
    G = torch.einsum("hm,bmx->bhx", wz, z)
    c = z_inv @ wi.T + W["fc_in.bias"]
    x = (p * p).sum(-1, keepdim=True) * w0[None, :] + torch.einsum("nhx,nx->nh", G[shape_of], p) + c[shape_of]
    masks = []
    for i in range(layers):
        masks.append(x > 0)
        net = torch.relu(x) @ W[f"blocks.{i}.fc_0.weight"].T + W[f"blocks.{i}.fc_0.bias"]
        masks.append(net > 0)
        x = x + (torch.relu(net) @ W[f"blocks.{i}.fc_1.weight"].T + W[f"blocks.{i}.fc_1.bias"])
    m_last = x > 0
    out = (torch.relu(x) @ W["fc_out.weight"].T + W["fc_out.bias"]).squeeze(-1)
    g = W["fc_out.weight"].expand(p.shape[0], -1)
    if fault != "no_last_mask":
        g = g * m_last
    if loss_type == "occupancy":
        out = torch.sigmoid(out)
        if fault != "no_sigmoid_slope":
            g = g * (out * (1 - out))[:, None]
    for i in reversed(range(layers)):
        gy = (g @ W[f"blocks.{i}.fc_1.weight"]) * masks[2 * i + 1]           # W1^T g
        g = g + (gy @ W[f"blocks.{i}.fc_0.weight"]) * masks[2 * i]           # W0^T g_y
    s = (shape_of + 1) % z.shape[0] if fault == "other_shape" else shape_of
    grad = torch.einsum("nhx,nh->nx", G[s], g)
    if fault != "no_2pw0":
        grad = grad + 2 * p * (g @ w0)[:, None]
    return out, grad


def central_differences(sd, p, shape_of, z, layers, loss_type, h=1e-6):
    """(N, 3) float64 central differences of the float64 value."""
    p = p.to(F64)
    cols = []
    for k in range(3):
        e = torch.zeros(3, dtype=F64)
        e[k] = h
        up = D.decode(sd, p + e, shape_of, z, layers, loss_type, F64)["out"]
        dn = D.decode(sd, p - e, shape_of, z, layers, loss_type, F64)["out"]
        cols.append((up - dn) / (2 * h))
    return torch.stack(cols, dim=1)


def ragged_counts(kind):
    """Atom counts of the stand-alone update's cases: a one-atom molecule among larger ones; 40 molecules of 1 to 3 atoms."""
    return (7, 1, 12, 5, 9) if kind == "ragged5" else tuple(1 + (i * 7) % 3 for i in range(40))


# ---- the cases of tests/test_gpu_field_guidance.py whose seeds are chosen here, on the CPU (tests/test_shape_decoder_grad_cpu.py
# checks the fragile cap of each) --------------------------------------------------------------------------------------------
DECODE_TILE = 256                                          # shapemol_sd_tile (the GPU test reads it from the library)
SIZE_SEEDS = {(1, 32, "signeddist"): 201, (8, 32, "signeddist"): 208, (4, 1, "signeddist"): 241, (4, 256, "signeddist"): 242,
              (4, 32, "occupancy"): 243, (8, 256, "occupancy"): 244}
CHAIN_B, CHAIN_STEPS, CHAIN_LR, CHAIN_SEED = 4, 20, 4.0, 1
CHAIN_MARGIN = 2.0 ** -21


def edge_seed(T):
    """Seed of the tile-edge case of T points per shape (T = 15 with seed 115 has 4 fragile points of 30: above the cap)."""
    return 1015 if T == 15 else 100 + T


def size_z_scale(Z):
    return 0.5 / max(1.0, (Z / 32.0) ** 0.5)


def chain_inputs(seed):
    bb = synth.synthetic_batch(CHAIN_B, seed=seed, atoms_range=(5, 8))
    eps, u = hash_noise(len(bb["batch"]), CHAIN_STEPS, seed)
    return bb, eps, u


def oracle_chain(bb, eps, u, grad_lr, grad_step):
    """The reference's guided chain on the CPU: oracle.score, the float64 field update of the float32 prediction while
    t > grad_step, oracle.posterior_step.  -> (pos, v, the predictions the posterior step consumed, the least |v| / max|v| over
    the ReLU inputs of the guided steps)."""
    sd, dm, _cfg, _ = oracle_model()
    dsd = D.state_dict(4, 32)
    pos, v, batch = T(bb["init_pos"]), T(bb["init_v"]), T(bb["batch"])
    shape = T(bb["shape"]).view(CHAIN_B, -1, 3)
    preds, least = [], np.inf
    for st in range(CHAIN_STEPS):
        t = torch.full((CHAIN_B,), dm.T - 1 - st, dtype=torch.int64)
        out = O.score(sd, dm, pos, v, batch, shape, t)
        pred = out["pred_ligand_pos"]
        if grad_lr is not None and dm.T - 1 - st > grad_step:
            o64, g64, taps = value_grad(dsd, pred, batch, shape, 4, "signeddist", F64)
            least = min(least, min(float((tp.abs() / tp.abs().max()).min()) for tp in taps))
            pred = guide(pred, o64, g64, batch, CHAIN_B, grad_lr).float()
        preds.append(pred)
        pos, v, _, _ = O.posterior_step(sd, dm, pos, v, pred, out["pred_ligand_v"], batch, t, T(eps[st]), T(u[st]))
    return pos, v, preds, least
