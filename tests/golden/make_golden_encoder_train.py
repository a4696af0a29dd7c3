#!/usr/bin/env python3
"""Golden fixture of the shape encoder's training gradients, from the reference itself: tests/golden/shape_encoder_train.npz.

Same harness as make_golden_decoder_train.py: the reference's ``PointCloud_AE`` (models/shape_pointcloud_modelAE.py:105-150; latent 32,
hidden 128, signed distance) is filled with the hash weights of ``shapemol_amd.synth``, then ``get_train_loss(point_clouds,
sample_points, sample_values)`` and ``loss.backward()`` run on B = 3 clouds of N = 32 points and T = 50 sample points each, in float32
and in a float64 copy of the whole model.  Nothing here is imported by the product, the tests or the bench.

    python tests/golden/make_golden_encoder_train.py [--search]

Stored, in float32 and compressed: the inputs, the float32 loss, ``.grad`` of every encoder tensor from the float32 run (``grad.<key>``),
and the float32 run's error against the float64 run (``err.<key>`` = grad32 - grad64; the float64 gradient is grad - err to within
1e-7 of the error, which is all the gate's e32 needs).  layer_num is 1: with two blocks the two records pass the repository's limit of
1 MiB per file.  The blocks, which the reference keeps in a plain list, are leaves and do receive gradients.

Asserted here (tests/shape_encoder_train_f64.py on the same weights and clouds): float32 and float64 choose the same neighbour lists
at every stage and the same leaky-ReLU branch at every element.  SEED is the first seed for which both hold (``--search`` prints
it).  The cosine margin of 100 does not exist on hash weights (shape_encoder_train_f64.state_dict); the measured ratio is recorded.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
import make_golden_decoder as GD  # noqa: E402
import shape_encoder_f64 as F  # noqa: E402
import shape_encoder_train_f64 as TR  # noqa: E402
from shapemol_amd import synth  # noqa: E402

t_ = G.t_
HIDDEN, LATENT, LAYERS, K = 128, 32, 1, 20
DEC_SEED, ENC_SEED = 19, 17
B, T, N = 3, 50, 32
SEED = 2
ENC_KEYS = TR.keys(LAYERS)


def enc_tensor(enc, key):
    obj = enc
    for part in key.split("."):
        obj = obj[int(part)] if part.isdigit() else getattr(obj, part)
    return obj


def inputs(seed):
    clouds = (synth.hash_normal((B, N, 3), 631, seed) * np.array([1.5, 1.0, 0.6], np.float32)).astype(np.float32)
    q = synth.hash_normal((B, T, 3), 632, seed).astype(np.float32)
    sdf = (synth.hash_normal((B, T), 634, seed) * np.float32(0.5)).astype(np.float32)
    return clouds, q, sdf


def build():
    from models.shape_pointcloud_modelAE import PointCloud_AE
    cfg = types.SimpleNamespace(encoder="VN_DGCNN", hidden_dim=HIDDEN, latent_dim=LATENT, layer_num=LAYERS, num_k=K, point_dim=3,
                                loss_type="signeddist")
    ae = PointCloud_AE(cfg)
    GD.load_encoder(ae.encoder, synth.shape_encoder_state_dict(HIDDEN, LATENT, LAYERS, seed=ENC_SEED))
    GD.load_decoder(ae.generator, synth.shape_decoder_state_dict(HIDDEN, LATENT, LAYERS, seed=DEC_SEED))
    return ae


def to_double(ae):
    d = copy.deepcopy(ae).double()
    d.encoder.blocks = [copy.deepcopy(b).double() for b in ae.encoder.blocks]        # plain lists: .double() does not reach them
    d.generator.blocks = [copy.deepcopy(b).double() for b in ae.generator.blocks]
    return d


def grads(ae, clouds, q, vals, dtype):
    for k in ENC_KEYS:
        enc_tensor(ae.encoder, k).grad = None
    loss = ae.get_train_loss(t_(clouds).to(dtype), t_(q).to(dtype), t_(vals).to(dtype))
    loss.backward()
    return float(loss.detach()), {k: enc_tensor(ae.encoder, k).grad.detach().clone() for k in ENC_KEYS}


def wellposed(clouds):
    """TR.wellposed's measurements for these clouds on the synth weights (the reference's model computes the same function)."""
    sd = F.state_dict(LAYERS, LATENT, seed=ENC_SEED)
    pts = t_(clouds)
    f32, f64 = F.forward(sd, pts, LAYERS, F.F32), F.forward(sd, pts, LAYERS, F.F64)
    same_lists = all(torch.equal(a["idx"].sort(-1)[0], b["idx"].sort(-1)[0]) for a, b in zip(f32["stops"], f64["stops"]))
    if not same_lists:
        return dict(same_lists=False, same_masks=False, ratio=0.0)
    idx = torch.stack([s["idx"] for s in f64["stops"]])
    up = TR.upstream((B, LATENT, 3))
    _, i32 = TR.device_form(sd, pts, LAYERS, idx, F.F32, g_out=up)
    _, i64 = TR.device_form(sd, pts, LAYERS, idx, F.F64, g_out=up)
    least = min(float(c.abs().min()) for c in i64["cos"].values())
    diff = max(float((i32["cos"][k].double() - i64["cos"][k]).abs().max()) for k in i64["cos"])
    return dict(same_lists=True, same_masks=bool(all(torch.equal(i32["masks"][k], i64["masks"][k]) for k in i64["masks"])), ratio=least / diff)


def main():
    G.install_stand_ins()
    torch.set_num_threads(8)
    if "--search" in sys.argv:
        for seed in range(1, 400):
            w = wellposed(inputs(seed)[0])
            print("seed", seed, w, flush=True)
            if w["same_lists"] and w["same_masks"]:
                return
        raise SystemExit("no seed found")
    clouds, q, vals = inputs(SEED)
    w = wellposed(clouds)
    assert w["same_lists"] and w["same_masks"], w
    ae = build()
    loss32, g32 = grads(ae, clouds, q, vals, torch.float32)
    loss64, g64 = grads(to_double(ae), clouds, q, vals, torch.float64)
    # the reference's model is the function tests/shape_encoder_train_f64.py restates: its float64 gradient on the float64 lists
    rec = dict(hidden=HIDDEN, latent_dim=LATENT, layers=LAYERS, k=K, dec_seed=DEC_SEED, enc_seed=ENC_SEED, seed=SEED, clouds=clouds, q=q, values=vals,
               loss=np.float32(loss32), loss64=np.float64(loss64), cos_ratio=np.float64(w["ratio"]), enc_keys=np.array(ENC_KEYS))
    for k in ENC_KEYS:
        rec["grad." + k] = g32[k].numpy().astype(np.float32)
        rec["err." + k] = (g32[k].double() - g64[k]).numpy().astype(np.float32)
    path = os.path.join(HERE, "shape_encoder_train.npz")
    np.savez_compressed(path, **rec)
    print("shape_encoder_train: loss", loss32, loss64, "cos ratio", w["ratio"], "bytes", os.path.getsize(path), flush=True)


if __name__ == "__main__":
    main()
