#!/usr/bin/env python3
"""Golden fixture of the shape decoder, from the reference itself: tests/golden/shape_decoder.npz.

Same harness as make_golden.py / make_golden_r2.shape_encoder_fixture: the reference's own ``models`` package is imported in the
build container (third-party packages absent offline are supplied as stand-ins by make_golden.install_stand_ins) and its
``DecoderInner`` / ``PointCloud_AE`` (models/shape_pointcloud_modelAE.py:21-150) are filled with the hash weights of
``shapemol_amd.synth``; the list-held blocks are assigned directly.  Nothing here is imported by the product, the tests or the
bench.

    python tests/golden/make_golden_decoder.py

Contents: the decoder (hidden 128, latent 32, 4 blocks) on B = 3 shapes x T = 50 points under both loss types, with the
reference's z_inv; one PointCloud_AE.forward(inputs, None, point_coord) on 3 clouds of 64 points with its get_val_loss triple;
the key list of the reference's PointCloud_AE.state_dict().  The conditions that make the fixture worth comparing against are
asserted here, on the reference alone, and recorded in the file.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
from shapemol_amd import synth  # noqa: E402

t_ = G.t_
HIDDEN, LATENT, LAYERS, K = 128, 32, 4, 20
DEC_SEED, ENC_SEED = 19, 17
P_SCALE, Z_SCALE = 1.0, 0.5          # input scales: chosen so that the conditions asserted below hold


def load_decoder(dec, sd):
    dec.z_in.map_to_feat.weight.data = t_(sd["z_in.map_to_feat.weight"])
    for name in ("fc_in", "fc_out"):
        getattr(dec, name).weight.data = t_(sd[name + ".weight"])
        getattr(dec, name).bias.data = t_(sd[name + ".bias"])
    for i, blk in enumerate(dec.blocks):                       # a plain list in the reference: not in its state_dict
        for fc in ("fc_0", "fc_1"):
            getattr(blk, fc).weight.data = t_(sd[f"blocks.{i}.{fc}.weight"])
            getattr(blk, fc).bias.data = t_(sd[f"blocks.{i}.{fc}.bias"])


def load_encoder(enc, sd):
    def load(mod, prefix):
        mod.map_to_feat.weight.data = t_(sd[prefix + ".map_to_feat.weight"])
        mod.batchnorm.bn.weight.data = t_(sd[prefix + ".batchnorm.bn.weight"])
        mod.batchnorm.bn.bias.data = t_(sd[prefix + ".batchnorm.bn.bias"])
        mod.map_to_dir.weight.data = t_(sd[prefix + ".map_to_dir.weight"])
    load(enc.conv_pos, "conv_pos")
    for i, blk in enumerate(enc.blocks):
        load(blk, f"blocks.{i}")
    load(enc.conv_c, "conv_c")


def relu_inputs(dec, p, z):
    """Inputs of the 2 L + 1 ReLUs of one forward, taken by hooks on the reference's own sub-modules: fc_in's output, then
    each block's fc_0 output and the block's output."""
    taps, hooks = [], []
    hooks.append(dec.fc_in.register_forward_hook(lambda m, i, o: taps.append(o.detach())))
    for blk in dec.blocks:
        hooks.append(blk.fc_0.register_forward_hook(lambda m, i, o: taps.append(o.detach())))
        hooks.append(blk.register_forward_hook(lambda m, i, o: taps.append(o.detach())))
    zinv = []
    hooks.append(dec.z_in.register_forward_hook(lambda m, i, o: zinv.append((i[0] * o).sum(-1).detach())))
    with torch.no_grad():
        out = dec(p, z)
    for h in hooks:
        h.remove()
    return out, taps, zinv[0]


def main():
    G.install_stand_ins()
    from models.shape_pointcloud_modelAE import DecoderInner, PointCloud_AE
    sd = synth.shape_decoder_state_dict(HIDDEN, LATENT, LAYERS, seed=DEC_SEED)
    B, T = 3, 50
    p = (synth.hash_normal((B * T, 3), 611, 5) * np.float32(P_SCALE)).astype(np.float32).reshape(B, T, 3)
    z = (synth.hash_normal((B, LATENT, 3), 612, 5) * np.float32(Z_SCALE)).astype(np.float32)
    rec = dict(hidden=HIDDEN, latent_dim=LATENT, layers=LAYERS, k=K, dec_seed=DEC_SEED, enc_seed=ENC_SEED, p=p, z=z)
    for loss_type in ("signeddist", "occupancy"):
        dec = DecoderInner(3, LATENT, HIDDEN, LAYERS, loss_type)
        load_decoder(dec, sd)
        out, taps, z_inv = relu_inputs(dec, t_(p), t_(z))
        assert len(taps) == 2 * LAYERS + 1
        rec["out_" + loss_type] = out.numpy()
        if loss_type == "signeddist":
            o = out.numpy()
            span = float(o.max() - o.min()) / float(np.abs(o).max())
            assert span > 0.10, span                                              # the raw outputs are not one constant
            frac = np.array([float((t > 0).float().mean()) for t in taps])
            assert frac.min() >= 0.10 and frac.max() <= 0.90, frac                # every ReLU cuts: a missing or misplaced one shows
            rec.update(z_inv=z_inv.numpy(), out_span=span, relu_positive=frac)
        else:
            o = out.numpy()
            sat = float(((o <= 0.02) | (o >= 0.98)).mean())
            assert sat <= 0.10, sat                                               # the sigmoid is not saturated
            rec["sigmoid_saturated"] = sat
    # the auto-encoder: encoder and decoder of one PointCloud_AE
    cfg = types.SimpleNamespace(encoder="VN_DGCNN", hidden_dim=HIDDEN, latent_dim=LATENT, layer_num=LAYERS, num_k=K, point_dim=3,
                                loss_type="occupancy")
    ae = PointCloud_AE(cfg)                                                       # stays in train mode, as utils/shape.py:226-238 leaves it
    load_encoder(ae.encoder, synth.shape_encoder_state_dict(HIDDEN, LATENT, LAYERS, seed=ENC_SEED))
    load_decoder(ae.generator, sd)
    clouds = (synth.hash_normal((3, 64, 3), 621, 5) * np.array([1.5, 1.0, 0.6], np.float32)).astype(np.float32)
    q = (synth.hash_normal((3, 40, 3), 622, 5) * np.float32(P_SCALE)).astype(np.float32)
    vals = (synth.hash_u24(3 * 40, 623, 5) % 2).astype(np.float32).reshape(3, 40)
    with torch.no_grad():
        z_ae, net_out = ae(t_(clouds).unsqueeze(1), None, t_(q))
        loss, acc, rec_ = ae.get_val_loss(t_(clouds), t_(q), t_(vals))
    rec.update(ae_clouds=clouds, ae_q=q, ae_values=vals, ae_z=z_ae.numpy(), ae_out=net_out.numpy(),
               ae_val=np.array([float(loss), float(acc), float(rec_)], np.float64),
               ae_keys=np.array(sorted(ae.state_dict().keys())))
    np.savez_compressed(os.path.join(HERE, "shape_decoder.npz"), **rec)
    print("shape_decoder: span", rec["out_span"], "relu positive", np.round(rec["relu_positive"], 3), "saturated", rec["sigmoid_saturated"],
          "val", rec["ae_val"], "keys", len(rec["ae_keys"]), flush=True)


if __name__ == "__main__":
    main()
