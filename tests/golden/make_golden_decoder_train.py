#!/usr/bin/env python3
"""Golden fixture of the shape decoder's training gradients, from the reference itself: tests/golden/shape_decoder_train.npz
(inputs and the signed-distance run) and tests/golden/shape_decoder_train_occupancy.npz (the occupancy run).

Same harness as make_golden_decoder.py: the reference's ``PointCloud_AE`` (models/shape_pointcloud_modelAE.py:105-150; latent 32,
hidden 128, 2 blocks) is filled with the hash weights of ``shapemol_amd.synth`` (``fc_1.weight`` non-zero), then for both loss
types ``get_train_loss(point_clouds, sample_points, sample_values)`` and ``loss.backward()`` run on B = 3 clouds and T = 50 sample
points each.  Nothing here is imported by the product, the tests or the bench.

    python tests/golden/make_golden_decoder_train.py [--search]

Stored per loss type: the loss; ``.grad`` of every generator tensor -- the blocks, which the reference keeps in a plain list, are
leaves and do receive gradients, whatever its optimiser then does with them; the latent's gradient, taken by calling
``generator(point_coord, z)`` on the detached, grad-requiring encoder output.  And the same quantities from a float64 copy of the
reference's generator evaluated at the SAME latent (the float32 encoder's output, cast): the gate compares float32 evaluations of
one function of one input, and the encoder's own float32 error is not the decoder's.

Asserted here, on the reference alone: no point is fragile (some float64 ReLU input within 2^-18 of that ReLU's maximum, as
tests/shape_decoder_grad_f64.py::fragile), and every ReLU has 40-60 % positive inputs.  SEED is the first seed for which both
hold (``--search`` prints it).
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
import make_golden_decoder as GD  # noqa: E402
from shapemol_amd import synth  # noqa: E402

t_ = G.t_
HIDDEN, LATENT, LAYERS, K = 128, 32, 2, 20
DEC_SEED, ENC_SEED = 19, 17
B, T, CLOUD = 3, 50, 64
SEED = 7
FRAGILE = 2.0 ** -18
GEN_KEYS = ["z_in.map_to_feat.weight", "fc_in.weight", "fc_in.bias"] + \
           [f"blocks.{i}.{fc}.{w}" for i in range(LAYERS) for fc in ("fc_0", "fc_1") for w in ("weight", "bias")] + ["fc_out.weight", "fc_out.bias"]


def gen_tensor(dec, key):
    obj = dec
    for part in key.split("."):
        obj = obj[int(part)] if part.isdigit() else getattr(obj, part)
    return obj


def gen_double(dec):
    d = copy.deepcopy(dec).double()
    d.blocks = [copy.deepcopy(b).double() for b in dec.blocks]       # a plain list: .double() does not reach it
    return d


def zero_grads(dec):
    for k in GEN_KEYS:
        gen_tensor(dec, k).grad = None


def relu_taps(dec, p, z):
    taps, hooks = [], []
    hooks.append(dec.fc_in.register_forward_hook(lambda m, i, o: taps.append(o.detach())))
    for blk in dec.blocks:
        hooks.append(blk.fc_0.register_forward_hook(lambda m, i, o: taps.append(o.detach())))
        hooks.append(blk.register_forward_hook(lambda m, i, o: taps.append(o.detach())))
    with torch.no_grad():
        dec(p, z)
    for h in hooks:
        h.remove()
    return [t.reshape(-1, t.shape[-1]) for t in taps]


def inputs(seed):
    clouds = (synth.hash_normal((B, CLOUD, 3), 621, seed) * np.array([1.5, 1.0, 0.6], np.float32)).astype(np.float32)
    q = synth.hash_normal((B, T, 3), 622, seed).astype(np.float32)
    sdf = (synth.hash_normal((B, T), 624, seed) * np.float32(0.5)).astype(np.float32)
    occ = (synth.hash_u24(B * T, 623, seed) % 2).astype(np.float32).reshape(B, T)
    return clouds, q, {"signeddist": sdf, "occupancy": occ}


def build(loss_type):
    from models.shape_pointcloud_modelAE import PointCloud_AE
    cfg = types.SimpleNamespace(encoder="VN_DGCNN", hidden_dim=HIDDEN, latent_dim=LATENT, layer_num=LAYERS, num_k=K, point_dim=3,
                                loss_type=loss_type)
    ae = PointCloud_AE(cfg)
    GD.load_encoder(ae.encoder, synth.shape_encoder_state_dict(HIDDEN, LATENT, LAYERS, seed=ENC_SEED))
    GD.load_decoder(ae.generator, synth.shape_decoder_state_dict(HIDDEN, LATENT, LAYERS, seed=DEC_SEED))
    return ae


def conditions(ae, q, z):
    """(no point fragile, every ReLU 40-60 % positive, the fractions) from the float64 generator."""
    taps = relu_taps(gen_double(ae.generator), t_(q).double(), z.double())
    bad = torch.zeros(taps[0].shape[0], dtype=torch.bool)
    for v in taps:
        bad |= (v.abs() < FRAGILE * v.abs().max()).any(dim=1)
    frac = np.array([float((v > 0).double().mean()) for v in taps])
    return not bool(bad.any()), bool(frac.min() >= 0.40 and frac.max() <= 0.60), frac


def record(seed):
    clouds, q, values = inputs(seed)
    rec = dict(hidden=HIDDEN, latent_dim=LATENT, layers=LAYERS, k=K, dec_seed=DEC_SEED, enc_seed=ENC_SEED, seed=seed, clouds=clouds, q=q)
    ok = True
    for loss_type in ("signeddist", "occupancy"):
        ae = build(loss_type)
        vals = values[loss_type]
        zero_grads(ae.generator)
        loss = ae.get_train_loss(t_(clouds), t_(q), t_(vals))
        loss.backward()
        grads = {k: gen_tensor(ae.generator, k).grad.detach().clone() for k in GEN_KEYS}
        # the latent (train mode: the encoder's batch norm uses the batch's statistics, as in get_train_loss) and its gradient
        with torch.no_grad():
            z = ae.encoder(t_(clouds).unsqueeze(1))
        zero_grads(ae.generator)
        zl = z.detach().clone().requires_grad_(True)
        loss_z = torch.mean((ae.generator(t_(q), zl) - t_(vals)) ** 2)
        loss_z.backward()
        assert float(loss_z.detach()) == float(loss.detach())
        for k in GEN_KEYS:
            assert torch.equal(gen_tensor(ae.generator, k).grad, grads[k]), k
        # float64 generator at the same latent
        g64 = gen_double(ae.generator)
        z64 = z.double().clone().requires_grad_(True)
        loss64 = torch.mean((g64(t_(q).double(), z64) - t_(vals).double()) ** 2)
        loss64.backward()
        fine, cut, frac = conditions(ae, q, z)
        ok = ok and fine and cut
        rec.update({f"values_{loss_type}": vals, f"z_{loss_type}": z.numpy(), f"loss_{loss_type}": np.float32(float(loss.detach())),
                    f"loss64_{loss_type}": np.float64(float(loss64.detach())), f"dz_{loss_type}": zl.grad.numpy(), f"dz64_{loss_type}": z64.grad.numpy(),
                    f"relu_positive_{loss_type}": frac})
        for k in GEN_KEYS:
            rec[f"grad_{loss_type}.{k}"] = grads[k].numpy()
            rec[f"grad64_{loss_type}.{k}"] = gen_tensor(g64, k).grad.numpy()
    return rec, ok


def main():
    G.install_stand_ins()
    torch.set_num_threads(8)
    if "--search" in sys.argv:
        for seed in range(1, 200):
            _, ok = record(seed)
            print("seed", seed, ok, flush=True)
            if ok:
                return
        raise SystemExit("no seed found")
    rec, ok = record(SEED)
    assert ok, ("fragile point or a ReLU outside 40-60 %", rec["relu_positive_signeddist"], rec["relu_positive_occupancy"])
    rec["gen_keys"] = np.array(GEN_KEYS)
    # two files, since one would pass the repository's limit of 1 MiB per file: the occupancy run's records on their own
    occ = {k: v for k, v in rec.items() if k.endswith("_occupancy") or "_occupancy." in k}
    np.savez_compressed(os.path.join(HERE, "shape_decoder_train.npz"), **{k: v for k, v in rec.items() if k not in occ})
    np.savez_compressed(os.path.join(HERE, "shape_decoder_train_occupancy.npz"), **occ)
    print("shape_decoder_train: loss", rec["loss_signeddist"], rec["loss_occupancy"], "relu positive", np.round(rec["relu_positive_signeddist"], 3), flush=True)


if __name__ == "__main__":
    main()
