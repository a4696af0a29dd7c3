#!/usr/bin/env python3
"""Golden fixture of the gradient shape guidance, from the reference itself: tests/golden/field_guidance.npz.

Same harness as make_golden_decoder.py: the reference's own ``DecoderInner`` (models/shape_pointcloud_modelAE.py:69-103) is
filled with the hash weights of ``shapemol_amd.synth`` (the list-held blocks are assigned directly), and the arithmetic of the
reference's `use_grad` block (models/molopt_score_model.py:592-615) is applied per molecule with torch.autograd on the CPU.

    python tests/golden/make_golden_field_guidance.py

Contents, for B = 3 molecules of 7, 12 and 9 atoms, latent 32, 4 blocks, both loss types: ``out``; the autograd gradient of
mean(clip(out, max=0.5) - 0.5) per molecule, exactly as the block takes it; the updated positions for one ``grad_lr``.  Asserted
here: both d < 0.5 and d >= 0.5 occur for both loss types, and the fragile cap of tests/shape_decoder_grad_f64.py holds.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
from make_golden_decoder import HIDDEN, LATENT, LAYERS, DEC_SEED, load_decoder  # noqa: E402
from shapemol_amd import synth  # noqa: E402

t_ = G.t_
COUNTS, GRAD_LR, SEED, P_SCALE, Z_SCALE = (7, 12, 9), 2.0, 5, 1.3, 0.5


def main():
    G.install_stand_ins()
    from models.shape_pointcloud_modelAE import DecoderInner
    import shape_decoder_f64 as D
    import shape_decoder_grad_f64 as DG
    sd = synth.shape_decoder_state_dict(HIDDEN, LATENT, LAYERS, seed=DEC_SEED)
    n, B = sum(COUNTS), len(COUNTS)
    p = (synth.hash_normal((n, 3), 611, SEED) * np.float32(P_SCALE)).astype(np.float32)
    z = (synth.hash_normal((B, LATENT, 3), 612, SEED) * np.float32(Z_SCALE)).astype(np.float32)
    batch = np.repeat(np.arange(B), COUNTS).astype(np.int64)
    rec = dict(hidden=HIDDEN, latent_dim=LATENT, layers=LAYERS, dec_seed=DEC_SEED, p=p, z=z, batch=batch, grad_lr=GRAD_LR)
    for loss_type in ("signeddist", "occupancy"):
        dec = DecoderInner(3, LATENT, HIDDEN, LAYERS, loss_type)
        load_decoder(dec, sd)
        pos = t_(p).clone()
        outs, grads = [], []
        for j in range(B):                                        # the reference's block, molecule by molecule
            idx = torch.where(t_(batch) == j)
            single = pos[idx].unsqueeze(0).clone().requires_grad_(True)
            d = dec(single, t_(z)[j].unsqueeze(0))
            outs.append(d.detach()[0].clone())
            d = torch.clip(d, max=0.5) - 0.5
            m = torch.mean(d)
            g = torch.autograd.grad(m, single)[0]
            grads.append(g[0])
            pos[idx] = pos[idx] - GRAD_LR * d.detach().unsqueeze(2).repeat(1, 1, 3)[0] * g[0]
        out = torch.cat(outs).numpy()
        assert (out < 0.5).any() and (out >= 0.5).any(), (loss_type, out.min(), out.max())
        ref = DG.reference(D.state_dict(LAYERS, LATENT, seed=DEC_SEED), t_(p), t_(batch), t_(z), LAYERS, loss_type)
        assert DG.cap_ok(ref["fragile"]), int(ref["fragile"].sum())
        rec["out_" + loss_type], rec["grad_" + loss_type], rec["pos_" + loss_type] = out, torch.cat(grads).numpy(), pos.numpy()
        print(loss_type, "inside", int((out < 0.5).sum()), "outside", int((out >= 0.5).sum()), "fragile", int(ref["fragile"].sum()), flush=True)
    np.savez_compressed(os.path.join(HERE, "field_guidance.npz"), **rec)


if __name__ == "__main__":
    main()
