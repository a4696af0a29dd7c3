#!/usr/bin/env python3
"""Times one training step of the shape decoder's loss (forward + backward of mean((net_out - values)^2) through
DecoderInner.train_field) on one GPU, warm, median of repeated steps, at

  32 x 2048   32 shapes of 2048 sample points (this tool's choice: the reference ships no auto-encoder training config in its tree)
  3 x 50      the fixture's size

next to torch device autograd of the same MLP on the same inputs (the reference's concatenated formulation; gradients of every
parameter, z and p) and next to decode_grad alone (the sweep without the stores and without any parameter gradient).  Prints one
JSON line.  The achieved fraction is of the peak of v_mfma_f32_16x16x4_f32, 157.3 TFLOP/s on an MI355X, counting what a step
must execute: the forward (2 L Linears), the two transposed products per block of the way back, and the 2 L weight-gradient
products -- 3 x the forward's matrix work.

    python tools/shape_decoder_train_bench.py [--reps 20] [--warmup 3]

How the time splits between the sweep (sd_train_kernel) and the weight-gradient products (sd_dw_kernel) is a per-kernel figure:
run this tool under `rocprofv3 --kernel-trace --stats -- python tools/shape_decoder_train_bench.py --reps 5 --only 32x2048`.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from shapemol_amd import synth  # noqa: E402
from shapemol_amd.shape_autoencoder import DecoderInner  # noqa: E402
from shape_decoder_bench import H, L, PEAK_FP32_MFMA, Z, timed  # noqa: E402


def torch_step(params, loss_type):
    lin = torch.nn.functional.linear

    def f(p, z, v):
        W = params
        z_dir = torch.einsum("mk,bkx->bmx", W["z_in.map_to_feat.weight"], z)
        z_inv = (z * z_dir).sum(-1)
        feat = torch.cat([(p * p).sum(-1, keepdim=True), torch.einsum("bmi,bni->bmn", p, z), z_inv[:, None, :].expand(-1, p.shape[1], -1)], dim=2)
        x = lin(feat, W["fc_in.weight"], W["fc_in.bias"])
        for i in range(L):
            net = lin(torch.relu(x), W[f"blocks.{i}.fc_0.weight"], W[f"blocks.{i}.fc_0.bias"])
            x = x + lin(torch.relu(net), W[f"blocks.{i}.fc_1.weight"], W[f"blocks.{i}.fc_1.bias"])
        out = lin(torch.relu(x), W["fc_out.weight"], W["fc_out.bias"]).squeeze(-1)
        out = torch.sigmoid(out) if loss_type == "occupancy" else out
        return torch.autograd.grad(torch.mean((out - v) ** 2), [p, z] + list(W.values()))
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    loss_type = "signeddist"
    sd = synth.shape_decoder_state_dict(H, Z, L, seed=19)
    dec = DecoderInner(3, Z, H, L, loss_type)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    dec = dec.cuda()
    params = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in sd.items()}
    ref = torch_step(params, loss_type)
    res = {"device": torch.cuda.get_device_name(0), "hidden": H, "latent": Z, "layers": L, "peak_tflops_fp32_mfma": PEAK_FP32_MFMA / 1e12, "reps": a.reps}
    for B, T in ((32, 2048), (3, 50)):
        name = f"{B}x{T}"
        if a.only and a.only != name:
            continue
        p = torch.from_numpy(synth.hash_normal((B, T, 3), 611, 5).astype(np.float32)).cuda().requires_grad_(True)
        z = torch.from_numpy((synth.hash_normal((B, Z, 3), 612, 5) * np.float32(0.5)).astype(np.float32)).cuda().requires_grad_(True)
        v = torch.from_numpy((synth.hash_normal((B, T), 613, 5) * np.float32(0.5)).astype(np.float32)).cuda()

        def step():
            for q in dec.parameters():
                q.grad = None
            p.grad = z.grad = None
            torch.mean((dec.train_field(p, z) - v) ** 2).backward()
        med, best = timed(step, a.reps, a.warmup)
        tmed, tbest = timed(lambda: ref(p, z, v), a.reps, a.warmup)
        gmed, gbest = timed(lambda: dec.decode_grad(p.detach(), z.detach()), a.reps, a.warmup)
        step()
        tg = ref(p, z, v)
        names = ["p", "z"] + list(params)
        mine = [p.grad, z.grad] + [dict(dec.named_parameters())[k].grad for k in params]
        rel = [float((x - y).abs().max() / y.abs().max().clamp(min=1e-30)) for x, y in zip(mine, tg)]
        # (a ReLU input near 0 may fall on either side in two float32 evaluations: that point's dp then differs by a whole
        # column of a weight matrix, while a sum over the points barely moves -- so dp is reported apart from z and the weights)
        diff = {"p": rel[0], "z": rel[1], "weights": max(rel[2:])}
        n = B * T
        flops = 3 * 2 * n * 2 * L * H * H
        res[name] = {"points": n, "step_ms_median": med, "step_ms_min": best, "torch_autograd_ms_median": tmed, "torch_autograd_ms_min": tbest,
                     "speedup_vs_torch_autograd": tmed / med, "decode_grad_ms_median": gmed, "step_over_decode_grad": med / gmed,
                     "tflops": flops / med / 1e9, "fraction_of_peak": flops / (med * 1e-3) / PEAK_FP32_MFMA,
                     "max_rel_diff_vs_torch_autograd": diff, "tensors": len(names)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
