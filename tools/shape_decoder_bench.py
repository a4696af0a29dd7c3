#!/usr/bin/env python3
"""Times the device shape decoder (shapemol_amd.shape_autoencoder.DecoderInner) on one GPU, warm, median of repeated launches:

  grid   a 64^3 grid of query points for each of 16 shapes (4.2 M points), DecoderInner.forward
  atoms  256 molecules of 9..34 atoms (about 5.5 k atoms), DecoderInner.decode_atoms

and, as the baseline the kernel is judged against, the same MLP evaluated with torch device ops in fp32 on the same inputs
(the reference's formulation: concatenated feature, nn.functional.linear per layer; on the grid in the reference's dense form,
einsum 'bmi,bni->bmn' over (B, T, 3) in one piece, on the atoms with the latent gathered per atom).  Prints one JSON line.  The achieved
fraction is of the peak of the instruction the kernel uses, v_mfma_f32_16x16x4_f32: 157.3 TFLOP/s on an MI355X.

    python tools/shape_decoder_bench.py [--reps 20] [--warmup 3] [--grad]

--grad adds, per workload, the value-and-gradient kernel (decode_grad / decode_atoms_grad) next to the decode kernel in the same
run, torch device autograd of the same MLP (forward + autograd.grad of the sum with respect to the points), and on the atoms the
guidance pass guide_atoms.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shapemol_amd import synth  # noqa: E402
from shapemol_amd.shape_autoencoder import DecoderInner  # noqa: E402

PEAK_FP32_MFMA = 157.3e12
H, Z, L = 128, 32, 4


def flops_per_point():
    """What the kernel executes: fc_in factored (4 FMA per unit), 2 L Linears of H x H, fc_out."""
    return 2 * (4 * H + 2 * L * H * H + H)


def torch_decoder(sd, loss_type):
    W = {k: torch.from_numpy(v).cuda() for k, v in sd.items()}
    lin = torch.nn.functional.linear

    def f(p, shape_of, z):
        """p (B, T, 3) with shape_of None (dense), or p (N, 3) with a shape index per point."""
        z_dir = torch.einsum("mk,bkx->bmx", W["z_in.map_to_feat.weight"], z)
        z_inv = (z * z_dir).sum(-1)
        if shape_of is None:
            feat = torch.cat([(p * p).sum(-1, keepdim=True), torch.einsum("bmi,bni->bmn", p, z), z_inv[:, None, :].expand(-1, p.shape[1], -1)], dim=2)
        else:
            feat = torch.cat([(p * p).sum(-1, keepdim=True), torch.einsum("nx,nmx->nm", p, z[shape_of]), z_inv[shape_of]], dim=1)
        x = lin(feat, W["fc_in.weight"], W["fc_in.bias"])
        for i in range(L):
            net = lin(torch.relu(x), W[f"blocks.{i}.fc_0.weight"], W[f"blocks.{i}.fc_0.bias"])
            x = x + lin(torch.relu(net), W[f"blocks.{i}.fc_1.weight"], W[f"blocks.{i}.fc_1.bias"])
        out = lin(torch.relu(x), W["fc_out.weight"], W["fc_out.bias"]).squeeze(-1)
        return torch.sigmoid(out) if loss_type == "occupancy" else out
    return f


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--grad", action="store_true")
    a = ap.parse_args()
    loss_type = "signeddist"
    sd = synth.shape_decoder_state_dict(H, Z, L, seed=19)
    dec = DecoderInner(3, Z, H, L, loss_type)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    dec = dec.cuda()
    ref = torch_decoder(sd, loss_type)
    res = {"device": torch.cuda.get_device_name(0), "hidden": H, "latent": Z, "layers": L, "flops_per_point": flops_per_point(),
           "peak_tflops_fp32_mfma": PEAK_FP32_MFMA / 1e12, "reps": a.reps}
    # grid workload
    B, g = 16, a.grid
    ax = torch.linspace(-4.0, 4.0, g)
    pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(1, -1, 3).repeat(B, 1, 1).contiguous().cuda()
    z = torch.from_numpy((synth.hash_normal((B, Z, 3), 612, 5) * np.float32(0.5)).astype(np.float32)).cuda()
    n = B * g ** 3
    med, best = timed(lambda: dec(pts, z), a.reps, a.warmup)
    tmed, tbest = timed(lambda: ref(pts, None, z), max(3, a.reps // 4), 1)
    d = float((dec(pts, z) - ref(pts, None, z)).abs().max())
    res["grid"] = {"points": n, "ms_median": med, "ms_min": best, "points_per_s": n / med * 1e3, "tflops": n * flops_per_point() / med / 1e9,
                   "fraction_of_peak": n * flops_per_point() / (med * 1e-3) / PEAK_FP32_MFMA, "torch_ms_median": tmed, "torch_ms_min": tbest,
                   "speedup_vs_torch": tmed / med, "max_abs_diff_vs_torch": d}
    if a.grad:
        def torch_grad(p, shape_of, zz):
            q = p.clone().requires_grad_(True)
            return torch.autograd.grad(ref(q, shape_of, zz).sum(), q)[0]
        gmed, gbest = timed(lambda: dec.decode_grad(pts, z), a.reps, a.warmup)
        tgmed, tgbest = timed(lambda: torch_grad(pts, None, z), max(3, a.reps // 4), 1)
        gd = float((dec.decode_grad(pts, z)[1] - torch_grad(pts, None, z)).abs().max())
        res["grid"].update(grad_ms_median=gmed, grad_ms_min=gbest, grad_over_decode=gmed / med, torch_autograd_ms_median=tgmed,
                           torch_autograd_ms_min=tgbest, grad_speedup_vs_torch_autograd=tgmed / gmed, grad_max_abs_diff_vs_torch=gd)
    # atoms workload
    M = 256
    counts = 9 + synth.hash_u24(M, 631, 5) % 26
    batch = torch.from_numpy(np.repeat(np.arange(M), counts)).cuda()
    n = int(counts.sum())
    pos = torch.from_numpy((synth.hash_normal((n, 3), 632, 5) * np.float32(1.5)).astype(np.float32)).cuda()
    zm = torch.from_numpy((synth.hash_normal((M, Z, 3), 633, 5) * np.float32(0.5)).astype(np.float32)).cuda()
    med, best = timed(lambda: dec.decode_atoms(pos, batch, zm), a.reps, a.warmup)
    tmed, tbest = timed(lambda: ref(pos, batch, zm), a.reps, a.warmup)
    d = float((dec.decode_atoms(pos, batch, zm) - ref(pos, batch, zm)).abs().max())
    res["atoms"] = {"molecules": M, "points": n, "ms_median": med, "ms_min": best, "points_per_s": n / med * 1e3,
                    "fraction_of_peak": n * flops_per_point() / (med * 1e-3) / PEAK_FP32_MFMA, "torch_ms_median": tmed, "torch_ms_min": tbest,
                    "speedup_vs_torch": tmed / med, "max_abs_diff_vs_torch": d}
    if a.grad:
        gmed, gbest = timed(lambda: dec.decode_atoms_grad(pos, batch, zm), a.reps, a.warmup)
        umed, ubest = timed(lambda: dec.guide_atoms(pos, batch, zm, 1.0), a.reps, a.warmup)
        tgmed, tgbest = timed(lambda: torch_grad(pos, batch, zm), a.reps, a.warmup)
        res["atoms"].update(grad_ms_median=gmed, grad_ms_min=gbest, grad_over_decode=gmed / med, guide_ms_median=umed, guide_ms_min=ubest,
                            torch_autograd_ms_median=tgmed, torch_autograd_ms_min=tgbest, grad_speedup_vs_torch_autograd=tgmed / gmed)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
