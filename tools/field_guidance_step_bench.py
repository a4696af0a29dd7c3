#!/usr/bin/env python3
"""Times one reverse step at B = 256 (200-step chains, device noise, graph replay, no trajectories; best of 3, three rounds):
unguided, field-guided at every step, field-guided with grad_step = 900 (99 of the 200 steps pass the gate) and cloud-guided
(512 points).  Prints one JSON line of ms per step.

    python tools/field_guidance_step_bench.py
"""
import json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import shape_decoder_f64 as D
from util import T, hip_model, synth
from shapemol_amd.shape_autoencoder import DecoderInner
DEV = "cuda:0"
m = hip_model()
dec = DecoderInner(3, 32, 128, 4, "signeddist"); dec.load_state_dict(D.state_dict(4, 32), strict=True); dec = dec.to(DEV)
B, S = 256, 200
bb = synth.synthetic_batch(B, seed=2021)
args = (T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1))
cloud = (synth.hash_normal((512, 3), 71, 3) * 2.0).astype(np.float64)
modes = {"unguided": {}, "field": dict(use_grad=True, shape_AE=dec, grad_lr=1.0, grad_step=0),
         "field_gate_closed": dict(use_grad=True, shape_AE=dec, grad_lr=1.0, grad_step=900),
         "cloud": dict(use_pointcloud_data=(cloud, None, 0.5), grad_step=0)}
res = {"B": B, "atoms": int(len(bb["batch"])), "steps": S}
def run(kw):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    m.sample_diffusion(*args, num_steps=S, center_pos_mode="none", seed=1, return_traj=False, **kw)
    torch.cuda.synchronize(); return (time.perf_counter() - t0) * 1e3 / S
for rep in range(3):
    for name, kw in modes.items():
        run(kw)                       # warm: captures this kind's graph
        res.setdefault(name, []).append(min(run(kw) for _ in range(3)))
print(json.dumps(res))
