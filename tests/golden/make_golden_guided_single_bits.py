#!/usr/bin/env python3
"""The project's OWN outputs of the tuple forms of shape guidance, to the bit, recorded on an MI355X at the last commit that
still had separate single-cloud / single-mesh kernels (pc_guidance_kernel, mesh_classify_kernel, mesh_pull_kernel).

    python tests/golden/make_golden_guided_single_bits.py          (needs the built library and a GPU)

Since then the tuple forms ``use_pointcloud_data=(cloud, kdtree, radius)`` and ``use_mesh_data=(mesh, cloud, kdtree)`` run as a
set of one group through the group kernels; tests/test_gpu_guided_multi.py::test_one_group_is_the_single_cloud_chain and
tests/test_gpu_mesh_multi.py::test_one_group_is_the_single_mesh_chain demand ``torch.equal`` against this file, so that the
merged path is compared with the kernels it replaced and not only with itself.  Re-running this script on a later commit
records that commit's outputs: do so only for a deliberate change of the guidance arithmetic.

Inputs: chain_guided_b4_s20.npz, and chain_mesh_guided_b4_s20.npz with mesh_fixture.npz (synthetic weights seed 7, hash noise).
Runs: exact mode, use_graph=True, once with the fixture's fed draws and once with device Philox draws on seed 9.
Writes guided_single_bits.npz: ``{cloud,mesh}_{fed,philox}_{pos,v,pos_cond_traj}`` (pos_cond_traj stacked over the 20 steps).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from util import T, golden, hash_noise, hip_model, synth  # noqa: E402

DEV = "cuda:0"
SEED = 9


def runs(name, **guidance):
    m = hip_model()
    m.set_option("edge_bf16", 2)
    m.set_option("node_f16", 0)
    c = golden(name)
    B, S = int(c["B"]), int(c["S"])
    bb = synth.synthetic_batch(B, seed=int(c["seed"]))
    eps, u = hash_noise(len(bb["batch"]), S, int(c["seed"]))
    out = {}
    for tag, extra in (("fed", dict(guide_draws=T(c["draws"], DEV))), ("philox", dict(seed=SEED))):
        r = m.sample_diffusion(T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1),
                               num_steps=S, center_pos_mode="none", noise=(T(eps, DEV), T(u, DEV)), use_graph=True,
                               grad_step=int(c["grad_step"]), **guidance, **extra)
        out[tag + "_pos"] = r["pos"].cpu().numpy()
        out[tag + "_v"] = r["v"].cpu().numpy().astype(np.int8)
        out[tag + "_pos_cond_traj"] = torch.stack(r["pos_cond_traj"]).cpu().numpy()
    return out


def main():
    c = golden("chain_guided_b4_s20.npz")
    mf = golden("mesh_fixture.npz")
    data = {"cloud_" + k: v for k, v in runs("chain_guided_b4_s20.npz", use_pointcloud_data=(c["cloud"], None, float(c["radius"]))).items()}
    data.update({"mesh_" + k: v for k, v in runs("chain_mesh_guided_b4_s20.npz",
                                                 use_mesh_data=((mf["verts"], mf["faces"]), mf["cloud"], None)).items()})
    out = os.environ.get("GOLDEN_OUT", os.path.join(HERE, "guided_single_bits.npz"))
    np.savez_compressed(out, seed=SEED, **data)
    for k, v in data.items():
        print(k, v.shape, v.dtype)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
