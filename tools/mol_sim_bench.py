#!/usr/bin/env python
"""Similarity to the shape condition (shapemol_amd.similarity): samples per second of align_shapes and of get_rocs over N
samples of 20..30 atoms against one condition molecule, positions on the host as the sampling driver returns them, beside
the numpy oracle of the same overlay rule on the same machine's host (a few samples).  ShaEP is not available, so there is no
figure for the reference's own path.  The wall time is a host clock around the call, which ends in a stream synchronise; it
includes the host plan, the uploads and the output allocation.  No figure is a gate.

    python tools/mol_sim_bench.py [--samples 1000] [--reps 7] [--oracle-samples 8] [--out profiles/mol_sim/bench.json]
"""
import argparse
import hashlib
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--oracle-samples", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import mol_sim_oracle as O
    from shapemol_amd import _lib, align_shapes, get_rocs
    if not torch.cuda.is_available():
        raise SystemExit("mol_sim_bench: no HIP device (there is no CPU path to time)")
    rng = np.random.default_rng(2026)
    cond = O.walk(rng, 26)
    samples = [O.walk(rng, int(n)) + rng.uniform(-2, 2, 3) for n in rng.integers(20, 31, a.samples)]
    terms = int(sum(len(s) * len(cond) for s in samples))

    def timed(fn):
        fn()                                                  # warm-up: code objects load, the context is made, workspaces grow
        wall = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            wall.append(time.perf_counter() - t0)
        return out, wall

    r, wall_align = timed(lambda: align_shapes(samples, cond))
    _, wall_score = timed(lambda: get_rocs(samples, cond))
    score, iters = r.tanimoto.cpu().numpy(), r.iterations.cpu().numpy()
    k = min(a.oracle_samples, a.samples)
    pb = O.rocs_parameters(len(cond))
    t0 = time.perf_counter()
    exp = [O.align(s, cond, *O.rocs_parameters(len(s)), *pb) for s in samples[:k]]
    cpu = (time.perf_counter() - t0) / k
    diff = float(max(abs(e["tanimoto"] - score[i]) for i, e in enumerate(exp)))
    med_a, med_s = float(np.median(wall_align)), float(np.median(wall_score))
    res = dict(samples=a.samples, condition_atoms=len(cond), atom_pairs=terms, reps=a.reps, device=torch.cuda.get_device_name(0),
               library_sha256=hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(),
               align=dict(wall_s=[float(w) for w in wall_align], wall_s_median=med_a, samples_per_s=a.samples / med_a,
                          converged=int(r.converged.sum()), iterations_mean=float(iters.mean()), iterations_max=int(iters.max()),
                          tanimoto_mean=float(score.mean()), tanimoto_max=float(score.max())),
               fixed_pose=dict(wall_s=[float(w) for w in wall_score], wall_s_median=med_s, samples_per_s=a.samples / med_s),
               numpy_oracle=dict(machine="the GPU host's CPU", cpu=cpu_name(), samples=k, s_per_sample=cpu, samples_per_s=1.0 / cpu,
                                 largest_difference_to_device=diff),
               note="wall: host clock around align_shapes / get_rocs (host plan, upload of positions and tables, output allocation, the launches, "
                    "synchronise); positions start on the host.  The numpy oracle is context, not a gate; ShaEP was not available.")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
