#!/usr/bin/env python
"""Geometry scores (shapemol_amd.evaluation): frames per second and atom pairs per second of evaluate_trajectory over every
recorded frame of a chain -- B molecules of 20..35 atoms x F frames, positions and classes already on the device, as they are
when a chain ends -- beside the vectorised numpy oracle of the same rule on the same machine's host (a few frames).  The wall
time is a host clock around the call, which ends in a stream synchronise; it includes the host plan and the output allocation.
No figure is a gate.

    python tools/mol_eval_bench.py [--mols 256] [--frames 1000] [--reps 7] [--out profiles/mol_eval/bench.json]
    python tools/mol_eval_bench.py --reference-loops DIR [--out profiles/mol_eval/reference_loops.json]
        host only: the time of the reference's own check_stability + pair_distance_from_pos_v loops (DIR = its checkout) on a few
        of the same molecules, on whatever CPU runs this -- a different machine from the GPU host, and labelled so.
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


def chain_frames(n_mols, n_frames, seed=2024):
    """Random-walk molecules of 20..35 atoms (1.1-1.6 A steps); frame f is the base moved by noise that shrinks to 0 at the last
    frame, like a chain settling.  Returns sizes, pos (F, N, 3) float32, classes (F, N) int64 of add_aromatic."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(20, 36, n_mols)
    base = []
    for n in sizes:
        u = rng.standard_normal((n, 3))
        u *= (rng.uniform(1.1, 1.6, n) / np.linalg.norm(u, axis=1))[:, None]
        base.append(np.cumsum(u, 0))
    base = np.concatenate(base)
    scale = np.linspace(1.0, 0.0, n_frames)[:, None, None]
    pos = (base[None] + scale * rng.standard_normal((n_frames,) + base.shape)).astype(np.float32)
    cls = rng.choice(15, (n_frames, len(base)), p=np.r_[0.1, 0.5, np.full(13, 0.4 / 13)])
    return sizes, pos, cls


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def reference_loops(ref, out, n_mols=8):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_mol_eval as G
    from shapemol_amd.mol_surface import VOCAB_ELEMENTS
    G.REF = ref
    analyze, ebl = G.load_reference()
    sizes, pos, cls = chain_frames(n_mols, 1)
    off = np.concatenate([[0], np.cumsum(sizes)])
    z = np.asarray(VOCAB_ELEMENTS["add_aromatic"])[cls[0]]
    t0 = time.perf_counter()
    for b in range(n_mols):
        p, e = pos[0, off[b]:off[b + 1]].astype(np.float64), z[off[b]:off[b + 1]].tolist()
        analyze.check_stability(p, e)
        ebl.pair_distance_from_pos_v(p, e)
    dt = time.perf_counter() - t0
    pairs = int(sum(n * (n - 1) // 2 for n in sizes))
    res = dict(what="the reference's own Python loops (analyze.check_stability + eval_bond_length.pair_distance_from_pos_v), one frame",
               machine="the CPU-only development machine, NOT the GPU host", cpu=cpu_name(), molecules=n_mols, atoms=int(off[-1]), pairs=pairs,
               seconds=dt, s_per_molecule=dt / n_mols, pairs_per_s=pairs / dt)
    print(json.dumps(res))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(res, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mols", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--oracle-frames", type=int, default=2)
    ap.add_argument("--reference-loops", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reference_loops:
        return reference_loops(a.reference_loops, a.out)
    import torch
    import mol_eval_oracle as O
    from shapemol_amd import StabilityRule, _lib, evaluate_trajectory
    from shapemol_amd.mol_surface import VOCAB_ELEMENTS
    if not torch.cuda.is_available():
        raise SystemExit("mol_eval_bench: no HIP device (there is no CPU path to time)")
    rule, orule = StabilityRule.from_json(O.RULE_JSON), O.Rule.load()
    sizes, pos, cls = chain_frames(a.mols, a.frames)
    batch = np.repeat(np.arange(a.mols), sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    pairs = int(sum(n * (n - 1) // 2 for n in sizes)) * a.frames
    d_pos, d_cls, d_batch = torch.from_numpy(pos).cuda(), torch.from_numpy(cls).cuda(), torch.from_numpy(batch).cuda()
    rep = evaluate_trajectory(d_pos, d_cls, d_batch, rule)                    # warm-up: code objects load, the context is made
    wall = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = evaluate_trajectory(d_pos, d_cls, d_batch, rule)
        wall.append(time.perf_counter() - t0)
    k = a.oracle_frames
    t0 = time.perf_counter()
    exp = O.evaluate(pos[-k:], cls[-k:], off, orule, orule.slots(VOCAB_ELEMENTS["add_aromatic"]))
    cpu = (time.perf_counter() - t0) / k
    equal = all(np.array_equal(getattr(rep, key)[-k:].cpu().numpy(), exp[key]) for key in
                ("nr_bonds", "n_stable_atoms", "mol_stable", "hist_cc", "hist_all", "class_counts"))
    med = float(np.median(wall))
    last = rep.validity(frame=a.frames - 1)
    res = dict(mols=a.mols, frames=a.frames, atoms_per_frame=int(off[-1]), pairs=pairs, reps=a.reps, device=torch.cuda.get_device_name(0),
               library_sha256=hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(),
               wall_s=[float(w) for w in wall], wall_s_median=med, frames_per_s=a.frames / med, pairs_per_s=pairs / med,
               numpy_oracle=dict(machine="the GPU host's CPU", cpu=cpu_name(), frames=k, s_per_frame=cpu, frames_per_s=1.0 / cpu, pairs_per_s=pairs / a.frames / cpu),
               device_equals_oracle_on_those_frames=bool(equal), validity_last_frame=last,
               note="wall: host clock around evaluate_trajectory (host plan, output allocation, class-range reduction, upload of the tables, the launches, synchronise); "
                    "inputs already on the device.  The numpy oracle is context, not a gate.")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    if not equal:
        raise SystemExit("mol_eval_bench: the device differs from the oracle")


if __name__ == "__main__":
    main()
