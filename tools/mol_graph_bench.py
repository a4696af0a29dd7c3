#!/usr/bin/env python
"""Bond graphs (shapemol_amd.mol_graph): wall time of bond_graph on one frame of 1000 molecules and of bond_graph_trajectory
on 1000 frames of 256 molecules -- molecule sizes drawn from the MOSES prior of shapemol_amd.synth, positions and classes
already on the device -- beside evaluate_geometry / evaluate_trajectory on the same inputs and the numpy oracle on the host
(a few molecules).  The wall time is a host clock around the call, which ends in a stream synchronise; it includes the host
plan, the output allocation and the copy of the bond list.  No figure is a gate.

    python tools/mol_graph_bench.py [--reps 7] [--out profiles/mol_graph/bench.json]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def frames_of(n_mols, n_frames, seed=2024):
    """Random-walk molecules (1.1-1.6 A steps) of MOSES-prior sizes; frame f is the base moved by noise that shrinks to 0 at the
    last frame, like a chain settling.  Returns sizes, pos (F, N, 3) float32, classes (F, N) int64 of add_aromatic."""
    from shapemol_amd import synth
    rng = np.random.default_rng(seed)
    nums, p = synth.moses_atom_prior()
    sizes = rng.choice(nums, size=n_mols, p=p)
    base = []
    for n in sizes:
        u = rng.standard_normal((n, 3))
        u *= (rng.uniform(1.1, 1.6, n) / np.linalg.norm(u, axis=1))[:, None]
        base.append(np.cumsum(u, 0))
    base = np.concatenate(base)
    scale = np.linspace(1.0, 0.0, n_frames)[:, None, None] if n_frames > 1 else np.zeros((1, 1, 1))
    pos = (base[None] + scale * rng.standard_normal((n_frames,) + base.shape)).astype(np.float32)
    cls = rng.choice(15, (n_frames, len(base)), p=np.r_[0.1, 0.5, np.full(13, 0.4 / 13)])
    return sizes, pos, cls


def timed(fn, reps):
    import torch
    fn()                                              # warm-up: code objects load, the contexts and workspaces are made
    fn()
    wall = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0)
    return [float(w) for w in wall]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--oracle-mols", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import mol_eval_oracle as E
    import mol_graph_oracle as O
    from shapemol_amd import StabilityRule, _lib, bond_graph, bond_graph_trajectory, evaluate_geometry, evaluate_trajectory
    from shapemol_amd.mol_surface import VOCAB_ELEMENTS
    if not torch.cuda.is_available():
        raise SystemExit("mol_graph_bench: no HIP device (there is no CPU path to time)")
    rule, orule = StabilityRule.from_json(E.RULE_JSON), E.Rule.load()
    bl = np.linspace(0.8, 2.4, 41)
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, library_sha256=hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest(), cases={})
    for name, mols, frames in (("one_frame_1000_mols", 1000, 1), ("trajectory_1000_frames_256_mols", 256, 1000)):
        sizes, pos, cls = frames_of(mols, frames)
        batch = np.repeat(np.arange(mols), sizes)
        d_pos, d_cls, d_batch = torch.from_numpy(pos).cuda(), torch.from_numpy(cls).cuda(), torch.from_numpy(batch).cuda()
        if frames == 1:
            graph = lambda: bond_graph(d_pos[0], d_cls[0], d_batch, rule, bond_bins=bl)                  # noqa: E731
            geo = lambda: evaluate_geometry(d_pos[0], d_cls[0], d_batch, rule)                           # noqa: E731
        else:
            graph = lambda: bond_graph_trajectory(d_pos, d_cls, d_batch, rule, bond_bins=bl)             # noqa: E731
            geo = lambda: evaluate_trajectory(d_pos, d_cls, d_batch, rule)                               # noqa: E731
        wg, we = timed(graph, a.reps), timed(geo, a.reps)
        r = graph()
        k = min(a.oracle_mols, mols)
        off = np.concatenate([[0], np.cumsum(sizes)])
        t0 = time.perf_counter()
        exp = O.graph(pos[-1:, :off[k]], cls[-1:, :off[k]], off[:k + 1], orule, orule.slots(VOCAB_ELEMENTS["add_aromatic"]), bl=bl)
        cpu = time.perf_counter() - t0
        nb = int(exp["bond_offsets"][-1])
        f = -1 if frames > 1 else slice(None)
        equal = (np.array_equal(r.n_bonds[f][..., :k].cpu().numpy().reshape(-1), exp["n_bonds"][0]) and
                 np.array_equal(r.frag[f][..., :off[k]].cpu().numpy().reshape(-1), exp["frag"][0]) and
                 np.array_equal(r.ring[f][..., :off[k]].cpu().numpy().reshape(-1), exp["ring"][0]))
        mg, me = float(np.median(wg)), float(np.median(we))
        res["cases"][name] = dict(mols=mols, frames=frames, atoms_per_frame=int(off[-1]), bonds=int(len(r.bond_list)), graph_wall_s=wg, graph_wall_s_median=mg,
                                  geometry_wall_s=we, geometry_wall_s_median=me, graph_over_geometry=mg / me,
                                  molecules_per_s=mols * frames / mg,
                                  numpy_oracle=dict(machine="the GPU host's CPU", molecules=k, bonds=nb, seconds=cpu, molecules_per_s=k / cpu,
                                                    device_over_oracle_molecules_per_s=(mols * frames / mg) / (k / cpu)),
                                  device_equals_oracle_on_those_molecules=bool(equal), complete_fraction_last_frame=r.validity(frame=None if frames == 1 else frames - 1)["complete"])
        print(json.dumps({name: res["cases"][name]}))
        if not equal:
            raise SystemExit("mol_graph_bench: the device differs from the oracle")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
