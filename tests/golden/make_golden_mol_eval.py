#!/usr/bin/env python3
"""Generate tests/golden/mol_eval_rule.json and tests/golden/mol_eval.npz from the reference itself.

Runs only where the reference is checked out (REF below); nothing here is imported by the product, the tests or the bench.
It executes the reference's own ``utils/evaluation/analyze.py`` and ``utils/evaluation/eval_bond_length.py`` as shipped.
``eval_bond_length.py`` imports ``utils.eval_bond_length_config`` and ``utils.data``: the first is aliased to the
``utils/evaluation/eval_bond_length_config.py`` that the reference ships, the second (bond types of RDKit molecules, not used
by the pair-distance functions) is an empty stand-in.

  * mol_eval_rule.json   the tables of analyze.py as data: elements, bonds1..3 (pm), margins, allowed_bonds
  * mol_eval.npz         40 small molecules (1..40 atoms, float32 positions, classes of the three vocabularies): random-walk
                         chains and rings with 1.1-1.6 A steps, a few perturbed, with coincident atoms and with NaN
                         coordinates; per molecule check_stability(..., return_nr_bonds=True) for hs False and True; for the
                         set the two pair-length profiles, their Jensen-Shannon distances and the empirical distributions.

    python tests/golden/make_golden_mol_eval.py
"""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)
from shapemol_amd.mol_surface import VOCAB_ELEMENTS  # noqa: E402

MODES = ("basic", "add_aromatic", "full")


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    ev = os.path.join(REF, "utils", "evaluation")
    utils = types.ModuleType("utils")
    utils.__path__ = []
    sys.modules["utils"] = utils
    utils.data = sys.modules["utils.data"] = types.ModuleType("utils.data")
    utils.eval_bond_length_config = _load("utils.eval_bond_length_config", os.path.join(ev, "eval_bond_length_config.py"))
    return _load("ref_analyze", os.path.join(ev, "analyze.py")), _load("ref_eval_bond_length", os.path.join(ev, "eval_bond_length.py"))


def dump_rule(analyze, path):
    z = sorted(analyze.atom_decoder)
    sym = [analyze.atom_decoder[k] for k in z]
    table = lambda t: [[t[a][b] for b in sym] for a in sym]  # noqa: E731
    rule = {"elements": z, "bonds1": table(analyze.bonds1), "bonds2": table(analyze.bonds2), "bonds3": table(analyze.bonds3),
            "margins": [analyze.margin1, analyze.margin2, analyze.margin3], "allowed_bonds": [analyze.allowed_bonds[s] for s in sym]}
    with open(path, "w") as f:
        json.dump(rule, f)
    return rule


def walk(rng, n, ring, zigzag):
    """n atoms, consecutive ones 1.1 .. 1.6 A apart: a zigzag chain (bond angle about 110 degrees, so that only neighbours
    bond), a persistent random walk, or a ring (closed: the last atom is a step from the first)."""
    if ring and n >= 3:
        r = rng.uniform(1.1, 1.6) / (2 * np.sin(np.pi / n))
        a = 2 * np.pi * np.arange(n) / n
        pos = np.stack([r * np.cos(a), r * np.sin(a), 0.15 * rng.standard_normal(n)], 1)
        return pos + rng.uniform(-3, 3, 3)
    pos = [rng.uniform(-3, 3, 3)]
    d = rng.standard_normal(3)
    d /= np.linalg.norm(d)
    side = np.cross(d, rng.standard_normal(3))
    side /= np.linalg.norm(side)
    for k in range(1, n):
        step = rng.uniform(1.1, 1.6)
        if zigzag:
            u = 0.82 * d + 0.57 * side * (1 if k % 2 else -1)
        else:
            u = d + 0.9 * rng.standard_normal(3)
            d = u / np.linalg.norm(u)
        pos.append(pos[-1] + step * u / np.linalg.norm(u))
    return np.array(pos)


def classes_of(rng, n, mode, heavy):
    """Classes of the vocabulary: mostly carbon, nitrogen and oxygen where `heavy`, else anything."""
    z = np.array(VOCAB_ELEMENTS[mode])
    if heavy:
        p = np.where(z == 6, 6.0, np.where((z == 7) | (z == 8), 1.0, 0.05))
        return rng.choice(len(z), n, p=p / p.sum())
    return rng.integers(0, len(z), n)


def main():
    analyze, ebl = load_reference()
    dump_rule(analyze, os.path.join(HERE, "mol_eval_rule.json"))
    rng = np.random.default_rng(20261020)
    sizes = [1, 1, 2, 2, 3, 3, 4, 5, 6, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 28, 30, 31, 32, 33, 35, 36, 38, 40, 40]
    pos, cls, mode, kind = [], [], [], []
    for m, n in enumerate(sizes):
        md = MODES[m % 3]
        ring, zig = m % 5 == 2, m % 5 in (0, 1)
        p = walk(rng, n, ring, zig).astype(np.float32)
        c = classes_of(rng, n, md, heavy=m % 4 != 3)
        k = "ring" if ring and n >= 3 else "zigzag" if zig else "walk"
        if m in (9, 19, 29):                      # perturbed: every atom moved by up to 0.3 A
            p = (p + rng.uniform(-0.3, 0.3, p.shape)).astype(np.float32)
            k += "+perturbed"
        if m in (12, 27) and n >= 3:              # coincident atoms: d == 0, bin 0 of the histograms
            p[2] = p[0]
            k += "+coincident"
        if m in (16, 34):                         # a NaN coordinate: order 0 and no histogram entry for that atom's pairs
            p[1, 1] = np.nan
            k += "+nan"
        pos.append(p); cls.append(c.astype(np.int64)); mode.append(m % 3); kind.append(k)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out = {"off": off, "pos": np.concatenate(pos), "classes": np.concatenate(cls), "mode": np.array(mode, np.int64), "kind": np.array(kind)}
    all_pairs = []
    for hs in (False, True):
        ms, ns, nb = [], [], []
        for p, c, md in zip(pos, cls, mode):
            z = [VOCAB_ELEMENTS[MODES[md]][i] for i in c.tolist()]
            with np.errstate(invalid="ignore"):
                r = analyze.check_stability(p.astype(np.float64), z, hs=hs, return_nr_bonds=True)
                if not hs:
                    all_pairs += ebl.pair_distance_from_pos_v(p.astype(np.float64), z)
            assert r[2] == len(p)
            ms.append(bool(r[0])); ns.append(int(r[1])); nb.append(np.asarray(r[3], np.int64))
        tag = "hs" if hs else "nohs"
        out[f"mol_stable_{tag}"], out[f"n_stable_{tag}"], out[f"nr_bonds_{tag}"] = np.array(ms), np.array(ns, np.int64), np.concatenate(nb)
    with np.errstate(invalid="ignore"):
        profile = ebl.get_pair_length_profile(all_pairs)
    metrics = ebl.eval_pair_length_profile(profile)
    cfg = sys.modules["utils.eval_bond_length_config"]
    for k in ("CC_2A", "All_12A"):
        out[f"profile_{k}"] = np.asarray(profile[k], np.float64)
        out[f"jsd_{k}"] = np.float64(metrics[f"JSD_{k}"])
        out[f"empirical_{k}"] = np.asarray(cfg.PAIR_EMPIRICAL_DISTRIBUTIONS[k], np.float64)
        out[f"bins_{k}"] = np.asarray(cfg.PAIR_EMPIRICAL_BINS[k], np.float64)
    d = np.array([x[1] for x in all_pairs])
    cc = np.array([x[0] == (6, 6) for x in all_pairs])
    stable = out["n_stable_nohs"].sum() / off[-1]
    print(f"{len(sizes)} molecules, {off[-1]} atoms, {len(all_pairs)} pairs; stable molecules {out['mol_stable_nohs'].sum()} (hs: {out['mol_stable_hs'].sum()}), "
          f"stable atoms {stable:.3f}; C-C pairs {cc.sum()}, of them >= 2 A: {(d[cc] >= 2).sum()}; pairs >= 12 A: {(d >= 12).sum()}; NaN: {np.isnan(d).sum()}")
    np.savez_compressed(os.path.join(HERE, "mol_eval.npz"), **out)
    print("wrote", os.path.getsize(os.path.join(HERE, "mol_eval.npz")), "bytes")


if __name__ == "__main__":
    main()
