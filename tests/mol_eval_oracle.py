"""Vectorised float64 numpy oracle of the geometry scores: what shapemol_amd.evaluation computes on the
device, written independently of it.  tests/test_mol_eval_cpu.py holds it to the reference's own loops (the results stored in
tests/golden/mol_eval.npz); the GPU tests hold the kernels to it.

The arithmetic is the reference's: d = sqrt((dx*dx + dy*dy) + dz*dz) in float64 (np.sum over three squares adds them in this
order), the nested strict tests of analyze.get_bond_order on 100 * d, np.searchsorted(..., side='left') for the bins."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RULE_JSON = os.path.join(HERE, "golden", "mol_eval_rule.json")
GOLDEN = os.path.join(HERE, "golden", "mol_eval.npz")
MODES = ("basic", "add_aromatic", "full")
WAVE_ATOMS, MAX_ATOMS, MAX_ELEMENTS, MAX_CLASSES, MAX_EDGES, THREADS = 64, 1024, 16, 32, 255, 256
CC_BINS, ALL_BINS = np.linspace(0, 2, 100), np.linspace(0, 12, 100)


class Rule:
    """The JSON rule as float64 arrays (the oracle's own reader)."""

    def __init__(self, d):
        self.elements = np.asarray(d["elements"], np.float64)
        self.bonds = np.stack([np.asarray(d[k], np.float64) for k in ("bonds1", "bonds2", "bonds3")])
        self.margins = np.asarray(d["margins"], np.float64)
        self.allowed = np.asarray(d["allowed_bonds"], np.float64)

    @classmethod
    def load(cls, path=RULE_JSON):
        with open(path) as f:
            return cls(json.load(f))

    def thresholds(self):
        return self.bonds + self.margins[:, None, None]

    def slots(self, atomic_numbers):
        return np.array([int(np.flatnonzero(self.elements == z)[0]) for z in atomic_numbers], np.int64)


def distances(pos):
    """(n, 3) -> (n, n) float64 pair distances; d[i, j] and d[j, i] are the same bits."""
    p = np.asarray(pos, np.float64)
    dx, dy, dz = (p[:, None, k] - p[None, :, k] for k in range(3))
    with np.errstate(invalid="ignore"):
        return np.sqrt((dx * dx + dy * dy) + dz * dz)


def bond_orders(d, slots, thr):
    """Order of every pair (0 on the diagonal): the nested strict tests on 100 * d."""
    with np.errstate(invalid="ignore"):
        p = 100 * d
        t = thr[:, slots[:, None], slots[None, :]]
        o = (p < t[0]) * (1 + (p < t[1]) * (1 + (p < t[2])))
    o = o.astype(np.int64)
    np.fill_diagonal(o, 0)
    return o


def histogram(d, edges, cut):
    """Counts (len(edges) + 1) of the distances below the cut-off; NaN enters nowhere."""
    with np.errstate(invalid="ignore"):
        d = d[d < cut]
    return np.bincount(np.searchsorted(edges, d, side="left"), minlength=len(edges) + 1).astype(np.int64)


def evaluate(pos, classes, off, rule, class_slots, hs=False, cc=(CC_BINS, 2.0), al=(ALL_BINS, 12.0)):
    """pos (F, N, 3), classes (F, N), off (B + 1) -> dict of the device outputs as numpy arrays, plus `orders`: the set of bond
    orders that occurred."""
    pos, classes = np.asarray(pos), np.asarray(classes)
    F, N = classes.shape
    B, C = len(off) - 1, len(class_slots)
    thr, class_slots = rule.thresholds(), np.asarray(class_slots)
    carbon = np.flatnonzero(rule.elements == 6.0)
    out = dict(nr_bonds=np.zeros((F, N), np.int32), n_stable_atoms=np.zeros((F, B), np.int32), mol_stable=np.zeros((F, B), bool),
               hist_cc=np.zeros((F, len(cc[0]) + 1), np.int64), hist_all=np.zeros((F, len(al[0]) + 1), np.int64),
               class_counts=np.zeros((F, C), np.int64), orders=set())
    for f in range(F):
        out["class_counts"][f] = np.bincount(classes[f], minlength=C)
        for b in range(B):
            s = slice(off[b], off[b + 1])
            slots = class_slots[classes[f, s]]
            d = distances(pos[f, s])
            o = bond_orders(d, slots, thr)
            out["orders"] |= set(np.unique(o[np.triu_indices(len(slots), 1)]).tolist())
            nb = o.sum(1)
            allowed = rule.allowed[slots]
            stable = (allowed == nb) if hs else ((allowed >= nb) & (nb > 0))
            out["nr_bonds"][f, s] = nb
            out["n_stable_atoms"][f, b] = stable.sum()
            out["mol_stable"][f, b] = stable.all()
            iu = np.triu_indices(len(slots), 1)
            du = d[iu]
            if len(carbon):
                both = (slots[iu[0]] == carbon[0]) & (slots[iu[1]] == carbon[0])
                out["hist_cc"][f] += histogram(du[both], *cc)
            out["hist_all"][f] += histogram(du, *al)
    return out


def profile(hist_cc, hist_all):
    """get_pair_length_profile: counts over their sum."""
    return {"CC_2A": np.array(hist_cc) / np.sum(hist_cc), "All_12A": np.array(hist_all) / np.sum(hist_all)}


def jsd(empirical, prof):
    from scipy.spatial import distance
    return {f"JSD_{k}": distance.jensenshannon(empirical[k], prof[k]) for k in empirical}


def load_golden():
    """The fixture file as a dict, with `vocab`: the atomic numbers of every vocabulary's classes."""
    from shapemol_amd.mol_surface import VOCAB_ELEMENTS
    g = dict(np.load(GOLDEN))
    g["vocab"] = {m: np.asarray(VOCAB_ELEMENTS[m]) for m in MODES}
    return g
