#!/usr/bin/env python3
"""Generate tests/golden/mol_sim.npz and tests/golden/mol_sim_gaussint.json from the reference itself.

Runs only where the reference is checked out (REF below); nothing here is imported by the product, the tests or the bench.
It executes the reference's own ``utils/evaluation/shaep_utils.py`` (``VAB_2nd_order``, ``shape_tanimoto``, ``get_ROCS``) and
``utils/espsim/electrostatics.py`` + ``helpers.py`` (``GaussInt``, ``SimilarityMetric``) as shipped, with ``rdkit`` stood in by
empty modules: none of these functions touches it.  Needs numpy, torch and scipy (``scipy.spatial.distance.cdist`` makes the
distance matrices that ``GaussInt`` takes, as ``GetIntegralsViaGaussians`` does).

  * mol_sim_gaussint.json   the two coefficient tables of GaussInt as data, read from its local variables while it runs
  * mol_sim.npz             40 pairs of molecules of 1..64 atoms, float64: random walks with 1.1-1.6 A steps, some with
                            coincident atoms, identical molecules, far-apart molecules, charges of mixed sign, one pair with
                            zero prefactors and one with zero charges (the zero denominators).  Per pair: the three
                            VAB_2nd_order integrals and shape_tanimoto with float64 per-atom tensors; get_ROCS with its
                            defaults (float32 coefficients); the three GaussInt integrals and SimilarityMetric for both
                            metrics (NaN where it raises).

The far-apart pairs have at most 25 atoms per molecule and come in two kinds.  torch.cdist switches to a matrix-product
formulation above 25 rows whose error is absolute in |x|^2, and even its direct form squares a rounded square root, so the
reference's r^2 carries up to 1.5 ulp, which the exponent multiplies by B r^2.  One kind sits 15 A apart (B r^2 of about 90,
S_ab of about 1e-40: the amplification stays below the summation bound of a pair of that size); the other 70 A apart, where
every term underflows to exactly 0 on both sides.

    python tests/golden/make_golden_mol_sim.py
"""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np
import scipy.spatial
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


class _Empty(types.ModuleType):
    """An empty stand-in module: any name imported from it is None."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for name in ("rdkit", "rdkit.Chem", "rdkit.Chem.AllChem", "rdkit.Chem.rdMolAlign", "rdkit.Chem.rdMolDescriptors", "rdkit.Chem.rdForceFieldHelpers",
                 "rdkit.Chem.rdmolfiles", "rdkit.Geometry"):
        sys.modules[name] = _Empty(name)
    for name in ("utils", "utils.espsim"):
        pkg = types.ModuleType(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    shaep = _load("ref_shaep_utils", os.path.join(REF, "utils", "evaluation", "shaep_utils.py"))
    helpers = _load("utils.espsim.helpers", os.path.join(REF, "utils", "espsim", "helpers.py"))
    esp = _load("utils.espsim.electrostatics", os.path.join(REF, "utils", "espsim", "electrostatics.py"))
    return shaep, esp, helpers


def gaussint_tables(esp):
    """The local tables a_flat and b_flat of GaussInt, taken from its frame when it returns."""
    seen = {}

    def tracer(frame, event, arg):
        if frame.f_code.co_name != "GaussInt":
            return None

        def local(frame, event, arg):
            if event == "return":
                seen["a"], seen["b"] = frame.f_locals["a_flat"].tolist(), frame.f_locals["b_flat"].tolist()
            return local
        return local

    sys.settrace(tracer)
    try:
        esp.GaussInt(np.zeros((1, 1)), np.ones(1), np.ones(1))
    finally:
        sys.settrace(None)
    return seen


def walk(rng, n):
    u = rng.standard_normal((n, 3))
    u *= (rng.uniform(1.1, 1.6, n) / np.linalg.norm(u, axis=1))[:, None]
    p = np.cumsum(u, 0)
    return p - p.mean(0) + rng.uniform(-1, 1, 3)


def main():
    shaep, esp, helpers = load_reference()
    tables = gaussint_tables(esp)
    with open(os.path.join(HERE, "mol_sim_gaussint.json"), "w") as f:
        json.dump(tables, f)
    rng = np.random.default_rng(20261021)
    sizes = [(1, 1), (1, 2), (2, 2), (3, 2), (3, 3), (4, 7), (5, 5), (6, 9), (8, 8), (10, 4), (12, 15), (14, 14), (16, 11), (18, 25), (20, 23), (21, 21),
             (22, 30), (24, 24), (25, 19), (26, 26), (27, 33), (28, 12), (30, 30), (31, 40), (32, 32), (33, 64), (35, 20), (36, 36), (38, 51), (40, 40),
             (42, 17), (45, 45), (48, 60), (50, 50), (55, 63), (60, 60), (63, 1), (64, 64), (64, 37), (20, 25)]
    A, B, kinds = [], [], []
    par = {k: [] for k in ("alpha_a", "p_a", "alpha_b", "p_b", "w_a", "w_b")}
    for m, (na, nb) in enumerate(sizes):
        a, b, kind = walk(rng, na), walk(rng, nb), "walk"
        if m in (2, 6, 24, 37):                          # identical molecules
            b, kind = a.copy(), "identical"
        if m in (7, 22) and na >= 3 and nb >= 3:         # coincident atoms, inside a molecule and across the pair
            a[2], b[1], kind = a[0], a[0], "coincident"
        if m in (12, 18):                                # far apart, S_ab still a normal number
            b, kind = b + np.array([15.0, 0.0, 0.0]) + (a.mean(0) - b.mean(0)), "far"
        if m in (15, 39):                                # far apart, every term of S_ab underflows to 0
            b, kind = b + np.array([0.0, 70.0, 0.0]) + (a.mean(0) - b.mean(0)), "underflow"
        al_a, al_b = rng.uniform(0.5, 1.2, na), rng.uniform(0.5, 1.2, nb)
        p_a, p_b = rng.uniform(0.5, 1.0, na), rng.uniform(0.5, 1.0, nb)
        w_a, w_b = 0.4 * rng.standard_normal(na), 0.4 * rng.standard_normal(nb)
        if m == 9:
            p_a, p_b, kind = np.zeros(na), np.zeros(nb), "zero-prefactors"
        if m == 10:
            w_b, kind = np.zeros(nb), "zero-charges"
        A.append(a); B.append(b); kinds.append(kind)
        for k, v in zip(par, (al_a, p_a, al_b, p_b, w_a, w_b)):
            par[k].append(v)
    out = {"off_a": np.concatenate([[0], np.cumsum([len(a) for a in A])]).astype(np.int64),
           "off_b": np.concatenate([[0], np.cumsum([len(b) for b in B])]).astype(np.int64),
           "pos_a": np.concatenate(A), "pos_b": np.concatenate(B), "kind": np.array(kinds)}
    out.update({k: np.concatenate(v) for k, v in par.items()})
    res = {k: [] for k in ("vaa", "vbb", "vab", "tanimoto", "rocs", "esp_aa", "esp_bb", "esp_ab", "esp_carbo", "esp_tanimoto")}
    t = lambda x: torch.as_tensor(x, dtype=torch.float64)  # noqa: E731
    for m, (a, b) in enumerate(zip(A, B)):
        al_a, p_a, al_b, p_b, w_a, w_b = (par[k][m] for k in par)
        res["vaa"].append(shaep.VAB_2nd_order(t(a), t(a), t(al_a), t(al_a), t(p_a), t(p_a)).item())
        res["vbb"].append(shaep.VAB_2nd_order(t(b), t(b), t(al_b), t(al_b), t(p_b), t(p_b)).item())
        res["vab"].append(shaep.VAB_2nd_order(t(a), t(b), t(al_a), t(al_b), t(p_a), t(p_b)).item())
        res["tanimoto"].append(shaep.shape_tanimoto(t(a), t(b), t(al_a), t(al_b), t(p_a), t(p_b)).item())
        res["rocs"].append(shaep.get_ROCS(t(a), t(b)).item())
        d = scipy.spatial.distance.cdist
        iaa, ibb, iab = esp.GaussInt(d(a, a), w_a, w_a), esp.GaussInt(d(b, b), w_b, w_b), esp.GaussInt(d(a, b), w_a, w_b)
        res["esp_aa"].append(iaa); res["esp_bb"].append(ibb); res["esp_ab"].append(iab)
        for metric in ("carbo", "tanimoto"):
            try:
                assert esp.GetIntegralsViaGaussians(a, b, w_a, w_b, metric) == helpers.SimilarityMetric(iaa, ibb, iab, metric)
                res[f"esp_{metric}"].append(helpers.SimilarityMetric(iaa, ibb, iab, metric))
            except ValueError:
                res[f"esp_{metric}"].append(np.nan)
    out.update({k: np.array(v, np.float64) for k, v in res.items()})
    np.savez_compressed(os.path.join(HERE, "mol_sim.npz"), **out)
    for m, k in enumerate(kinds):
        if k != "walk":
            print(m, sizes[m], k, "vab", res["vab"][m], "tanimoto", res["tanimoto"][m], "rocs", res["rocs"][m], "carbo", res["esp_carbo"][m])
    print("wrote", os.path.getsize(os.path.join(HERE, "mol_sim.npz")), "bytes;", len(sizes), "pairs;", len(tables["a"]), "GaussInt terms")


if __name__ == "__main__":
    main()
