"""Shared by the tests of mesh shape guidance with one mesh per group of molecules: the fixtures of
tests/golden/make_golden_mesh_multi.py as the list form of ``use_mesh_data``."""
import numpy as np

from util import golden, synth

FN = "mesh_guidance_multi_fn.npz"
CHAINS = ("chain_mesh_guided_multi_b6_s20.npz", "chain_mesh_guided_multi_b6_s20_gap.npz")


def meshes():
    """[(verts, faces, cloud)] of the three groups (stored once, in the function fixture)."""
    f = golden(FN)
    return [(f["verts"][f["vert_off"][g]:f["vert_off"][g + 1]], f["faces"][f["face_off"][g]:f["face_off"][g + 1]],
             f["clouds"][f["cloud_off"][g]:f["cloud_off"][g + 1]]) for g in range(len(f["group_mols"]))]


def mesh_groups(c):
    """The list form of use_mesh_data of a fixture: [((verts, faces) or None, cloud, None, n_mols)]."""
    ms = meshes()
    return [(((ms[g][0], ms[g][1]), ms[g][2], None, int(n)) if c["has_mesh"][g] else (None, None, None, int(n)))
            for g, n in enumerate(c["group_mols"])]


def atom_ranges(counts, group_mols):
    """(mol_off, atom_off) of the groups, from the molecules' atom counts."""
    mol_off = np.concatenate([[0], np.cumsum(group_mols)])
    return mol_off, np.concatenate([[0], np.cumsum(counts)])[mol_off]


def chain_batch(c):
    return synth.synthetic_batch(int(c["B"]), seed=int(c["seed"]))
