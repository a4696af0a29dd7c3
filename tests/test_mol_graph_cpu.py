"""The bond graphs without a GPU: the crafted cases of tests/mol_graph_cases.py are well-posed (no pair
within 1e-6 relative of a threshold, and the oracle finds the structure a case is named after), the oracle's per-atom order
sums equal the reference's own nr_bonds on the mol_eval fixture, the host refusals of shapemol_graph_check, the ABI names, and
the pure-Python helpers to_molblock and atom_type_jsd."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mol_eval_oracle as E  # noqa: E402
import mol_graph_cases as K  # noqa: E402
import mol_graph_oracle as O  # noqa: E402

SLOTS = np.arange(10)             # "basic": the class index is the rule's row


@pytest.fixture(scope="module")
def orule():
    return E.Rule.load()


def test_every_case_keeps_its_margin(orule):
    thr = orule.thresholds()
    cases = [(k, v[0], v[1]) for k, v in K.structures().items()] + [(f"ragged{k}", p, c) for k, (p, c) in enumerate(K.ragged_batch())]
    for name, pos, cls in cases:
        m = O.margin(pos, SLOTS[cls], thr)
        assert m > 1e-6, (name, m)
    assert min(O.margin(p, SLOTS[c], thr) for _, p, c in cases) < 0.1           # the measure is not vacuous


def test_every_case_is_the_structure_it_is_named_after(orule):
    thr = orule.thresholds()
    for name, (pos, cls, exp) in K.structures().items():
        if exp is None:
            continue
        o, d, bonds, rings, frag = O.molecule(pos, SLOTS[cls], thr)
        n_frags = len(set(frag.tolist()))
        assert (len(bonds), n_frags, len(bonds) - len(cls) + n_frags) == (exp["n_bonds"], exp["n_frags"], exp["n_cycles"]), name
        assert {O.ring_bit(r) for r in rings} == exp["rings"], name
        if "orders" in exp:
            assert [b[2] for b in bonds] == exp["orders"], name
    s = K.structures()
    o, d, bonds, rings, frag = O.molecule(s["fused66"][0], SLOTS[s["fused66"][1]], thr)
    assert rings[[b[:2] for b in bonds].index((2, 3))] == 6                     # the shared bond of the fused rings
    frag = O.molecule(s["scrambled"][0], SLOTS[s["scrambled"][1]], thr)[4]
    assert frag[:7].tolist() == [0] * 7 and frag[7:].tolist() == [7] * 3
    assert O.molecule(s["nan_atom"][0], SLOTS[s["nan_atom"][1]], thr)[4].tolist() == [0, 0, 2, 3, 3]
    o = O.molecule(s["walk40"][0], SLOTS[s["walk40"][1]], thr)[0]
    assert set(np.unique(o).tolist()) == {0, 1, 2, 3}
    sizes = [len(c) for _, c in K.ragged_batch()]
    assert sizes == [1, 9, 2, 64, 65, 30, 256, 63, 255, 2]
    g = O.graph(*(lambda p, c, b, off: (p[None], c[None], off))(*K.pack(K.ragged_batch())), orule, SLOTS)
    nb = g["n_bonds"][0]
    assert nb[1] > 0 and nb[2] == 0 and nb[3] > 0 and g["bond_offsets"][2] == g["bond_offsets"][3]       # the offsets repeat


def test_oracle_order_sums_equal_the_reference(orule):
    """On the mol_eval fixture (the reference's own check_stability results) the kept pairs add up to its nr_bonds."""
    g = E.load_golden()
    for m in range(len(g["off"]) - 1):
        s = slice(g["off"][m], g["off"][m + 1])
        slots = orule.slots(g["vocab"][E.MODES[g["mode"][m]]])
        r = O.graph(g["pos"][None, s], g["classes"][None, s], [0, s.stop - s.start], orule, slots)
        assert np.array_equal(r["nr_bonds"][0], g["nr_bonds_nohs"][s])
        sums = np.zeros(s.stop - s.start, np.int64)
        for i, j, o in r["bond_list"]:
            sums[i] += o
            sums[j] += o
        assert np.array_equal(sums, g["nr_bonds_nohs"][s])


def check(sizes, E_=10, C_=10, cc=None, al=None, bl=None, frames=1):
    from shapemol_amd import _lib
    from shapemol_amd._native import ptr
    lib = _lib.load()
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    slots = np.zeros(C_, np.int32)
    cc, al, bl = (np.ascontiguousarray(x if x is not None else np.linspace(0, 2, 100), np.float64) for x in (cc, al, bl))
    forms = np.full(len(sizes), -1, np.int32)
    rc = lib.shapemol_graph_check(frames, len(sizes), ptr(off), E_, C_, ptr(slots), ptr(cc), len(cc), 2.0, ptr(al), len(al), 12.0, ptr(bl), len(bl), ptr(forms))
    return (rc, lib.shapemol_last_error().decode() if rc else "", forms.tolist())


def test_host_refusals_name_the_offender():
    assert check([1, 64, 65, 256]) == (0, "", [0, 0, 1, 1])
    rc, msg, _ = check([5, 9, 257])
    assert rc == 1 and "molecule 2" in msg and "257" in msg and "limit is 256" in msg
    rc, msg, _ = check([5, 0, 3])
    assert rc == 1 and "molecule 1" in msg
    rc, msg, _ = check([5], E_=17)
    assert rc == 1 and "17 elements" in msg and "16" in msg
    rc, msg, _ = check([5], C_=33)
    assert rc == 1 and "33 atom classes" in msg and "32" in msg
    for kw, name in ((dict(cc=np.linspace(0, 2, 256)), "C-C"), (dict(al=np.linspace(0, 2, 256)), "all-pairs"), (dict(bl=np.linspace(0, 2, 256)), "bond-length")):
        rc, msg, _ = check([5], **kw)
        assert rc == 1 and name in msg and "255" in msg and "256" in msg
    rc, msg, _ = check([5], bl=np.array([1.0, 0.5]))
    assert rc == 1 and "ascending" in msg
    rc, msg, _ = check([5], frames=0)
    assert rc == 1 and "frames" in msg


def test_python_refusals_need_no_device():
    from shapemol_amd import StabilityRule, bond_graph, bond_graph_samples, bond_graph_trajectory
    rule = StabilityRule.from_json(E.RULE_JSON)
    pos, v, batch = np.zeros((5, 3), np.float32), np.array([1, 1, 3, 5, 0]), np.array([0, 0, 0, 1, 1])
    big = np.zeros((257, 3), np.float32)
    with pytest.raises(ValueError, match="limit is 256"):
        bond_graph(big, np.ones(257, np.int64), np.zeros(257, np.int64), rule)
    for kw in (dict(batch=np.array([0, 0, 0, 2, 2])), dict(batch=np.array([0, 1, 0, 1, 1])), dict(batch=np.array([0, 0, 0, 1])), dict(num_classes=33),
               dict(bond_bins=np.linspace(0, 2, 256)), dict(mode="aromatic")):
        args = dict(dict(pos=pos, v=v, batch=batch), **kw)
        with pytest.raises(ValueError):
            bond_graph(args.pop("pos"), args.pop("v"), args.pop("batch"), rule, **args)
    with pytest.raises(ValueError):
        bond_graph_trajectory([pos, pos], [v], batch, rule)
    with pytest.raises(ValueError, match="no atoms"):
        bond_graph_samples(([pos, np.zeros((0, 3))], [v, np.zeros(0, np.int64)]), rule)
    with pytest.raises(TypeError):
        bond_graph(pos, v.astype(np.float32), batch, rule)
    with pytest.raises(RuntimeError, match="no CPU path"):
        bond_graph(pos, v, batch, rule, device="cpu")


def test_abi_names_are_exported_and_bound():
    import shapemol_amd
    from shapemol_amd import _lib, mol_graph
    names = ("shapemol_graph_sizes", "shapemol_graph_check", "shapemol_graph_create", "shapemol_graph_destroy", "shapemol_graph_run",
             "shapemol_graph_bonds", "shapemol_graph_debug_fill")
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "shapemol_hip.h")).read()
    for n in names:
        assert n in _lib.EXPORTS and getattr(lib, n).argtypes is not None and f" {n}(" in header
    assert len(lib.shapemol_graph_run.argtypes) == 32 and len(lib.shapemol_graph_check.argtypes) == 15
    assert lib.shapemol_abi_version() == _lib.ABI_VERSION == 5
    assert tuple(mol_graph.sizes()) == (O.WAVE_ATOMS, O.MAX_ATOMS, E.MAX_ELEMENTS, E.MAX_CLASSES, E.MAX_EDGES, E.THREADS, O.RING_BITS)
    for n in ("GraphReport", "bond_graph", "bond_graph_trajectory", "bond_graph_samples", "atom_type_jsd", "to_molblock"):
        assert hasattr(shapemol_amd, n)


def test_to_molblock():
    from shapemol_amd import to_molblock
    pos = np.array([[0, 0, 0], [1.5, 0, 0], [2.8125, 0, 0], [-12.345678, 4, 0.5]])
    block = to_molblock(pos, [6, 7, 8, 17], np.array([[0, 1, 1], [1, 2, 2], [0, 3, 3]]), name="m")
    lines = block.split("\n")
    assert lines[0] == "m" and lines[3] == "  4  3  0  0  0  0  0  0  0  0999 V2000" and lines[-2] == "M  END" and lines[-1] == ""
    assert lines[4] == "    0.0000    0.0000    0.0000 C   0  0  0  0  0  0  0  0  0  0  0  0"
    assert lines[7].startswith("  -12.3457    4.0000    0.5000 Cl  0")
    assert lines[8:11] == ["  1  2  1  0", "  2  3  2  0", "  1  4  3  0"]
    assert len(lines) == 4 + 4 + 3 + 2
    for bad in ([[0, 4, 1]], [[0, 0, 1]], [[0, 1, 4]]):
        with pytest.raises(ValueError):
            to_molblock(pos, [6, 7, 8, 17], np.array(bad))
    with pytest.raises(ValueError):
        to_molblock(pos, [6, 7, 8], np.zeros((0, 3)))


def test_atom_type_jsd_is_the_direct_computation():
    from scipy.spatial import distance
    from shapemol_amd import atom_type_jsd
    emp = {6: 0.7, 7: 0.12, 8: 0.15, 9: 0.03}
    counts = {6: 70, 7: 9, 8: 20, 16: 1}                                     # sulfur is counted but is no key; no fluorine
    direct = distance.jensenshannon(np.array(list(emp.values())), np.array([70, 9, 20, 0]) / 100)
    assert atom_type_jsd(counts, emp) == direct
    cls = np.array([[30, 5, 10, 0, 1], [40, 4, 10, 0, 0]])                   # two frames of class counts; classes 0 and 4 are carbon
    by_class = atom_type_jsd(cls, emp, atomic_numbers=[6, 7, 8, 16, 6])
    assert by_class == distance.jensenshannon(np.array(list(emp.values())), np.array([71, 9, 20, 0]) / 100)
    assert atom_type_jsd({6: 0}, emp) is None
    with pytest.raises(ValueError):
        atom_type_jsd(cls, emp)
