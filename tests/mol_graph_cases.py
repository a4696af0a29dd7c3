"""Crafted molecules for the bond-graph tests, shared by tests/test_mol_graph_cpu.py (which asserts that
every case is well-posed) and tests/test_gpu_mol_graph.py.  All coordinates are multiples of 1/16 A, exact in float32, and
chosen so that no pair sits near a threshold of the rule in tests/golden/mol_eval_rule.json.  Atom classes are those of the
"basic" vocabulary, whose class index is the rule's row: 0 H, 1 C, 2 N, 3 O.  Carbon pairs bond below 1.23 (triple), 1.39
(double), 1.64 A (single)."""
import numpy as np

C_, N_, O_ = 1, 2, 3
TRI = [(0, 0, 0), (1.5, 0, 0), (0.75, 1.25, 0)]                      # sides 1.5, 1.4577, 1.4577


def mol(points, classes=None):
    p = np.asarray(points, np.float32).reshape(-1, 3)
    assert np.array_equal(p * 16, np.round(p * 16)) or np.isnan(p).any()
    return p, np.full(len(p), C_, np.int64) if classes is None else np.asarray(classes, np.int64)


def path(n, order=None):
    """n carbons 1.5 A apart on a line; `order`: the atom index of every position along the line."""
    p = np.zeros((n, 3), np.float32)
    p[:, 0] = 1.5 * np.arange(n)
    return mol(p if order is None else p[np.argsort(order)])


def cycle(n):
    """An even ring of n >= 6 carbons: two rows 3 A apart and one atom closing each end (1.58 A from both rows' ends)."""
    m = (n - 2) // 2
    top = [(1.5 * k, 0, 0) for k in range(m)]
    bottom = [(1.5 * k, -3, 0) for k in reversed(range(m))]
    return mol(top + [(1.5 * (m - 1) + 0.5, -1.5, 0)] + bottom + [(-0.5, -1.5, 0)])


HEX = [(0, 0, 0), (1.25, 0.75, 0), (2.5, 0, 0), (2.5, -1.5, 0), (1.25, -2.25, 0), (0, -1.5, 0)]


def shifted(points, d):
    return [(x + d[0], y + d[1], z + d[2]) for x, y, z in points]


def lattice_walk(rng, n, classes=(C_, C_, C_, N_)):
    """A random walk on the 1/4 A lattice with steps of 1.22 .. 1.5 A: bonds of every order, crowded and coincident atoms.
    Lattice distances are sqrt(k) / 4, so 100 * d = 25 sqrt(k) meets a threshold only where that is a multiple of 25; C and N
    have none (C-O 125 and N-O 150 are: no oxygen here)."""
    steps = []
    for v in ((1.5, 0, 0), (1.25, 0.75, 0), (1, 1, 0.5), (1.25, 0.5, 0), (1, 0.5, 0.5), (1.25, 0.25, 0.25)):
        for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)):
            for sx in (1, -1):
                for sy in (1, -1):
                    for sz in (1, -1):
                        steps.append((sx * v[perm[0]], sy * v[perm[1]], sz * v[perm[2]]))
    steps = np.unique(np.array(steps, np.float32), axis=0)
    p = np.cumsum(steps[rng.integers(0, len(steps), n)], 0)
    return mol(p, rng.choice(classes, n))


def structures():
    """name -> (pos, classes, expectation): what the structure is named after, checked against the oracle on the CPU."""
    rng = np.random.default_rng(24)
    cube = [(x, y, z) for x in (0, 1.5) for y in (0, 1.5) for z in (0, 1.5)]
    grid = [(0.25 * a, 0.25 * b, 0.25 * c) for a in range(4) for b in range(4) for c in range(4)]
    nan_path = np.array([(1.5 * k, 0, 0) for k in range(5)], np.float32)
    nan_path[2, 0] = np.nan
    scrambled = [3, 6, 0, 5, 1, 4, 2]
    s = {
        "path64": path(64) + (dict(n_bonds=63, n_frags=1, n_cycles=0, rings={0}),),
        "path256": path(256) + (dict(n_bonds=255, n_frags=1, n_cycles=0, rings={0}),),
        "cycle3": mol(TRI) + (dict(n_bonds=3, n_frags=1, n_cycles=1, rings={3}),),
        "cycle6": mol(HEX) + (dict(n_bonds=6, n_frags=1, n_cycles=1, rings={6}),),
        "cycle64": cycle(64) + (dict(n_bonds=64, n_frags=1, n_cycles=1, rings={31}),),        # 64 bonds: the bit of "larger than 30"
        "cycle256": cycle(256) + (dict(n_bonds=256, n_frags=1, n_cycles=1, rings={31}),),
        "fused66": mol(HEX + shifted(HEX, (2.5, 0, 0))[1:5]) + (dict(n_bonds=11, n_frags=1, n_cycles=2, rings={6}),),
        "spiro33": mol(TRI + [(-1.5, 0, 0), (-0.75, -1.25, 0)]) + (dict(n_bonds=6, n_frags=1, n_cycles=2, rings={3}),),
        "cube": mol(cube) + (dict(n_bonds=12, n_frags=1, n_cycles=5, rings={4}),),
        "two_rings": mol(TRI + shifted(HEX, (10, 0, 0))) + (dict(n_bonds=9, n_frags=2, n_cycles=2, rings={3, 6}),),
        "scrambled": mol(np.concatenate([path(7, scrambled)[0], np.array(shifted(TRI, (0, 8, 0)), np.float32)])) +
        (dict(n_bonds=9, n_frags=2, n_cycles=1, rings={0, 3}),),
        "cluster20": mol(grid[:20]) + (dict(n_bonds=190, n_frags=1, n_cycles=171, rings={3}),),
        "orders123": mol([(0, 0, 0), (1.5, 0, 0), (2.8125, 0, 0), (4, 0, 0)]) + (dict(n_bonds=3, n_frags=1, n_cycles=0, rings={0}, orders=[1, 2, 3]),),
        "nan_atom": mol(nan_path) + (dict(n_bonds=2, n_frags=3, n_cycles=0, rings={0}),),
        "lone_pair": mol([(0, 0, 0), (5, 0, 0)]) + (dict(n_bonds=0, n_frags=2, n_cycles=0, rings=set()),),
        "hetero": mol(HEX, [C_, N_, C_, O_, C_, N_]) + (dict(n_bonds=6, n_frags=1, n_cycles=1, rings={6}),),
        "walk40": lattice_walk(rng, 40) + (None,),
    }
    return s


def pack(mols):
    """[(pos, classes), ...] -> pos (N, 3), classes (N,), batch (N,), off (B + 1)."""
    sizes = [len(m[1]) for m in mols]
    return (np.concatenate([m[0] for m in mols]), np.concatenate([m[1] for m in mols]), np.repeat(np.arange(len(mols)), sizes),
            np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))


def ragged_batch():
    """T1: molecules of 1, 2, 9, 64, 65, 30, 256, 63 and 255 atoms in one batch, both launch forms, with a molecule without
    bonds (two distant atoms) between two with bonds."""
    rng = np.random.default_rng(7)
    mols = [mol([(0, 0, 0)]), lattice_walk(rng, 9), mol([(0, 0, 0), (5, 0, 0)]), lattice_walk(rng, 64), lattice_walk(rng, 65), lattice_walk(rng, 30),
            lattice_walk(rng, 256), lattice_walk(rng, 63), lattice_walk(rng, 255), mol([(0, 0, 0), (1.5, 0, 0)])]
    return mols
