"""Model configurations at the edges of what shapemol_create accepts, with their batches (tests/test_config_space_cpu.py,
tests/test_gpu_config_space.py; the audit behind the table is profiles/config_space/README.md).

Every case is a deterministic function of this table: a model configuration (util.model_cfg overrides), the number of atom types,
a weight seed (synth.synthetic_state_dict) and two batches:

  full    molecules of k + 2 .. k + 14 atoms (at least 6): every atom has k neighbours, so neighbour lists and per-layer taps can be
          compared row by row
  ragged  molecules of 1, 2, 9, 16, 17, 18, 33 and 40 atoms, built as tests/golden/make_golden.py builds forward_ragged: at
          KP = 32 atoms whose second half tile is empty or holds one slot, an atom with no neighbour at all, and the k + 1 boundary
          of k = 16 and 17

REFUSED holds the rows of the grid that shapemol_create refuses (hidden width 32 with k > 16).

The batch seeds are the first (from the case's base seed) that give every molecule with more than k + 1 atoms a relative kNN
margin of at least precision.MARGIN (test_config_space_cpu.py checks it): otherwise neighbour order, not arithmetic, decides a
comparison with the kernels.
"""
import numpy as np
import torch

import precision as P
from util import O, model_cfg, synth

RAGGED_COUNTS = (1, 2, 9, 16, 17, 18, 33, 40)
OUTPUTS = ("pred_ligand_pos", "pred_ligand_h", "pred_ligand_v")
BATCHES = ("full", "ragged")


def _model(H, k, S, SL, D, L):
    return {"hidden_dim": H, "n_heads": H // 8, "knn": k, "shape_dim": S, "shape_latent_dim": SL, "time_emb_dim": D, "num_layers": L}


# name: (model overrides, atom types, weight seed, seed of the full batch, seed of the ragged batch)
CASES = {
    "h32_k16_c17": (_model(32, 16, 32, 32, 8, 2), 17, 7, 103, 203),     # full 16-slot tile; two output tiles of the atom-type head at H = 32
    "h32_k9": (_model(32, 9, 5, 8, 4, 2), 15, 7, 104, 204),             # low edge of KP = 16; small S, SL, D together
    "h128_k17": (_model(128, 17, 32, 32, 8, 2), 15, 7, 105, 205),       # the same half-tile edge at full width
    "h128_k1": (_model(128, 1, 1, 4, 4, 1), 15, 7, 106, 206),           # one neighbour, one shape point, smallest latent and time width, one layer
    "h128_max": (_model(128, 8, 64, 64, 16, 1), 15, 7, 107, 207),       # upper limits of S, SL, D
    "h128_sl36": (_model(128, 8, 33, 36, 6, 3), 15, 7, 108, 208),       # one past 32 in S and SL (non-tiled shape-term kernel), D not a power of two
    "h32_max_k16": (_model(32, 16, 64, 64, 16, 1), 32, 7, 110, 211),    # every upper limit the reduced model supports at once (32 atom types)
}
# Rows of the grid that shapemol_create refuses (check_cfg: knn > 16 needs hidden_dim 128; profiles/config_space/README.md has the
# reason): the packer and the oracle still take them, no context can be created.  name: (model overrides, atom types)
REFUSED = {
    "h32_k32": (_model(32, 32, 32, 32, 8, 2), 15),
    "h32_k17": (_model(32, 17, 32, 32, 8, 2), 15),
    "h32_max_k32": (_model(32, 32, 64, 64, 16, 1), 32),
}
KP32 = tuple(n for n, c in CASES.items() if c[0]["knn"] > 16)
CHAIN_CASES = ("h128_k17", "h128_sl36", "h32_max_k16")
CHAIN_STEPS = 3


def overrides(name):
    return dict((CASES.get(name) or REFUSED[name])[0])


def config(name):
    return model_cfg(**overrides(name))


def classes(name):
    return (CASES.get(name) or REFUSED[name])[1]


def weight_seed(name):
    return CASES[name][2]


def state_dict(name):
    return synth.synthetic_state_dict(config(name), seed=weight_seed(name), num_classes=classes(name))


def full_batch(name, seed=None):
    """Molecules of k + 2 .. k + 14 atoms (a floor of 6 for the smallest k): six of them for k > 17, eight otherwise."""
    ov, C = CASES[name][0], classes(name)
    k, S = ov["knn"], ov["shape_dim"]
    seed = CASES[name][3] if seed is None else seed
    nmol = 6 if k > 17 else 8
    bb = synth.synthetic_batch(nmol, seed=seed, atoms_range=(max(k + 2, 6), k + 14), shape_points=S, num_classes=C)
    t = (synth.hash_u24(nmol, 9, seed) % 1000).astype(np.int64)
    return dict(pos=bb["init_pos"], v=bb["init_v"], batch=bb["batch"], shape=bb["shape"], t=t, counts=bb["counts"])


def ragged_batch(name, seed=None):
    """The sizes of RAGGED_COUNTS with hash-drawn positions (x2, as forward_ragged), types, shapes and per-molecule t."""
    ov, C = CASES[name][0], classes(name)
    S = ov["shape_dim"]
    seed = CASES[name][4] if seed is None else seed
    counts = np.array(RAGGED_COUNTS, np.int64)
    n, nmol = int(counts.sum()), len(counts)
    return dict(pos=synth.hash_normal((n, 3), 201, seed) * np.float32(2.0), v=(synth.hash_u24(n, 202, seed) % C).astype(np.int64),
                batch=np.repeat(np.arange(nmol, dtype=np.int64), counts), shape=synth.hash_normal((nmol, S, 3), 203, seed),
                t=(synth.hash_u24(nmol, 9, seed) % 1000).astype(np.int64), counts=counts)


def batch(name, which, seed=None):
    return full_batch(name, seed) if which == "full" else ragged_batch(name, seed)


def first_seed(name, which, tries=64):
    """The first seed from the case's base seed whose batch has a kNN margin of at least precision.MARGIN."""
    base = CASES[name][3 if which == "full" else 4]
    k = CASES[name][0]["knn"]
    for seed in range(base, base + tries):
        if P.knn_margin(batch(name, which, seed), k) >= P.MARGIN:
            return seed
    raise AssertionError(f"{name}/{which}: no seed in {base}..{base + tries - 1} has a kNN margin of {P.MARGIN}")


# ------------------------------------------------------------------------------------------------------------------------
# oracle evaluations, computed once per process and left unchanged
# ------------------------------------------------------------------------------------------------------------------------
_memo = {}


def oracle(name):
    """(oracle state dict, O.Dims) of a case."""
    key = ("model", name)
    if key not in _memo:
        _memo[key] = (O.state_dict_from_numpy(state_dict(name)), O.Dims(config(name), classes(name)))
    return _memo[key]


def score3(sd, dm, bt, dtype=torch.float64):
    """{output: float64 ndarray} of the three outputs of one oracle evaluation (any batch: no assumption on neighbour counts)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))       # noqa: E731
    out = O.score(sd, dm, T(bt["pos"]), T(bt["v"]), T(bt["batch"]), T(bt["shape"]), T(bt["t"]), dtype=dtype)
    return {k: out[k].double().numpy() for k in OUTPUTS}


def refs(name, which):
    """(batch, float32 oracle outputs, float64 oracle outputs): with the taps, neighbour lists and edge weights of
    precision.oracle_outputs on the full batch, the three outputs on the ragged one."""
    key = ("refs", name, which)
    if key not in _memo:
        sd, dm = oracle(name)
        bt = batch(name, which)
        if which == "full":
            _memo[key] = (bt, P.oracle_outputs(sd, dm, bt, torch.float32), P.oracle_outputs(sd, dm, bt, torch.float64))
        else:
            _memo[key] = (bt, score3(sd, dm, bt, torch.float32), score3(sd, dm, bt, torch.float64))
    return _memo[key]


def chain_noise(name, n):
    """Host-fed noise (eps (steps, N, 3), u (steps, N, C)) of the short chains."""
    C, seed = classes(name), CASES[name][3]
    eps, u = zip(*[synth.step_noise(n, C, s, seed=seed) for s in range(CHAIN_STEPS)])
    return np.stack(eps), np.stack(u)


def chain_ref(name):
    """(full batch, eps, u, the oracle's chain of CHAIN_STEPS reverse steps from the full batch's positions and types)."""
    key = ("chain", name)
    if key not in _memo:
        sd, dm = oracle(name)
        bt = full_batch(name)
        eps, u = chain_noise(name, len(bt["batch"]))
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a))       # noqa: E731
        r = O.sample_chain(sd, dm, T(bt["pos"]), T(bt["v"]), T(bt["batch"]), T(bt["shape"]), CHAIN_STEPS, lambda s: (eps[s], u[s]),
                           keep_traj=False)
        _memo[key] = (bt, eps, u, r)
    return _memo[key]
