"""Inputs, launch-form arithmetic and float64 recompositions of the chain-form tests (tests/test_chain_forms_cpu.py,
tests/test_gpu_chain_forms.py): the kernels that only a reverse step launches -- graph_kernel, the coordinate update folded into
the next x2h kernel (VnFold) or into the posterior kernel (DdpmFold), x2h_chain16_kernel -- and the streaming edge kernels'
tails, at the shapes where those forms switch or fill up.  No GPU code here: the formulas below restate the host's launch
decisions (csrc/sm_launch.h: stream_geom, and step_forms' fold and graph_fused) so that the shapes follow from the device's
CU count; tests/test_launch_geom_cpu.py holds them to that header over a sweep of sizes and CU counts, and the GPU tests check
them against the library's own record (debug_read "launch")."""
import numpy as np
import torch

import precision as P
from util import O, synth

GRAPH_CAP = 128         # kGraphCap: the largest molecule graph_kernel takes
FOLD_CAP = 256          # kVnFoldCap: rows of the folded coordinate update's LDS table
LAUNCH = ("sampling", "graph_fused", "vn_fold", "ddpm_fold", "x2h_chain", "stream_chunk", "stream_grid", "num_cu")
PROFILES = ("random", "lattice")
GRAPH_KS = (8, 4, 12, 16, 24, 32)
STREAM_KS = {8: (9, 40), 12: (13, 40), 24: (26, 48)}      # k (KP 8, 16, 32): molecule sizes of the streaming-tail batches


def kp_of(k):
    return 8 if k <= 8 else (16 if k <= 16 else 32)


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------------
# the host's launch arithmetic
# ------------------------------------------------------------------------------------------------------------------------
def stream_jobs(n, kp):
    """16-slot tiles of the streaming edge kernels: 16 / KP atoms each, or half an atom (k > 16)."""
    return 2 * n if kp > 16 else ceil_div(n, 16 // kp)


def stream_chunk(n, kp, num_cu):
    """Tiles per workgroup; k > 16: whole rounds of two tiles."""
    per_cu = ceil_div(stream_jobs(n, kp), num_cu)
    return max(1, per_cu) if kp <= 16 else max(2, ceil_div(per_cu, 2) * 2)


def stream_grid(n, kp, num_cu):
    return ceil_div(stream_jobs(n, kp), stream_chunk(n, kp, num_cu))


def fold_atoms(mode, n, kp, num_cu, hidden=128):
    """Atoms of one workgroup as step_forms' fold counts them (None: no fold on this path): the exact mode's streaming kernels own
    `chunk` tiles; the f16x2 kernels one tile per wave of max(waves, H / 16) waves, or `chunk` tiles when they loop."""
    if kp > 16:
        return None
    apj = 16 // kp
    if mode == "exact":
        return stream_chunk(n, kp, num_cu) * apj
    njobs = ceil_div(n, apj)
    waves = max(4, min(12, ceil_div(njobs, num_cu)))
    grid = max(1, min(num_cu, ceil_div(njobs, waves)))
    if njobs > grid * waves:
        lgrid = max(1, min(num_cu, ceil_div(njobs, 8)))
        return ceil_div(njobs, lgrid) * apj
    return max(waves, hidden // 16) * apj


def fold_expected(mode, counts, k, num_cu):
    """step_forms' fold for a chain on this batch with the true max_mol_atoms hint."""
    a = fold_atoms(mode, int(np.sum(counts)), kp_of(k), num_cu)
    return a is not None and a + 2 * (int(np.max(counts)) - 1) <= FOLD_CAP


def graph_fused_expected(counts):
    return int(np.max(counts)) <= GRAPH_CAP


def fold_largest_molecule(atoms_per_wg):
    """The largest max_mol_atoms at which a workgroup of that many atoms still folds."""
    return (FOLD_CAP - atoms_per_wg) // 2 + 1


def full_table_counts(atoms_per_wg, big, n_min=0, over=False):
    """Atom counts whose workgroup of atoms [w * a, w * a + a) starts on the last atom of a `big`-atom molecule and ends on the
    first atom of the next `big`-atom one: its span is a + 2 (big - 1) rows, the whole table when big = fold_largest_molecule(a).
    Filled with further molecules up to n_min atoms.  over: the second of the two molecules one atom larger (the table too small:
    the fold must go off)."""
    a = atoms_per_wg
    first = (-(big - 1)) % a or a                      # the workgroup boundary falls on the first big molecule's last atom
    counts = [first, big] + ([a - 2] if a > 2 else []) + [big + (1 if over else 0)]
    fill = [min(big, 97), 33, 9]
    i = 0
    while sum(counts) < n_min:
        counts.append(min(fill[i % len(fill)], max(1, n_min - sum(counts))))
        i += 1
    return np.asarray(counts, np.int64)


def straddled_span(counts, atoms_per_wg):
    """The largest molecule span (rows of the fold's table) over the workgroups of atoms_per_wg consecutive atoms."""
    off = np.concatenate([[0], np.cumsum(counts)])
    mol = np.repeat(np.arange(len(counts)), counts)
    n = int(off[-1])
    return max(int(off[mol[min(n, f + atoms_per_wg) - 1] + 1] - off[mol[f]]) for f in range(0, n, atoms_per_wg))


# ------------------------------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------------------------------
def graph_counts(k, extra=()):
    """The molecule sizes of the graph-stage tests.  KP = 8 (two atoms per wave, 32 candidate lanes per atom): 1, 2, k - 1 .. k + 2
    and both sides of every chunk edge up to the cap, ordered so that the 1-atom and the 128-atom molecule, and the 128-atom and the
    31-atom one, share a wave; KP >= 16 (64 lanes): 1, 2, k, k + 1 and the edges at 64 and 128.  N is odd."""
    if kp_of(k) == 8:
        c = [1, 128, 31, 2, k - 1, k, k + 1, k + 2, 32, 33, 63, 64, 65, 96, 97, 127]
    else:
        c = [1, 128, 63, 2, k, k + 1, 64, 65, 127]
    return np.asarray(c + list(extra), np.int64)


def graph_lanes(k):
    return 32 if kp_of(k) == 8 else 64


def wave_pairs(counts, k):
    """(chunks of the first atom's molecule, chunks of the second's) of every wave of graph_kernel whose two atoms lie in
    different molecules (KP = 8: atoms 2w and 2w + 1)."""
    if kp_of(k) != 8:
        return []
    mol = np.repeat(np.arange(len(counts)), counts)
    ch = [ceil_div(int(c), graph_lanes(k)) for c in counts]
    return [(ch[mol[i]], ch[mol[i + 1]]) for i in range(0, len(mol) - 1, 2) if mol[i] != mol[i + 1]]


def spread_counts(n, lo, hi, seed):
    """Molecule sizes in [lo, hi] (hashed) that sum to exactly n."""
    out, i = [], 0
    draws = synth.hash_u24(4 * (n // lo + 2), 301, seed)
    while sum(out) < n:
        out.append(min(lo + int(draws[i]) % (hi - lo + 1), n - sum(out)))
        i += 1
    return np.asarray(out, np.int64)


def lattice_positions(counts, seed):
    """Small-integer coordinates: every molecule on a cube grid of about its own atom count of cells, atom 1 on top of atom 0:
    squared distances are small integers (exact in float32), so many of them tie, some at zero."""
    pos = []
    for m, c in enumerate(counts):
        g = max(2, int(round(float(c) ** (1.0 / 3.0))))
        p = (synth.hash_u24(3 * int(c), 401 + m, seed).reshape(int(c), 3) % g).astype(np.float32) - np.float32(g // 2)
        if c > 1:
            p[1] = p[0]
        pos.append(p)
    return np.concatenate(pos).astype(np.float32)


def batch(counts, seed, profile="random", C=15, steps=0):
    """dict(counts, batch, init_pos, init_v, shape[, eps, u]) of the given molecule sizes."""
    counts = np.asarray(counts, np.int64)
    n, b = int(counts.sum()), len(counts)
    pos = synth.hash_normal((n, 3), 101, seed) if profile == "random" else lattice_positions(counts, seed)
    bb = dict(counts=counts, batch=np.repeat(np.arange(b, dtype=np.int64), counts), init_pos=pos,
              init_v=(np.arange(n) % C).astype(np.int64), shape=synth.hash_normal((b, 32, 3), 103, seed))
    if steps:
        eps, u = zip(*[synth.step_noise(n, C, s, seed=seed) for s in range(steps)])
        bb["eps"], bb["u"] = np.stack(eps), np.stack(u)
    return bb


def kth_ties(pos, k):
    """(atoms whose k-th and (k + 1)-th squared distances are equal in float32, zero distances) of one molecule."""
    x = torch.from_numpy(np.ascontiguousarray(pos, np.float32))
    d = x[:, None, :] - x[None, :, :]
    d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).clone()
    d2.fill_diagonal_(float("inf"))
    s = torch.sort(d2, dim=1)[0]
    return int((s[:, k - 1] == s[:, k]).sum()) if len(pos) > k + 1 else 0, int((d2 == 0).sum()) // 2


# ------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def graph_reference(sd, dm, bb):
    """(nbr (N, KP) int32 with -1 in the unused slots, valid mask, e_w float32 oracle (N, KP), e_w float64 oracle (N, KP)) of the
    initial positions: O.knn_edges in its own order (ascending (squared distance, index)) and O._edge_weight on those edges."""
    n, k, kp = len(bb["batch"]), dm.k, kp_of(dm.k)
    pos, b = _t(bb["init_pos"]), _t(bb["batch"])
    src, dst = O.knn_edges(pos, b, k)
    slot = torch.arange(len(dst)) - torch.searchsorted(dst, dst)          # position of the edge among its centre's
    nbr = np.full((n, kp), -1, np.int32)
    nbr[dst.numpy(), slot.numpy()] = src.numpy()
    ew = []
    for dt in (torch.float32, torch.float64):
        with torch.no_grad():
            e = O._edge_weight(O._Precision(sd, dt), pos.to(dt), src, dst).double().numpy().reshape(-1)
        full = np.zeros((n, kp), np.float64)
        full[dst.numpy(), slot.numpy()] = e
        ew.append(full)
    return nbr, nbr >= 0, ew[0], ew[1]


def step_state(bb, r, s):
    """(pos, v) before reverse step s of a chain with trajectories r: the initial state, or the chain's own state after step
    s - 1."""
    if s == 0:
        return bb["init_pos"], bb["init_v"]
    return np.asarray(r["pos_traj"][s - 1], np.float32), np.asarray(r["v_traj"][s - 1], np.int64)


def recompose(sd, dm, bb, r, s):
    """The score at the chain's own state before step s (timestep T - 1 - s) by the float32 and the float64 oracle:
    ({output: float64 array} x 2, timesteps (B,)).  No chain divergence enters: both oracles and the device see the same state,
    and the kNN graph is float32 in both oracles."""
    pos, v = step_state(bb, r, s)
    t = torch.full((len(bb["counts"]),), dm.T - 1 - s, dtype=torch.long)
    outs = []
    for dt in (torch.float32, torch.float64):
        o = O.score(sd, dm, _t(pos), _t(v), _t(bb["batch"]), _t(bb["shape"]), t, dtype=dt)
        outs.append({k: o[k].double().numpy() for k in ("pred_ligand_pos", "pred_ligand_v")})
    return outs[0], outs[1], t


def score_gate(got_pos, got_v, r32, r64):
    """precision.gate on a step's two predictions: {output: (eH, e32, eH / bound(e32))}."""
    return P.gate({"pred_ligand_pos": np.asarray(got_pos), "pred_ligand_v": np.asarray(got_v)}, r32, r64)


# ------------------------------------------------------------------------------------------------------------------------
# cases (shapes that depend on the CU count take it as an argument; the CPU tests use 256, the MI355X's)
# ------------------------------------------------------------------------------------------------------------------------
def fold_cases(num_cu=256):
    """{name: (mode, k, counts, vn_fold expected)}: the fold's table exactly full and one atom over, per launch path."""
    cases = {}
    for mode, k, chunk, tag in (("exact", 8, 1, "k8_chunk1"), ("exact", 8, 2, "k8_chunk2"), ("exact", 12, 2, "k12_chunk2"), ("f16x2", 8, 0, "k8")):
        kp = kp_of(k)
        apj = 16 // kp
        # exact mode: N in the range that gives `chunk` tiles per workgroup; f16x2: few enough tiles for one per wave
        n_min = 0 if chunk <= 1 else ((chunk - 1) * num_cu + 1) * apj
        a = chunk * apj if mode == "exact" else fold_atoms(mode, 300, kp, num_cu)
        big = fold_largest_molecule(a)
        for over in (False, True):
            counts = full_table_counts(a, big, n_min, over)
            cases[f"{mode}_{tag}_{'over' if over else 'full'}"] = (mode, k, counts, not over)
    return cases


def stream_sizes(kp, num_cu=256):
    """{name: N} of the streaming kernels' tails: tiles one fewer than (m), equal to (e) and one more than (p) a multiple c = 1, 2 of
    the CU count (k > 16 has two tiles per atom: two fewer / more), and three tiles per workgroup with a short last workgroup."""
    apj = 1 if kp >= 16 else 16 // kp
    out = {}
    for c in (1, 2):
        for d in (-1, 0, 1):
            jobs = num_cu * c + (2 * d if kp > 16 else d)
            n = jobs // 2 if kp > 16 else jobs * apj - (apj - 1)          # the odd N of a two-atom tile
            out[f"c{c}{'mep'[d + 1]}"] = n
    jobs3 = 2 * num_cu + 2                                             # three tiles per workgroup (four on whole rounds), not a multiple
    out["chunk3_short"] = jobs3 // 2 if kp > 16 else jobs3 * apj - (apj - 1)
    return out


def stream_batch(k, n, seed=5):
    lo, hi = STREAM_KS[k]
    return batch(spread_counts(n, lo, hi, seed), seed)
