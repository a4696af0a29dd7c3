"""Stress profiles and the error measure of the precision gates (tests/test_gpu_precision.py, tests/test_precision_cpu.py).

A profile is a deterministic function of its configuration and seeds: a reference-layout state dict {key: ndarray} and a batch,
loadable into shapemol_amd.ScorePosNet3D and the CPU oracle alike.

  P0  natural       synth.synthetic_state_dict as everywhere else in the suite
  P1  small         every MLP's first Linear (net.0: each Linear that feeds a LayerNorm), weight and bias, scaled by 2^-6
  P2  wide range    every Linear / vector-neuron weight and bias redrawn heavy-tailed (Laplace, one entry in 256 an outlier
                    x16) at a per-tensor power-of-two scale in 2^-8 .. 2^2
  P3  geometry      P0 weights; molecules translated by 20-60 A per axis, one near-coincident atom pair (0.005-0.02 A) per
                    molecule, t = 0 / 999 / mixed by molecule

The error of an output Y against the float64 oracle Y64 is max|Y - Y64| / max|Y64|.  The gate (see bound()) compares the
kernel's error eH with the float32 oracle's own error e32 on the same inputs.
"""
import numpy as np
import torch

from util import O, model_cfg, synth
from tools_knn import knn_margin_rel

PROFILES = ("P0", "P1", "P2", "P3")
SMALL = 2.0 ** -6           # P1 scale
P2_EXP = (-8, 2)            # P2: per-tensor scale 2^e, e in this closed range
MARGIN = 1e-5               # least relative kNN margin (d2_{k+1} - d2_k) / d2_k of every profile's batch
U = 2.0 ** -24              # float32 unit roundoff

# name: (model overrides, molecules, atoms_range or None for the MOSES prior, batch seed of P0-P2, batch seed of P3, atom types).
# The batch seeds are the first that give every atom a kNN margin of at least MARGIN (tests/test_precision_cpu.py checks it).
CONFIGS = {
    "b4": ({}, 4, None, 11, 11, 15),
    "b256": ({}, 256, None, 2021, 2021, 15),
    "k24": ({"knn": 24}, 16, (26, 48), 24, 24, 15),
    "k32": ({"knn": 32}, 16, (40, 80), 33, 35, 15),
    "small": ({"hidden_dim": 32, "n_heads": 4, "num_layers": 2}, 16, None, 16, 16, 15),
    "c23": ({}, 16, None, 23, 23, 23),      # the `full` vocabulary: two output tiles of the atom-type head, C > 16
}
WEIGHT_SEED = 7


def bound(e32):
    """The gate on the kernel's relative error eH:  eH <= 4 e32 + 16 u  (u = 2^-24).

    Error model.  The float32 oracle and a kernel that claims float32 precision evaluate the same graph of operations on the
    same inputs (same kNN graph, same float32 time features).  To first order each output's error is a sum of the local
    rounding errors, each multiplied by the same sensitivity of the output to that operation; only the local errors differ.
    float32 rounds each product and each partial sum to within u relative.  The exactly split bf16 products represent both
    operands exactly and drop three piece products (ml, lm < 2^-24 |x w| each, ll < 2^-32), so a product term is within
    3u of exact before the fp32 accumulation, which rounds as float32's does (in another order).  Its local errors are at most
    about three times float32's, and the realised error of a sum of many such terms, with independent signs, scales alike:
    factor 4.  The additive 16u (16 ulps of max|Y64|) covers the final float32 rounding of each result, which both sides
    pay once, and outputs with few operations before them (e_w: one MLP), where e32 may be small by chance.
    A two-piece f16 operand (hi + lo, both fp16) is within 2^-22 relative only where lo is a normal fp16 number and
    within 2^-25 ABSOLUTE below |x| = 2^-3: with P1's weights (|w| < 2^-9) that is above 2^-16 = 256u relative per operand,
    far outside the factor 4 (the negative controls)."""
    return 4.0 * e32 + 16.0 * U


def rel_err(y, y64):
    y64 = np.asarray(y64, np.float64)
    s = float(np.abs(y64).max())
    return float(np.abs(np.asarray(y, np.float64) - y64).max()) / s if s > 0 else 0.0


# ------------------------------------------------------------------------------------------------------------------------
# profiles
# ------------------------------------------------------------------------------------------------------------------------
def config(name):
    ov = CONFIGS[name][0]
    return model_cfg(**ov)


def classes(name):
    return CONFIGS[name][5]


def _laplace(shape, tag, seed):
    """Laplace draws of unit variance from hash uniforms (u = 0 excluded by half a grid step)."""
    u = synth.hash_uniform(shape, tag, seed).astype(np.float64) + 2.0 ** -25 - 0.5
    return -np.sign(u) * np.log1p(-2.0 * np.abs(u)) / np.sqrt(2.0)


def state_dict(profile, cfg, seed=WEIGHT_SEED, num_classes=15):
    """(state dict {key: float32 ndarray}, {key: scale applied}) of a profile."""
    from shapemol_amd.spec import ModelDims, state_dict_spec
    sdn = synth.synthetic_state_dict(cfg, seed=seed, num_classes=num_classes)
    scales = {}
    if profile == "P1":
        for k in sdn:
            if ".net.0." in k:
                sdn[k] = (sdn[k] * np.float32(SMALL)).astype(np.float32)
                scales[k] = SMALL
    elif profile == "P2":
        lo, hi = P2_EXP
        for key, (shape, kind, fan_in) in state_dict_spec(ModelDims(cfg, num_classes)).items():
            if kind not in ("weight", "bias"):
                continue
            tag = synth.key_tag(key)
            e = lo + int(synth.hash_u24(1, tag ^ 0x5C, seed)[0]) % (hi - lo + 1)
            z = _laplace(tuple(shape), tag ^ 0x3A, seed)
            z = np.where(synth.hash_u24(z.size, tag ^ 0x4B, seed).reshape(z.shape) % 256 == 0, 16.0 * z, z)
            sdn[key] = (z / np.sqrt(3.0 * fan_in) * 2.0 ** e).astype(np.float32)      # (the variance of U(-1, 1) / sqrt(fan_in))
            scales[key] = 2.0 ** e
    elif profile not in ("P0", "P3"):
        raise ValueError(profile)
    return sdn, scales


def batch(profile, cname):
    """dict(pos (N,3) f32, v (N,) i64, batch (N,) i64, shape (B,S,3) f32, t (B,) i64) of a profile in configuration cname."""
    _, nmol, rng, seed, seed3, ncls = CONFIGS[cname]
    geo = profile == "P3"
    bb = synth.synthetic_batch(nmol, seed=seed3 if geo else seed, atoms_range=rng, num_classes=ncls)
    pos, b = bb["init_pos"].copy(), bb["batch"]
    t = (synth.hash_u24(nmol, 9, seed) % 1000).astype(np.int64)
    if geo:
        start = np.concatenate([[0], np.cumsum(bb["counts"])[:-1]])
        u = synth.hash_uniform((nmol, 3), 201, seed3).astype(np.float64)
        sgn = np.where(synth.hash_u24(nmol * 3, 202, seed3).reshape(nmol, 3) % 2 == 0, 1.0, -1.0)
        d = synth.hash_normal((nmol, 3), 203, seed3).astype(np.float64)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        gap = 0.005 + 0.015 * synth.hash_uniform((nmol,), 204, seed3).astype(np.float64)
        for m, s in enumerate(start):                           # atom s + 1 next to atom s
            pos[s + 1] = (pos[s].astype(np.float64) + gap[m] * d[m]).astype(np.float32)
        pos = (pos.astype(np.float64) + (sgn * (20.0 + 40.0 * u))[b]).astype(np.float32)
        t = np.where(np.arange(nmol) % 3 == 0, 0, np.where(np.arange(nmol) % 3 == 1, 999, t)).astype(np.int64)
    return dict(pos=pos, v=bb["init_v"], batch=b, shape=bb["shape"], t=t, counts=bb["counts"])


def knn_margin(bt, k):
    """Least relative kNN margin over the molecules of a batch (float64 distances of the float32 positions)."""
    start = np.concatenate([[0], np.cumsum(bt["counts"])])
    return min(knn_margin_rel(bt["pos"][start[i]:start[i + 1]], k) for i in range(len(bt["counts"])))


# ------------------------------------------------------------------------------------------------------------------------
# the outputs the gate compares
# ------------------------------------------------------------------------------------------------------------------------
def stop_layers(L):
    return [l for l in (1, 2, 4, 8) if l <= L]


def _by_neighbour(nbr, val):
    """Rows of (nbr, val) reordered by neighbour index (the kernels fill the slots in their own order)."""
    o = np.argsort(nbr, axis=1, kind="stable")
    return np.take_along_axis(nbr, o, 1), np.take_along_axis(val, o, 1)


def oracle_outputs(sd, dm, bt, dtype=torch.float64, operands=None):
    """{output name: float64 ndarray} of one oracle evaluation, plus 'nbr' (N, k) sorted per atom."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))       # noqa: E731
    taps = {}
    out = O.score(sd, dm, T(bt["pos"]), T(bt["v"]), T(bt["batch"]), T(bt["shape"]), T(bt["t"]), taps, dtype=dtype, operands=operands)
    n = len(bt["batch"])
    src, dst = taps["edge_index"].numpy()
    k = len(src) // n
    assert np.array_equal(dst, np.repeat(np.arange(n), k)), "every atom needs k neighbours"
    nbr, ew = _by_neighbour(src.reshape(n, k), taps["e_w"].double().numpy().reshape(n, k))
    r = {"nbr": nbr, "ew": ew}
    pos = bt["pos"].astype(np.float64)
    for nl in stop_layers(dm.L):
        r[f"h@{nl}"] = taps[f"h_{nl - 1}"].double().numpy()
        r[f"dx@{nl}"] = taps[f"x_{nl - 1}"].double().numpy() - pos
    for key in ("pred_ligand_pos", "pred_ligand_h", "pred_ligand_v"):
        r[key] = out[key].double().numpy()
    return r


def gate(res, r32, r64):
    """{output: (eH, e32, eH / bound(e32))} for the outputs of res (a kernel's or an emulation's) against the two oracles."""
    out = {}
    for key in r64:
        if key == "nbr" or key not in res:
            continue
        eh, e32 = rel_err(res[key], r64[key]), rel_err(r32[key], r64[key])
        out[key] = (eh, e32, eh / bound(e32))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# operand formats of the kernels, emulated on the CPU (O.score(..., operands=...)): both matrix operands of every Linear rounded,
# the arithmetic after that in the oracle's dtype
# ------------------------------------------------------------------------------------------------------------------------
def bf16x3(x):
    """The exact three-piece bf16 split (sm_device.h) represents every float32 exactly: the operand is its float32 value."""
    return x.float().to(x.dtype)


def f16x2(x):
    """Two round-to-nearest fp16 pieces of the float32 operand: hi = f16(x), lo = f16(x - hi) (fp16 subnormals kept)."""
    x32 = x.float()
    hi = x32.half()
    lo = (x32 - hi.float()).half()
    return hi.to(x.dtype) + lo.to(x.dtype)
