"""Float64 / float32 oracles of the training step's four device operators (shapemol_amd/training.py: HipMLP, HipEdgeMLP,
HipSegAttention, HipVN; kernels csrc/sm_train.h, host code csrc/train_ops.hip): plain torch on the CPU, the reference's
formulation of each operator, every gradient from torch autograd.  The cases are tests/train_ops_cases.py; the CPU test
(tests/test_train_ops_cpu.py) proves them well-posed, the GPU test (tests/test_gpu_train_ops.py) gates the kernels.

Inputs are deterministic functions of the case and its seed (hash draws, shapemol_amd/synth.py: no generator state, the same
on every machine), rounded to float32 once; the float64 and the float32 run start from the same float32 values.

The gate per tensor is the project's: eH = max|res - r64| / max|r64| against precision.bound(e32) = 4 e32 + 16 * 2^-24.

Well-posedness (conditions on the float64 run alone, NOT measurements; the cap is zero offenders in every case):
  * MLP and edge form: no ReLU pre-activation pre = xhat * gamma + beta within 2^-16 * (|xhat * gamma| + |beta|) of zero.  A
    float32 evaluation of pre carries a few 2^-24 of that scale, so within the condition neither float32 side (oracle or
    kernel) can sit on the other side of the mask, and the mask's derivative is the same function for all three.
  * VN: no <p, d> within 2^-16 * |p| |d| of zero (the leaky-ReLU's mask), and no |pf| below 2^-10 of its channel's mean norm
    (pf / |pf| is ill-conditioned there).
They are reached by the choice of the seed (find_seed below, run on the CPU; the seed found stands in the cases file), not by
shifting beta, which would switch whole columns always-on and stop testing the mask.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from precision import bound, rel_err
from util import synth

F64, F32 = torch.float64, torch.float32
MASK_MARGIN = 2.0 ** -16        # relative distance of a mask argument from zero
NORM_FLOOR = 2.0 ** -10         # least |pf| relative to the channel's mean norm
SANE_E32 = 1e-3                 # the float32 oracle's own sanity bound

MLP_OUT = ("y", "dx", "dW1", "db1", "dgamma", "dbeta", "dW2", "db2")
EDGE_OUT = ("y", "dr", "dh", "ds", "dW1", "db1", "dgamma", "dbeta", "dW2", "db2")
ATTN_OUT = ("out", "dq", "dk", "dvals")
VN_OUT = ("out", "dx", "do3", "dWf", "dWd", "dbn_w", "dbn_b", "run_mean", "run_var")


class _Draw:
    """float32 normal draws, one tag per call in call order: a pure function of (seed, call index, element index)."""

    def __init__(self, seed):
        self.seed, self.tag = int(seed), 0

    def __call__(self, *shape, sc=1.0):
        self.tag += 1
        return (torch.from_numpy(synth.hash_normal(tuple(shape), self.tag, self.seed)) * sc).float()

    def ints(self, n, lo, hi):
        """n integers in [lo, hi]."""
        self.tag += 1
        return torch.from_numpy(lo + synth.hash_u24(n, 1000 + self.tag, self.seed) % (hi - lo + 1))


def _leaves(tensors, dtype):
    return [t.to(dtype).clone().requires_grad_(True) for t in tensors]


def _np(t):
    return t.detach().double().numpy()


# ------------------------------------------------------------------------------------------------------------------------
# graphs: edges (src = neighbour, dst = centre) grouped by centre with CSR offsets, as training.EdgeGraph wants them
# ------------------------------------------------------------------------------------------------------------------------
def graph(n_atoms, degrees, draw):
    """(src, dst, ptr) int64 of a degree specification:
    ("rand", lo, hi)   degrees uniform in [lo, hi]; with more than two atoms, atom 1 has no edges as centre and atom 2 is
                       nobody's neighbour (its edges go to atom 0)
    ("set", (a, b..))  every degree one of the listed values, atom 0 the first listed, atom 1 the second, ...; atom 2 is
                       nobody's neighbour
    ("total", E)       exactly E edges, spread evenly (the first E % n atoms one more)
    ("hub", d)         d edges per atom, every edge's neighbour is atom 0: one perm_src segment holds all edges"""
    kind = degrees[0]
    if kind == "rand":
        deg = draw.ints(n_atoms, degrees[1], degrees[2])
        if n_atoms > 2:
            deg[1] = 0
    elif kind == "set":
        vals = torch.tensor(degrees[1])
        deg = vals[draw.ints(n_atoms, 0, len(vals) - 1)]
        deg[:min(len(vals), n_atoms)] = vals[:n_atoms]
    elif kind == "total":
        deg = torch.full((n_atoms,), degrees[1] // n_atoms, dtype=torch.int64)
        deg[:degrees[1] % n_atoms] += 1
    elif kind == "hub":
        deg = torch.full((n_atoms,), degrees[1], dtype=torch.int64)
    else:
        raise ValueError(degrees)
    ptr = torch.zeros(n_atoms + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(deg, 0)
    E = int(ptr[-1])
    dst = torch.repeat_interleave(torch.arange(n_atoms), deg)
    src = torch.zeros(E, dtype=torch.int64) if kind == "hub" else draw.ints(E, 0, n_atoms - 1)
    if kind in ("rand", "set") and n_atoms > 2:
        src[src == 2] = 0
    return src, dst, ptr


# ------------------------------------------------------------------------------------------------------------------------
# MLP: Linear -> LayerNorm(1e-5) -> ReLU -> Linear  (models/common.py:47-67)
# ------------------------------------------------------------------------------------------------------------------------
def _mlp_weights(draw, k_in, hidden, n_out):
    return [draw(hidden, k_in, sc=k_in ** -0.5), draw(hidden, sc=0.3), 1 + draw(hidden, sc=0.2), draw(hidden, sc=0.3),
            draw(n_out, hidden, sc=hidden ** -0.5), draw(n_out, sc=0.3)]


def mlp_inputs(case):
    """dict(x, ws = [W1, b1, gamma, beta, W2, b2], dy) of float32 CPU tensors."""
    draw = _Draw(case.seed)
    return dict(x=draw(case.rows, case.k_in), ws=_mlp_weights(draw, case.k_in, case.hidden, case.n_out), dy=draw(case.rows, case.n_out))


def _mlp_tail(rows_in, w, dy, dtype, taps):
    z = F.linear(rows_in, w[0], w[1])
    hidden = w[0].shape[0]
    xhat = F.layer_norm(z, (hidden,), None, None, 1e-5)
    if taps is not None:
        taps["xhat_gamma"], taps["beta"] = _np(xhat * w[2]), _np(w[3])
    y = F.linear(torch.relu(F.layer_norm(z, (hidden,), w[2], w[3], 1e-5)), w[4], w[5])
    y.backward(dy.to(dtype))
    return y


def mlp(inp, dtype, taps=None):
    """{name: float64 ndarray} of MLP_OUT in dtype; taps (a dict) receives the ReLU's argument for the predicates."""
    b = _leaves([inp["x"]] + inp["ws"], dtype)
    y = _mlp_tail(b[0], b[1:], inp["dy"], dtype, taps)
    return dict(zip(MLP_OUT, [_np(y)] + [_np(t.grad) for t in b]))


# ------------------------------------------------------------------------------------------------------------------------
# Edge form: the MLP on the concatenation [r_e | h_dst | h_src | s_dst]  (models/uni_transformer.py:60-66)
# ------------------------------------------------------------------------------------------------------------------------
def edge_inputs(case):
    draw = _Draw(case.seed)
    src, dst, ptr = graph(case.n_atoms, case.degrees, draw)
    E, K1 = src.numel(), case.k_edge + 2 * case.k_node + case.k_shape
    return dict(src=src, dst=dst, ptr=ptr, r=draw(E, case.k_edge), h=draw(case.n_atoms, case.k_node), s=draw(case.n_atoms, case.k_shape),
                ws=_mlp_weights(draw, K1, case.hidden, case.n_out), dy=draw(E, case.n_out))


def edge_mlp(inp, dtype, taps=None):
    b = _leaves([inp["r"], inp["h"], inp["s"]] + inp["ws"], dtype)
    rows = torch.cat([b[0], b[1][inp["dst"]], b[1][inp["src"]], b[2][inp["dst"]]], -1)
    y = _mlp_tail(rows, b[3:], inp["dy"], dtype, taps)
    return dict(zip(EDGE_OUT, [_np(y)] + [_np(t.grad) if t.grad is not None else np.zeros(tuple(t.shape)) for t in b]))


# ------------------------------------------------------------------------------------------------------------------------
# Segment attention: scaled logits, softmax over each centre's edges, weighted sum  (models/uni_transformer.py:71-81)
# ------------------------------------------------------------------------------------------------------------------------
def attn_inputs(case):
    draw = _Draw(case.seed)
    _, dst, ptr = graph(case.n_atoms, case.degrees, draw)
    n, E, heads, dh, W = case.n_atoms, dst.numel(), case.heads, case.dh, case.W
    q, k = draw(n, heads * dh) * 2, draw(E, heads * dh) * 2
    if case.big_logits:
        # the first `big_logits` atoms with two or more edges: one end of the atom's edge list gets logit +100, the other -100,
        # in every head (k_e = +-q_i * 100 sqrt(dh) / |q_i|^2); the +100 on the first edge of even atoms, on the last of odd ones
        done = 0
        qv, kv = q.view(n, heads, dh), k.view(E, heads, dh)
        for i in range(n):
            e0, e1 = int(ptr[i]), int(ptr[i + 1])
            if e1 - e0 < 2 or done == case.big_logits:
                continue
            big = qv[i].double() * (100.0 * math.sqrt(dh)) / (qv[i].double() ** 2).sum(-1, keepdim=True)
            hi, lo = (e0, e1 - 1) if done % 2 == 0 else (e1 - 1, e0)
            kv[hi], kv[lo] = big.float(), (-big).float()
            done += 1
        assert done == case.big_logits
    return dict(dst=dst, ptr=ptr, q=q, k=k, vals=draw(E, heads, W), dout=draw(n, heads, W))


def seg_attention(inp, heads, dtype, taps=None):
    b = _leaves([inp["q"], inp["k"], inp["vals"]], dtype)
    dst, n = inp["dst"], inp["q"].shape[0]
    dh, W = inp["q"].shape[1] // heads, inp["vals"].shape[2]
    logit = (b[0][dst].view(-1, heads, dh) * b[1].view(-1, heads, dh) / math.sqrt(dh)).sum(-1)
    idx = dst.view(-1, 1).expand_as(logit)
    mx = torch.full((n, heads), float("-inf"), dtype=dtype).scatter_reduce(0, idx, logit.detach(), "amax")
    ex = torch.exp(logit - mx[dst])
    alpha = ex / torch.zeros((n, heads), dtype=dtype).index_add(0, dst, ex)[dst]
    out = torch.zeros((n, heads, W), dtype=dtype).index_add(0, dst, alpha.unsqueeze(-1) * b[2])      # atoms without edges: zeros
    out.backward(inp["dout"].to(dtype))
    if taps is not None:
        taps["logit"] = _np(logit)
    return dict(zip(ATTN_OUT, [_np(out)] + [_np(t.grad) for t in b]))


# ------------------------------------------------------------------------------------------------------------------------
# VN: VNLinearLeakyReLU with VNBatchNorm, mean over the channels  (models/shape_vn_layers.py:41-61,95-110)
# ------------------------------------------------------------------------------------------------------------------------
def vn_counts(case):
    """Atoms per molecule: case.atoms spread over case.n_mol molecules, the first ones one more."""
    c = np.full(case.n_mol, case.atoms // case.n_mol, np.int64)
    c[:case.atoms % case.n_mol] += 1
    return torch.from_numpy(c)


def vn_inputs(case):
    draw = _Draw(case.seed)
    n, ch, cin = case.atoms, case.C, 1 + case.rows_o + case.rows_s
    batch = torch.repeat_interleave(torch.arange(case.n_mol), vn_counts(case))
    return dict(batch=batch, x=draw(n, 3), o3=draw(n, case.rows_o, 3, sc=0.5), shape=draw(case.n_mol, case.rows_s, 3),
                ws=[draw(ch, cin, sc=cin ** -0.5), draw(ch, cin, sc=cin ** -0.5), 1 + draw(ch, sc=0.2), draw(ch, sc=0.3)],
                run_mean=draw(ch, sc=0.1) + 1.0, run_var=draw(ch, sc=0.1).abs() + 0.5, gout=draw(n, 3))


def vn(inp, training, dtype, taps=None):
    b = _leaves([inp["x"], inp["o3"]] + inp["ws"], dtype)
    rm0, rv0 = inp["run_mean"].to(dtype), inp["run_var"].to(dtype)
    z = torch.cat((b[0].unsqueeze(1), b[1], inp["shape"].to(dtype)[inp["batch"]]), dim=1)
    pf = torch.einsum("oc,ncd->nod", b[2], z)
    nrm = torch.sqrt((pf * pf).sum(2)) + 1e-6
    if training:
        mean, var = nrm.mean(0), ((nrm - nrm.mean(0)) ** 2).mean(0)
    else:
        mean, var = rm0, rv0
    nbn = (nrm - mean) / torch.sqrt(var + 1e-5) * b[4] + b[5]
    p = pf / nrm.unsqueeze(2) * nbn.unsqueeze(2)
    d = torch.einsum("oc,ncd->nod", b[3], z)
    dot = (p * d).sum(2, keepdim=True)
    mask = (dot >= 0).to(dtype)
    out = (0.2 * p + 0.8 * (mask * p + (1 - mask) * (p - (dot / ((d * d).sum(2, keepdim=True) + 1e-6)) * d))).mean(dim=1)
    out.backward(inp["gout"].to(dtype))
    if taps is not None:
        taps.update(dot=_np(dot.squeeze(2)), p_norm=_np(p.norm(dim=2)), d_norm=_np(d.norm(dim=2)), pf_norm=_np(pf.norm(dim=2)))
    r = dict(zip(VN_OUT, [_np(out)] + [_np(t.grad) if t.grad is not None else np.zeros(tuple(t.shape)) for t in b]))
    if training:        # what nn.BatchNorm1d leaves behind: momentum 0.1, unbiased variance
        cnt = nrm.shape[0]
        r["run_mean"], r["run_var"] = _np(0.9 * rm0 + 0.1 * mean), _np(0.9 * rv0 + 0.1 * var * cnt / max(cnt - 1, 1))
    else:
        r["run_mean"], r["run_var"] = _np(rm0), _np(rv0)
    return r


# ------------------------------------------------------------------------------------------------------------------------
# well-posedness predicates (float64 taps alone): the number of offenders
# ------------------------------------------------------------------------------------------------------------------------
def relu_offenders(taps):
    xg, beta = taps["xhat_gamma"], taps["beta"][None, :]
    return int((np.abs(xg + beta) <= MASK_MARGIN * (np.abs(xg) + np.abs(beta))).sum())


def vn_offenders(taps):
    mask = int((np.abs(taps["dot"]) <= MASK_MARGIN * taps["p_norm"] * taps["d_norm"]).sum())
    small = int((taps["pf_norm"] < NORM_FLOOR * taps["pf_norm"].mean(0, keepdims=True)).sum())
    return mask + small


# ------------------------------------------------------------------------------------------------------------------------
# one case: inputs, both oracles, offenders (cached: the gate test and the C-ABI tests share one evaluation, nobody writes to it)
# ------------------------------------------------------------------------------------------------------------------------
def _evaluate(kind, case, inp, dtype, taps=None):
    if kind == "mlp":
        return mlp(inp, dtype, taps)
    if kind == "edge":
        return edge_mlp(inp, dtype, taps)
    if kind == "attn":
        return seg_attention(inp, case.heads, dtype, taps)
    return vn(inp, case.training, dtype, taps)


INPUTS = {"mlp": mlp_inputs, "edge": edge_inputs, "attn": attn_inputs, "vn": vn_inputs}


def offenders(kind, case, inp=None):
    taps = {}
    _evaluate(kind, case, inp if inp is not None else INPUTS[kind](case), F64, taps)
    return 0 if kind == "attn" else vn_offenders(taps) if kind == "vn" else relu_offenders(taps)


@functools.lru_cache(maxsize=None)
def evaluate(kind, case):
    """(inputs, r32, r64, offenders, taps) of a case of tests/train_ops_cases.py."""
    inp, taps = INPUTS[kind](case), {}
    r64 = _evaluate(kind, case, inp, F64, taps)
    r32 = _evaluate(kind, case, inp, F32)
    bad = 0 if kind == "attn" else vn_offenders(taps) if kind == "vn" else relu_offenders(taps)
    return inp, r32, r64, bad, taps


def find_seed(kind, case, tries=400):
    """The first seed from the case's own onwards with zero offenders (the CPU search behind the seeds of the cases file)."""
    for seed in range(case.seed, case.seed + tries):
        c = case._replace(seed=seed)
        if offenders(kind, c) == 0:
            return seed
    raise RuntimeError(f"no well-posed seed within {tries} of {case}")


# ------------------------------------------------------------------------------------------------------------------------
# the gate
# ------------------------------------------------------------------------------------------------------------------------
def gate(res, r32, r64, skip=()):
    """{tensor: (eH, e32, bound(e32), eH <= bound)} for every tensor of the float64 result (tensors without entries -- the
    gradient of an operand of zero rows or columns -- and those named in skip are left out; res may hold torch tensors or
    arrays)."""
    out = {}
    for key, ref in r64.items():
        if ref.size == 0 or key in skip:
            continue
        got = res[key].detach().cpu().numpy() if hasattr(res[key], "detach") else np.asarray(res[key])
        assert got.shape == ref.shape, (key, got.shape, ref.shape)
        eh, e32 = rel_err(got, ref), rel_err(r32[key], ref)
        if not np.isfinite(got).all():
            eh = float("inf")
        out[key] = (eh, e32, bound(e32), eh <= bound(e32))
    return out


def worst(gates):
    """(tensor, eH / bound) of the tensor closest to (or furthest beyond) its bound."""
    key = max(gates, key=lambda k: gates[k][0] / gates[k][2])
    return key, gates[key][0] / gates[key][2]


def report(name, gates):
    """Print the per-tensor table of a gate; True when every tensor passed."""
    for key, (eh, e32, b, ok) in gates.items():
        print(f"{name:40s} {key:9s} eH {eh:9.3e}  e32 {e32:9.3e}  bound {b:9.3e}  {'ok' if ok else 'FAIL'}")
    return all(g[3] for g in gates.values())


if __name__ == "__main__":      # the seed search: prints the cases whose seed has offenders, with the next seed that has none
    import train_ops_cases as TC
    for kind_, cases_ in TC.ALL.items():
        for case_ in cases_:
            if kind_ != "attn" and offenders(kind_, case_) != 0:
                print(kind_, case_[:-1], "->", find_seed(kind_, case_))
