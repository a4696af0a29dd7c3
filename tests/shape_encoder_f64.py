"""Float64 recompositions of the frozen shape encoder, one per stage (torch CPU; no GPU) -- TEST INFRASTRUCTURE.

Every recomposition takes the INPUT of one stage and the neighbour lists that go with it, evaluates that stage alone, and is
compared with the stage's output.  On the GPU (tests/test_gpu_shape_encoder.py) the inputs, the neighbour lists and the outputs
are the device's own workspace buffers (shapemol_se_debug_read, with shapemol_se_debug_stop_after(l) to see the buffers that
every block overwrites), so a neighbour that differs from the reference's never enters a value gate; on the CPU
(tests/test_shape_encoder_cpu.py) they are the intermediates of a float32 evaluation in the device's formulation whose latent
is pinned to oracle/shape_encoder_oracle.py.

Stages (csrc/sm_shape.h): kNN (validity only: `check_knn`), point linear `y = W' h`, edge stage (batch statistics, VN batch-norm,
VN leaky-ReLU, mean over k) for conv_pos and for a block, head (conv_c products, statistics, shared direction, mean over points).

Value gate (`gate`): with e32 the error of the same stage evaluated in float32 on the same inputs and eH the device's, both
against float64 and normalised by the largest entry of the float64 output, eH <= 4 e32 + 16 * 2^-24 -- the rule of
tests/precision.py for the main path: another but correct summation order may cost a small factor, a wrong operand costs orders
of magnitude.

Run as a script to rewrite profiles/shape_encoder/f32_stage_errors.json (the float32 errors per stage and shape, CPU only).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import shape_encoder_oracle as SE  # noqa: E402
from shapemol_amd import synth  # noqa: E402

U = 2.0 ** -24          # float32 unit roundoff
K = 20
EPS = 1e-6
CAP = 1e-3              # largest share of a stage's elements that may be left out of its value gate
F32, F64 = torch.float32, torch.float64

# (B, N, layer_num, latent_dim) of the stage gates; None stands for the largest N the library accepts on the device
# (2560 with 160 KiB of LDS per workgroup)
SHAPES = ((1, 32, 4, 32), (5, 48, 1, 7), (3, 512, 4, 32), (2, 80, 8, 256), (1, None, 2, 32))
WEIGHT_SEED = 17        # the golden fixture's


def T(a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def state_dict(layer_num, latent_dim, seed=WEIGHT_SEED):
    return {k: torch.from_numpy(v) for k, v in synth.shape_encoder_state_dict(128, latent_dim, layer_num, seed).items()}


def clouds(B, N, seed):
    """Random clouds scaled like the golden fixture's (anisotropic normal blobs), float32 (B, N, 3)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B, N, 3), generator=g, dtype=F32) * torch.tensor([1.5, 1.0, 0.6])).contiguous()


def rotated_copies(B, N, seed):
    """(B, N, 3): one random cloud and B - 1 random rotations of it.  A vector-neuron network turns the features with the cloud, so
    every copy has the first cloud's kNN margins, and the pooled batch statistics are those of one cloud: the way to a batch of
    several shapes whose every kNN has a safe margin (of 18000 seeded batches of five independent 48-point clouds none had one;
    one cloud in a hundred has)."""
    g = torch.Generator().manual_seed(seed + 1)
    x = clouds(1, N, seed).double()
    out = [x]
    for _ in range(B - 1):
        q, r = torch.linalg.qr(torch.randn((3, 3), generator=g, dtype=F64))
        q = q * torch.sign(torch.diagonal(r))
        out.append(x @ (q * torch.linalg.det(q)).t())
    return torch.cat(out).float().contiguous()


# ---- kNN ---------------------------------------------------------------------------------------------------------------
def d2_and_slack(feat):
    """feat (N, D) float32 features of one shape -> (d2, slack), both (N, N) float64.

    d2 is the squared distance in float64.  slack bounds the error of the device's float32 value of d2[i, j]:
      D > 3 (se_knn_kernel<384>): fl(xx_i + xx_j - 2 dot).  xx_i (se_sqnorm_kernel) is a sum of D squares, relative error below
        (D/64 + 7) u; dot is a sum of D products whose absolute values sum to at most |x_i| |x_j| <= (xx_i + xx_j) / 2
        (Cauchy-Schwarz, then AM-GM), so 2 dot carries at most D u (xx_i + xx_j) whatever the order of summation; two more
        roundings for the final add and subtract.  Together below (D + 4) u * 2 (xx_i + xx_j), the bound used here (twice what the
        count above needs).
      D == 3 (se_knn_kernel<3>): direct differences.  fl(x_i - x_j) is within u relative, its square within 3 u, the sum of three
        non-negative terms within 5 u: 8 u d2 is used.
    """
    x = T(feat, F64)
    D = x.shape[1]
    if D == 3:
        d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
        return d2, 8 * U * d2
    xx = (x * x).sum(1)
    d2 = ((xx[:, None] + xx[None, :]) - 2 * (x @ x.t())).clamp_min(0)
    # float64's own cancellation error (1e-16 (xx_i + xx_j)) is eight orders below the slack
    return d2, (D + 4) * U * 2 * (xx[:, None] + xx[None, :])


def knn_problems(feat, idx, k=K):
    """feat (B, N, D), idx (B, N, k) -> list of strings, empty when every row of idx is a valid ordered k-nearest set of the
    float64 distances within the slack of `d2_and_slack`:
      * k distinct indices in [0, N);
      * the point itself whenever its self-distance is the unique minimum within the slack;
      * max over the chosen of (d2 - slack) <= min over the others of (d2 + slack);
      * ascending: no earlier entry is farther than a later one by more than their two slacks."""
    feat, idx = T(feat), T(idx).long()
    B, N, _ = feat.shape
    out = []
    if tuple(idx.shape) != (B, N, k):
        return [f"idx has shape {tuple(idx.shape)}, expected {(B, N, k)}"]
    if int(idx.min()) < 0 or int(idx.max()) >= N:
        return [f"index out of range [0, {N}): min {int(idx.min())}, max {int(idx.max())}"]
    srt = idx.sort(-1)[0]
    dup = (srt[..., 1:] == srt[..., :-1]).any(-1)
    if dup.any():
        b, i = [int(v[0]) for v in torch.nonzero(dup, as_tuple=True)]
        return [f"shape {b} row {i}: duplicate neighbour in {idx[b, i].tolist()}"]
    for b in range(B):
        d2, s = d2_and_slack(feat[b])
        lo, hi = d2 - s, d2 + s
        chosen = torch.zeros((N, N), dtype=torch.bool)
        chosen.scatter_(1, idx[b], True)
        inf = torch.tensor(float("inf"), dtype=F64)
        worst_in = torch.where(chosen, lo, -inf).max(1)[0]
        best_out = torch.where(chosen, inf, hi).min(1)[0]
        bad = worst_in > best_out
        if bad.any():
            i = int(torch.nonzero(bad)[0])
            out.append(f"shape {b} row {i}: not a {k}-nearest set: a chosen neighbour at d2 {float(torch.where(chosen, d2, -inf)[i].max()):.9g}, "
                       f"a point left out at {float(torch.where(chosen, inf, d2)[i].min()):.9g} ({int(bad.sum())} such rows)")
        eye = torch.eye(N, dtype=torch.bool)
        self_first = hi.diagonal() < torch.where(eye, inf, lo).min(1)[0]
        miss = self_first & ~chosen.diagonal()
        if miss.any():
            out.append(f"shape {b} row {int(torch.nonzero(miss)[0])}: the point itself is the unique nearest and is not listed")
        lo_c, hi_c = lo.gather(1, idx[b]), hi.gather(1, idx[b])
        order = torch.cummax(lo_c, 1)[0][:, :-1] > hi_c[:, 1:]
        if order.any():
            i = int(torch.nonzero(order.any(1))[0])
            out.append(f"shape {b} row {i}: not ascending: d2 {d2.gather(1, idx[b])[i].tolist()}")
    return out


def knn_margin(feat, k=K):
    """Least over the rows of (d2 of the (k+1)-th nearest - d2 of the k-th) / (the larger of their two slacks), in float64: at
    4 and above no float32 evaluation within the slack can choose another SET of neighbours."""
    feat = T(feat)
    worst = float("inf")
    for b in range(feat.shape[0]):
        d2, s = d2_and_slack(feat[b])
        v, o = d2.sort(1)
        gap = v[:, k] - v[:, k - 1]
        sl = torch.maximum(s.gather(1, o[:, k - 1:k]), s.gather(1, o[:, k:k + 1]))[:, 0]
        worst = min(worst, float((gap / sl.clamp_min(1e-300)).min()))
    return worst


# ---- stages, in the arithmetic of `dtype` ---------------------------------------------------------------------------
def w_prime(wf, wd, dtype):
    """[Wf1 ; Wf2 - Wf1 ; Wd1 ; Wd2 - Wd1] (4C, C) from a block's map_to_feat / map_to_dir weights (C, 2C)."""
    wf, wd = T(wf, dtype), T(wd, dtype)
    C = wf.shape[0]
    return torch.cat([wf[:, :C], wf[:, C:] - wf[:, :C], wd[:, :C], wd[:, C:] - wd[:, :C]], 0)


def point_linear(h, wf, wd, dtype):
    """h (P, C, 3) -> y (P, 4C, 3) = W' h."""
    return torch.einsum("mc,pcx->pmx", w_prime(wf, wd, dtype), T(h, dtype))


def _global_idx(idx, N):
    idx = T(idx).long()
    P = idx.shape[0]
    return idx + (torch.arange(P) // N * N)[:, None]


def edge_pd_block(y, idx, N, dtype, rows=None):
    """p, d (R, k, C, 3) of the edges of `rows` from y (P, 4C, 3) = [Yf1 | Yf2 | Yd1 | Yd2]: p = Yf1[j] + Yf2[i], d = Yd1[j] + Yd2[i]."""
    y, j = T(y, dtype), _global_idx(idx, N)
    C = y.shape[1] // 4
    r = torch.arange(y.shape[0]) if rows is None else rows
    yj, yi = y[j[r]], y[r][:, None]
    return yj[:, :, :C] + yi[:, :, C:2 * C], yj[:, :, 2 * C:3 * C] + yi[:, :, 3 * C:]


def edge_pd_pos(x, idx, N, wf, wd, dtype, rows=None):
    """p, d (R, k, C, 3) of conv_pos from the points x (P, 3) and the (C, 2) weights: w[:, 0] (x_j - x_i) + w[:, 1] x_i."""
    x, j, wf, wd = T(x, dtype), _global_idx(idx, N), T(wf, dtype), T(wd, dtype)
    r = torch.arange(x.shape[0]) if rows is None else rows
    xi = x[r][:, None, None, :]
    dx = x[j[r]][:, :, None, :] - xi
    mk = lambda w: w[:, 0][None, None, :, None] * dx + w[:, 1][None, None, :, None] * xi      # noqa: E731
    return mk(wf), mk(wd)


def _norm_stats(p):
    """norm (..., C) = |p| + EPS over the last axis, and its batch mean / biased variance per channel."""
    norm = p.norm(dim=-1) + EPS
    flat = norm.reshape(-1, norm.shape[-1])
    return norm, flat.mean(0), flat.var(0, unbiased=False)


def _bn_lrelu(p, d, norm, mean, var, g, b):
    """VN batch-norm of p with the given statistics, then VN leaky-ReLU (slope 0.2) against d.  Also the mask of the elements whose
    float64 |dot| lies under the float32 rounding bound of that three-term dot product (3 u sum |q_k d_k|): the branch dot >= 0
    may go either way there."""
    nbn = (norm - mean) / torch.sqrt(var + 1e-5) * g + b
    q = p / norm.unsqueeze(-1) * nbn.unsqueeze(-1)
    dot = (q * d).sum(-1, keepdim=True)
    dsq = (d * d).sum(-1, keepdim=True)
    out = 0.2 * q + 0.8 * torch.where(dot >= 0, q, q - dot / (dsq + EPS) * d)
    unsure = dot.abs() < 3 * U * (q * d).abs().sum(-1, keepdim=True)
    return out, unsure[..., 0]


def edge_stage(pd_fn, g, b, dtype, rows=None):
    """Batch statistics over ALL edges, then batch-norm, leaky-ReLU and the mean over k for `rows` -> (h (R, C, 3), unsure (R, C, 3)).
    pd_fn(rows) returns p, d (R, k, C, 3) in `dtype`."""
    p, d = pd_fn(None)
    norm, mean, var = _norm_stats(p)
    if rows is not None:
        p, d = pd_fn(rows)
        norm = p.norm(dim=-1) + EPS
    out, unsure = _bn_lrelu(p, d, norm, mean, var, T(g, dtype), T(b, dtype))
    return out.mean(1), unsure.any(1)[..., None].expand(-1, -1, 3)


def head_linear(hcat, wf, wd, dtype):
    """hcat (P, KC, 3) -> pd (P, LAT + 1, 3): conv_c's map_to_feat rows, then the shared direction."""
    return torch.einsum("mc,pcx->pmx", torch.cat([T(wf, dtype), T(wd, dtype).reshape(1, -1)], 0), T(hcat, dtype))


def head_stage(hcat, wf, wd, g, b, B, dtype):
    """hcat (P, KC, 3) -> (pd (P, LAT + 1, 3), latent (B, LAT, 3)).  No element is left out here: each latent averages N points, and
    the leaky-ReLU is continuous at dot = 0."""
    pd = head_linear(hcat, wf, wd, dtype)
    p, d = pd[:, :-1], pd[:, -1:]
    norm, mean, var = _norm_stats(p)
    out, _ = _bn_lrelu(p, d, norm, mean, var, T(g, dtype), T(b, dtype))
    return pd, out.reshape(B, -1, *out.shape[1:]).mean(1)


# ---- the gate --------------------------------------------------------------------------------------------------------
def gate(dev, r32, r64, unsure=None):
    """(eH, e32, ok): errors of the device's and the float32 evaluation's output against float64, over the elements not in
    `unsure`, normalised by the largest float64 entry; ok = eH <= 4 e32 + 16 u.  Asserts that at most CAP of the elements are left out."""
    dev, r32, r64 = T(dev, F64), T(r32, F64), T(r64, F64)
    assert dev.shape == r64.shape == r32.shape, (dev.shape, r32.shape, r64.shape)
    keep = torch.ones_like(r64, dtype=torch.bool) if unsure is None else ~unsure
    left_out = 1.0 - float(keep.double().mean())
    assert left_out <= CAP, f"{left_out:.2e} of the stage's elements are left out of the value gate (cap {CAP})"
    s = float(r64.abs().max())
    eh = float(((dev - r64).abs() * keep).max()) / s
    e32 = float(((r32 - r64).abs() * keep).max()) / s
    return eh, e32, bool(np.isfinite(eh) and eh <= 4 * e32 + 16 * U)


def subsample(P, most=1024):
    """Rows of the edge-stage value gate: all of them up to `most`, else `most` evenly spread ones (first and last included)."""
    return None if P <= most else torch.linspace(0, P - 1, most).round().long().unique()


class Stages:
    """The stage gates of one configuration over a set of buffers.

    buffers(l) -> dict of the buffers after `l` blocks (l = 0: after conv_pos): idx (P, k), h0 (P, C, 3), hcat (P, L, C, 3) and, for
    l >= 1, y (P, 4C, 3) and xx (P,) of block l - 1; final() -> dict(hcat, pd, out (B, LAT, 3)).  `mutate(name, tensors)` may alter the
    weights a recomposition uses (the CPU test's negative cases)."""

    def __init__(self, sd, points, layer_num):
        self.sd, self.L = sd, layer_num
        self.x = T(points, F32)
        self.B, self.N = self.x.shape[:2]
        self.P = self.B * self.N
        self.rows = subsample(self.P)

    def _sel(self, a):
        return T(a) if self.rows is None else T(a)[self.rows]

    def knn(self, l, buf, prev):
        """kNN of conv_pos (l = 0, on the points) or of block l - 1 (on its input features)."""
        feat = self.x if l == 0 else self.block_input(l - 1, buf, prev).reshape(self.B, self.N, -1)
        return knn_problems(feat, T(buf["idx"]).reshape(self.B, self.N, K))

    def block_input(self, i, buf, prev):
        return T(buf["h0"]) if i == 0 else T(buf["hcat"])[:, i - 1]

    def conv_pos(self, buf):
        """-> {"conv_pos": (eH, e32, ok)}"""
        sd, x = self.sd, self.x.reshape(-1, 3)
        ev = lambda dt: edge_stage(lambda r: edge_pd_pos(x, buf["idx"], self.N, sd["conv_pos.map_to_feat.weight"], sd["conv_pos.map_to_dir.weight"], dt, r),  # noqa: E731
                                   sd["conv_pos.batchnorm.bn.weight"], sd["conv_pos.batchnorm.bn.bias"], dt, self.rows)
        (r64, unsure), (r32, _) = ev(F64), ev(F32)
        return {"conv_pos": gate(self._sel(buf["h0"]), r32, r64, unsure)}

    def block(self, i, buf, sd=None):
        """Block i from the buffers after i + 1 blocks -> {"linear{i}": ..., "edge{i}": ..., "xx{i}": ...}"""
        sd = sd or self.sd
        p = f"blocks.{i}"
        hin = self.block_input(i, buf, None)
        wf, wd = sd[p + ".map_to_feat.weight"], sd[p + ".map_to_dir.weight"]
        res = {f"linear{i}": gate(buf["y"], point_linear(hin, wf, wd, F32), point_linear(hin, wf, wd, F64))}
        xx = lambda dt: (T(hin, dt).reshape(self.P, -1) ** 2).sum(1)      # noqa: E731
        res[f"xx{i}"] = gate(buf["xx"], xx(F32), xx(F64))
        ev = lambda dt: edge_stage(lambda r: edge_pd_block(buf["y"], buf["idx"], self.N, dt, r), sd[p + ".batchnorm.bn.weight"],  # noqa: E731
                                   sd[p + ".batchnorm.bn.bias"], dt, self.rows)
        (r64, unsure), (r32, _) = ev(F64), ev(F32)
        res[f"edge{i}"] = gate(self._sel(T(buf["hcat"])[:, i]), r32, r64, unsure)
        return res

    def head(self, fin, sd=None):
        sd = sd or self.sd
        hcat = T(fin["hcat"]).reshape(self.P, -1, 3)
        ev = lambda dt: head_stage(hcat, sd["conv_c.map_to_feat.weight"], sd["conv_c.map_to_dir.weight"], sd["conv_c.batchnorm.bn.weight"],  # noqa: E731
                                   sd["conv_c.batchnorm.bn.bias"], self.B, dt)
        (pd64, z64), (pd32, z32) = ev(F64), ev(F32)
        return {"head_linear": gate(fin["pd"], pd32, pd64), "head": gate(fin["out"], z32, z64)}


# ---- a float32 (or float64) evaluation in the device's formulation, with every buffer kept ---------------------------------
@torch.no_grad()
def forward(sd, points, layer_num, dtype=F32, k=K, idx_from=None):
    """-> dict(stops=[buffers after l blocks, l = 0 .. L], final=dict(hcat, pd, out), feats=[kNN input of conv_pos and of each
    block, (B, N, D)]).  The neighbours are the oracle's own `_knn` (topk of -d2 in the reference's arithmetic) on this
    evaluation's features, or those of the evaluation `idx_from` (to compare two precisions on one graph)."""
    x = T(points, dtype)
    B, N, _ = x.shape
    P = B * N
    knn = lambda l, f: SE._knn(f.transpose(1, 2), k).reshape(P, k) if idx_from is None else idx_from["stops"][l]["idx"]      # noqa: E731
    idx = knn(0, x)
    g = lambda p: (sd[p + ".batchnorm.bn.weight"], sd[p + ".batchnorm.bn.bias"])      # noqa: E731
    h0, _ = edge_stage(lambda r: edge_pd_pos(x.reshape(P, 3), idx, N, sd["conv_pos.map_to_feat.weight"], sd["conv_pos.map_to_dir.weight"], dtype, r),
                       *g("conv_pos"), dtype)
    hcat = torch.zeros((P, layer_num, h0.shape[1], 3), dtype=dtype)
    stops, feats = [dict(idx=idx, h0=h0, hcat=hcat.clone())], [x]
    h = h0
    for i in range(layer_num):
        feats.append(h.reshape(B, N, -1))
        idx = knn(i + 1, h.reshape(B, N, -1))
        y = point_linear(h, sd[f"blocks.{i}.map_to_feat.weight"], sd[f"blocks.{i}.map_to_dir.weight"], dtype)
        h, _ = edge_stage(lambda r: edge_pd_block(y, idx, N, dtype, r), *g(f"blocks.{i}"), dtype)
        hcat[:, i] = h
        stops.append(dict(idx=idx, h0=h0, hcat=hcat.clone(), y=y, xx=(h0 if i == 0 else hcat[:, i - 1]).reshape(P, -1).pow(2).sum(1)))
    pd, out = head_stage(hcat.reshape(P, -1, 3), sd["conv_c.map_to_feat.weight"], sd["conv_c.map_to_dir.weight"], *g("conv_c"), B, dtype)
    return dict(stops=stops, final=dict(hcat=hcat, pd=pd, out=out), feats=feats)


def all_gates(sd, points, layer_num, stops, final):
    """Every kNN check and value gate of one configuration -> (problems [str], {stage: (eH, e32, ok)})."""
    st = Stages(sd, points, layer_num)
    problems, gates = [], {}
    for l, buf in enumerate(stops):
        problems += [f"kNN of {'conv_pos' if l == 0 else f'block {l - 1}'}: {m}" for m in st.knn(l, buf, None)]
        gates.update(st.conv_pos(buf) if l == 0 else st.block(l - 1, buf))
    gates.update(st.head(final))
    return problems, gates


def least_margin(feats):
    return min(knn_margin(f) for f in feats)


def f32_latent_error(sd, points, layer_num):
    """(e32, latent64): error of the whole float32 evaluation's latent against float64 on the same neighbour lists, normalised by the
    largest float64 entry -- what two correct float32 evaluations of one input may differ by, up to the factor of `gate`."""
    f32 = forward(sd, points, layer_num, F32)
    z64 = forward(sd, points, layer_num, F64, idx_from=f32)["final"]["out"]
    return float((f32["final"]["out"].double() - z64).abs().max() / z64.abs().max()), z64


def main():
    """profiles/shape_encoder/f32_stage_errors.json: per shape and stage, the float32 error against float64 on the float32
    evaluation's own intermediates (what `gate` scales the device's allowance by), the share of elements left out, the kNN margin."""
    res = []
    for (B, N, L, LAT) in SHAPES:
        N = N or 2560
        sd = state_dict(L, LAT)
        pts = T(np.load(os.path.join(ROOT, "tests", "golden", "shape_encoder.npz"))["points"]) if (B, N) == (3, 512) else clouds(B, N, 1000 + N)
        f = forward(sd, pts, L)
        problems, gates = all_gates(sd, pts, L, f["stops"], f["final"])
        assert not problems, problems
        res.append(dict(B=B, N=N, layer_num=L, latent_dim=LAT, knn_margin_over_slack=least_margin(f["feats"]),
                        e32={k: v[1] for k, v in gates.items()}))
        print(res[-1], flush=True)
    d = os.path.join(ROOT, "profiles", "shape_encoder")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "f32_stage_errors.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
