"""The shape encoder's backward in torch (CPU; no GPU) -- TEST INFRASTRUCTURE.

Two evaluations of every parameter gradient of VN_DGCNN_Encoder for a fixed upstream gradient, with the neighbour lists GIVEN (no
gradient flows through them):

  * `device_form`: the formulas of DESIGN.md section 21 / csrc/sm_shape_train.h written out in torch, in float32 or float64 -- per-point
    products Y = W' h, the closed-form gradient of VN batch-norm + VN leaky-ReLU with the batch sums S1, S2, the scatter into dY, the
    two products dh_in = W'^T dY and dW' = dY h^T, the map back to map_to_feat / map_to_dir, conv_pos's direct sums, conv_c;
  * `reference_autograd`: the reference's own dense form (oracle/shape_encoder_oracle.py: edge features [x_j - x_i | x_i], one Linear
    over 2C channels) under torch autograd.

`wellposed` measures what makes a case a fair comparison of float32 against float64: both precisions choose the same neighbour lists
at every stage and the same leaky-ReLU branch at every element, and the least |dot| / (|q| |d|) is at least 100 times the largest
float32-vs-float64 difference of that quantity.  It is a condition on the inputs, not a tolerance.

    python tests/shape_encoder_train_f64.py [--search]

rewrites profiles/shape_encoder_train/wellposed.json (`--search` walks the cloud seeds of every case first and prints what it finds).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import shape_encoder_f64 as F  # noqa: E402
from shape_encoder_f64 import F32, F64, K, EPS, T, ROOT  # noqa: E402
from oracle import shape_encoder_oracle as SE  # noqa: E402

# (B, N, layer_num, latent_dim) -> cloud seed (see `--search`); the cases of tests/test_gpu_shape_encoder_train.py, on the weights of
# `state_dict` (directions aligned with the features: the only way to the cosine margin, see there)
CASES = {(1, 32, 1, 7): 1, (3, 48, 2, 32): 1, (2, 32, 8, 256): 1, (2, 512, 4, 32): 1}
# the same on the plain hash weights of shape_encoder_f64.state_dict, for the cases in which float32 and float64 still choose the same
# lists and branches (checked on the CPU); no cosine margin exists there
GENERIC = {(1, 32, 1, 7): 15, (3, 48, 2, 32): 38}
# all four cases on the hash weights, gated with the float64 and float32 references forced onto the branches the DEVICE took (its
# backward reports them): a branch that float32 and float64 choose differently then drops out of the comparison
HASH = {(1, 32, 1, 7): 15, (3, 48, 2, 32): 38, (2, 32, 8, 256): 2, (2, 512, 4, 32): 7}
UP_SEED = 4242
ALIGN_EPS = 1e-3


def state_dict(L, LAT, kind="aligned"):
    """The weights of a case.  'generic': the hash weights of shape_encoder_f64.state_dict.  'aligned': the same, with
      * every map_to_dir = +-map_to_feat (even output channels +, odd -) + ALIGN_EPS x its hash weights, so d = +-p up to 1e-3 and
        |cos(q, d)| stays near 1: even channels take the branch dot >= 0 at every edge, odd channels the other one;
      * conv_c, whose direction is shared by all rows: map_to_feat row m = +-(0.5 + m / latent) x map_to_dir + ALIGN_EPS x its hash weights;
      * batch-norm weight in [0.05, 0.1] and bias in [0.9, 1.1], so s = gamma xh + beta stays positive and q keeps p's direction.
    Why: the cosines of hash weights spread over [-1, 1], and the least of the 1.6e5 .. 1.3e7 cosines of a case is then 1e-5 and below,
    under the float32-vs-float64 difference of that cosine (3e-5 and more); no cloud seed changes that (wellposed.json, 'generic')."""
    sd = F.state_dict(L, LAT)
    if kind == "generic":
        return sd
    assert kind == "aligned"
    sd = {k: v.clone() for k, v in sd.items()}
    for pre in ["conv_pos", *[f"blocks.{i}" for i in range(L)]]:
        wf = sd[pre + ".map_to_feat.weight"]
        sgn = torch.where(torch.arange(wf.shape[0]) % 2 == 0, 1.0, -1.0)[:, None]
        sd[pre + ".map_to_dir.weight"] = (sgn * wf + ALIGN_EPS * sd[pre + ".map_to_dir.weight"]).float()
    wd = sd["conv_c.map_to_dir.weight"].reshape(1, -1)
    m = torch.arange(LAT, dtype=F32)[:, None]
    sd["conv_c.map_to_feat.weight"] = (torch.where(m % 2 == 0, 1.0, -1.0) * (0.5 + m / LAT) * wd + ALIGN_EPS * sd["conv_c.map_to_feat.weight"]).float()
    for k in sd:
        c = torch.arange(sd[k].shape[0], dtype=F32)
        if k.endswith("bn.weight"):
            sd[k] = 0.05 + 0.05 * ((c * 37) % 11) / 11
        elif k.endswith("bn.bias"):
            sd[k] = 0.9 + 0.2 * ((c * 53) % 13) / 13
    return sd


def points(B, N, seed):
    """One random cloud (B = 1) or a cloud and B - 1 rotated copies of it (every copy has the first one's kNN margins)."""
    pts = F.clouds(1, N, seed) if B == 1 else F.rotated_copies(B, N, seed).reshape(B, N, 3)
    return pts.reshape(B, N, 3).contiguous()


def upstream(shape, seed=UP_SEED):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=F64)


def keys(L):
    return [f"{p}.{w}" for p in ["conv_pos", *[f"blocks.{i}" for i in range(L)], "conv_c"]
            for w in ("map_to_feat.weight", "batchnorm.bn.weight", "batchnorm.bn.bias", "map_to_dir.weight")]


def unflatten(flat, sd, L):
    """The flat gradient vector in the library's weight order -> {key: tensor}."""
    out, o = {}, 0
    for k in keys(L):
        n = sd[k].numel()
        out[k] = T(flat)[o:o + n].reshape(sd[k].shape)
        o += n
    assert o == T(flat).numel()
    return out


def as_lists(idx):
    """idx (L + 1, P, k) -> what shape_encoder_f64.forward takes as `idx_from`."""
    return {"stops": [{"idx": T(i).long()} for i in idx]}


# ---- device form ---------------------------------------------------------------------------------------------------------
def vn_backward(p, d, mean, var, gamma, beta, g_o, neg=None):
    """p, d, g_o broadcastable to (..., C, 3); statistics and affine (C,).  -> g_p, g_d, S1 (dbeta), S2 (dgamma), mask dot >= 0, cos.
    neg (..., C) bool: the branch dot < 0 is taken where it is set, whatever the sign of dot."""
    r = p.norm(dim=-1)
    n = r + EPS
    sig = torch.sqrt(var + 1e-5)
    xh = (n - mean) / sig
    s = gamma * xh + beta
    q = p * (s / n).unsqueeze(-1)
    d = d.expand_as(p)
    g_o = g_o.expand_as(p)
    dot = (q * d).sum(-1)
    D = (d * d).sum(-1) + EPS
    a = (g_o * d).sum(-1)
    neg = ((dot < 0) if neg is None else neg).unsqueeze(-1)
    u = lambda t: t.unsqueeze(-1)      # noqa: E731
    g_q = torch.where(neg, g_o - 0.8 * u(a / D) * d, g_o)
    g_d = torch.where(neg, -0.8 * (u(a / D) * q + u(dot / D) * g_o - 2 * u(a * dot / D ** 2) * d), torch.zeros_like(d))
    t = (g_q * p).sum(-1)
    g_s = t / n
    M = g_s.numel() // g_s.shape[-1]
    red = tuple(range(g_s.dim() - 1))
    S1, S2 = g_s.sum(red), (g_s * xh).sum(red)
    g_n = (gamma / sig) * (g_s - S1 / M - xh * S2 / M) - t * s / n ** 2
    g_p = g_q * u(s / n) + u(torch.where(r > 0, g_n / r, torch.zeros_like(r))) * p
    cos = dot / (q.norm(dim=-1) * d.norm(dim=-1)).clamp_min(1e-300)
    return g_p, g_d, S1, S2, ~neg[..., 0], cos


def device_masks(raw, L, LAT, C=128):
    """The backward's int32 branch record (L + 2, P, 256) -> {stage: neg}: (P, k, C) bool for conv_pos and the blocks, (P, LAT) for conv_c."""
    raw = T(raw).long()
    out = {}
    for i, name in enumerate(["conv_pos", *[f"blocks.{l}" for l in range(L)]]):
        out[name] = ((raw[i, :, :C, None] >> torch.arange(K)) & 1).bool().permute(0, 2, 1).contiguous()
    out["conv_c"] = raw[L + 1, :, :LAT].bool()
    return out


def device_form(sd, pts, L, idx, dtype, g_out=None, g_hcat=None, masks=None):
    """Every parameter gradient for the upstream gradient g_out (B, LAT, 3) of the latent -- or g_hcat (P, L, C, 3) at conv_c's input,
    conv_c skipped and its gradients zero -- in the arithmetic of `dtype`, on the neighbour lists idx (L + 1, P, k).
    -> (grads {key: tensor}, info dict(out, masks [per stage], cos [per stage], fwd))."""
    x = T(pts, dtype)
    B, N, _ = x.shape
    P = B * N
    f = F.forward(sd, x, L, dtype, idx_from=as_lists(idx))
    W = lambda k: T(sd[k], dtype)      # noqa: E731
    C = W("conv_pos.map_to_feat.weight").shape[0]
    h0, hcat = f["stops"][0]["h0"], f["final"]["hcat"]                      # (P, C, 3), (P, L, C, 3)
    forced = masks or {}
    grads, masks, coss = {}, {}, {}
    if g_hcat is None:
        pd = f["final"]["pd"]
        p, d = pd[:, :-1], pd[:, -1:]
        _, mean, var = F._norm_stats(p)
        g_o = (T(g_out, dtype) / N).repeat_interleave(N, 0)                   # (P, LAT, 3)
        g_p, g_d, S1, S2, masks["conv_c"], coss["conv_c"] = vn_backward(p, d, mean, var, W("conv_c.batchnorm.bn.weight"), W("conv_c.batchnorm.bn.bias"), g_o,
                                                                            forced.get("conv_c"))
        gd = g_d.sum(1)
        hc = hcat.reshape(P, -1, 3)
        wd = W("conv_c.map_to_dir.weight").reshape(-1)
        dhcat = (torch.einsum("mc,pmx->pcx", W("conv_c.map_to_feat.weight"), g_p) + wd[None, :, None] * gd[:, None, :]).reshape(P, L, C, 3)
        grads.update({"conv_c.map_to_feat.weight": torch.einsum("pmx,pcx->mc", g_p, hc), "conv_c.batchnorm.bn.weight": S2, "conv_c.batchnorm.bn.bias": S1,
                      "conv_c.map_to_dir.weight": torch.einsum("px,pcx->c", gd, hc).reshape(1, -1)})
    else:
        dhcat = T(g_hcat, dtype).clone()
        grads.update({k: torch.zeros_like(W(k)) for k in keys(L)[-4:]})
    dhcat = [dhcat[:, l].clone() for l in range(L)]
    dh0 = None
    for l in range(L - 1, -1, -1):
        pre = f"blocks.{l}"
        h = h0 if l == 0 else hcat[:, l - 1]
        il = f["stops"][l + 1]["idx"]
        y = f["stops"][l + 1]["y"]
        p, d = F.edge_pd_block(y, il, N, dtype)
        _, mean, var = F._norm_stats(p)
        g_o = (dhcat[l] / K)[:, None]
        g_p, g_d, S1, S2, masks[pre], coss[pre] = vn_backward(p, d, mean, var, W(pre + ".batchnorm.bn.weight"), W(pre + ".batchnorm.bn.bias"), g_o,
                                                                    forced.get(pre))
        j = F._global_idx(il, N).reshape(-1)
        dY = torch.zeros((P, 4 * C, 3), dtype=dtype)
        dY[:, C:2 * C] = g_p.sum(1)
        dY[:, 3 * C:] = g_d.sum(1)
        dY[:, :C].index_add_(0, j, g_p.reshape(-1, C, 3))
        dY[:, 2 * C:3 * C].index_add_(0, j, g_d.reshape(-1, C, 3))
        wp = F.w_prime(sd[pre + ".map_to_feat.weight"], sd[pre + ".map_to_dir.weight"], dtype)
        dh_in = torch.einsum("mc,pmx->pcx", wp, dY)
        dwp = torch.einsum("pmx,pcx->mc", dY, h)
        grads[pre + ".map_to_feat.weight"] = torch.cat([dwp[:C] - dwp[C:2 * C], dwp[C:2 * C]], 1)
        grads[pre + ".map_to_dir.weight"] = torch.cat([dwp[2 * C:3 * C] - dwp[3 * C:], dwp[3 * C:]], 1)
        grads[pre + ".batchnorm.bn.weight"], grads[pre + ".batchnorm.bn.bias"] = S2, S1
        if l == 0:
            dh0 = dh_in
        else:
            dhcat[l - 1] = dhcat[l - 1] + dh_in
    i0 = f["stops"][0]["idx"]
    xf = x.reshape(P, 3)
    p, d = F.edge_pd_pos(xf, i0, N, sd["conv_pos.map_to_feat.weight"], sd["conv_pos.map_to_dir.weight"], dtype)
    _, mean, var = F._norm_stats(p)
    g_p, g_d, S1, S2, masks["conv_pos"], coss["conv_pos"] = vn_backward(p, d, mean, var, W("conv_pos.batchnorm.bn.weight"), W("conv_pos.batchnorm.bn.bias"),
                                                                        (dh0 / K)[:, None], forced.get("conv_pos"))
    dx = xf[F._global_idx(i0, N)] - xf[:, None]
    two = lambda g: torch.stack([torch.einsum("pkcx,pkx->c", g, dx), torch.einsum("pkcx,px->c", g, xf)], 1)      # noqa: E731
    grads.update({"conv_pos.map_to_feat.weight": two(g_p), "conv_pos.map_to_dir.weight": two(g_d), "conv_pos.batchnorm.bn.weight": S2,
                  "conv_pos.batchnorm.bn.bias": S1})
    return grads, dict(out=f["final"]["out"], masks=masks, cos=coss, fwd=f)


# ---- the reference's form under autograd -------------------------------------------------------------------------------------
def _graph_feature(h, idx):
    """h (B, C, 3, N), idx (P, k) inside the shape -> (B, 2C, 3, N, k) = [x_j - x_i | x_i], as oracle._graph_feature with the lists given."""
    B, C, _, N = h.shape
    k = idx.shape[1]
    gi = F._global_idx(idx, N).reshape(-1)
    ptsf = h.reshape(B, C * 3, N).transpose(2, 1).reshape(B * N, C * 3)
    nb = ptsf[gi].view(B, N, k, C, 3)
    ctr = ptsf.view(B, N, 1, C, 3).expand(-1, -1, k, -1, -1)
    return torch.cat((nb - ctr, ctr), dim=3).permute(0, 3, 4, 1, 2).contiguous()


def _vn_linear_lrelu(sd, p, x, neg=None, slope=0.2):
    """oracle._vn_linear_lrelu; with `neg` (broadcastable to the dot product's shape) the branch is given, not chosen by dot's sign."""
    if neg is None:
        return SE._vn_linear_lrelu(sd, p, x, slope)
    lin = lambda w, t: torch.matmul(t.transpose(1, -1), w.t()).transpose(1, -1)   # noqa: E731
    q = lin(sd[p + ".map_to_feat.weight"], x)
    norm = torch.norm(q, dim=2) + EPS
    dims = [0] + list(range(2, norm.dim()))
    mean = norm.mean(dim=dims, keepdim=True)
    var = norm.var(dim=dims, unbiased=False, keepdim=True)
    shape = [1, -1] + [1] * (norm.dim() - 2)
    nbn = (norm - mean) / torch.sqrt(var + 1e-5) * sd[p + ".batchnorm.bn.weight"].view(shape) + sd[p + ".batchnorm.bn.bias"].view(shape)
    q = q / norm.unsqueeze(2) * nbn.unsqueeze(2)
    d = lin(sd[p + ".map_to_dir.weight"], x)
    dot = (q * d).sum(2, keepdim=True)
    mask = (~neg).to(q.dtype)
    dsq = (d * d).sum(2, keepdim=True)
    return slope * q + (1 - slope) * (mask * q + (1 - mask) * (q - (dot / (dsq + EPS)) * d))


def reference_autograd(sd, pts, L, idx, dtype=F64, g_out=None, g_hcat=None, masks=None):
    """-> ({key: gradient}, latent): torch autograd through the reference's dense form on the given neighbour lists; with `masks`
    ({stage: neg}, the layout of `device_masks`) on the given leaky-ReLU branches."""
    B_, N_ = T(pts).shape[:2]
    edge = lambda name: None if not masks else masks[name].reshape(B_, N_, K, -1).permute(0, 3, 1, 2).unsqueeze(2)      # noqa: E731  (B, C, 1, N, k)
    head = None if not masks else masks["conv_c"].reshape(B_, N_, -1).permute(0, 2, 1).unsqueeze(2)                      # (B, LAT, 1, N)
    w = {k: T(v, dtype).clone().requires_grad_(True) for k, v in sd.items() if k in set(keys(L))}
    x = T(pts, dtype)
    B, N, _ = x.shape
    h = _vn_linear_lrelu(w, "conv_pos", _graph_feature(x.unsqueeze(1).transpose(2, 3), T(idx[0])), edge("conv_pos")).mean(dim=-1)
    hs = []
    for i in range(L):
        h = _vn_linear_lrelu(w, f"blocks.{i}", _graph_feature(h, T(idx[i + 1])), edge(f"blocks.{i}")).mean(dim=-1)
        hs.append(h)
    hc = torch.cat(hs, dim=1)                                               # (B, L C, 3, N)
    out = _vn_linear_lrelu(w, "conv_c", hc, head).mean(dim=-1)
    if g_hcat is None:
        loss = (out * T(g_out, dtype)).sum()
    else:
        C = hs[0].shape[1]
        up = T(g_hcat, dtype).reshape(B, N, L, C, 3).permute(0, 2, 3, 4, 1).reshape(B, L * C, 3, N)
        loss = (hc * up).sum()
    ks = keys(L)
    gs = torch.autograd.grad(loss, [w[k] for k in ks], allow_unused=True)
    return {k: (torch.zeros_like(w[k]) if g is None else g) for k, g in zip(ks, gs)}, out.detach()


def rel(a, b):
    """Largest |a - b| over the largest |b|."""
    return float((T(a, F64) - T(b, F64)).abs().max() / T(b, F64).abs().max().clamp_min(1e-300))


# ---- well-posedness ------------------------------------------------------------------------------------------------------------
def wellposed(case, seed=None, kind="aligned"):
    """-> dict(same_lists, same_masks, least_cos, cos_diff, ratio, ok) of the case's float32 and float64 evaluations."""
    B, N, L, LAT = case
    seed = (CASES if kind == "aligned" else GENERIC)[case] if seed is None else seed
    sd, pts = state_dict(L, LAT, kind), points(B, N, seed)
    f32, f64 = F.forward(sd, pts, L, F32), F.forward(sd, pts, L, F64)
    srt = lambda f: [s["idx"].sort(-1)[0] for s in f["stops"]]      # noqa: E731
    same_lists = all(torch.equal(a, b) for a, b in zip(srt(f32), srt(f64)))
    res = dict(case=list(case), weights=kind, seed=seed, same_lists=bool(same_lists), same_masks=False, least_cos=0.0, cos_diff=float("inf"), ratio=0.0, ok=False)
    if not same_lists:
        return res
    idx = torch.stack([s["idx"] for s in f64["stops"]])
    up = upstream((B, LAT, 3))
    _, i32 = device_form(sd, pts, L, idx, F32, g_out=up)
    _, i64 = device_form(sd, pts, L, idx, F64, g_out=up)
    res["same_masks"] = bool(all(torch.equal(i32["masks"][k], i64["masks"][k]) for k in i64["masks"]))
    res["least_cos"] = min(float(c.abs().min()) for c in i64["cos"].values())
    res["cos_diff"] = max(float((i32["cos"][k].double() - i64["cos"][k]).abs().max()) for k in i64["cos"])
    res["ratio"] = res["least_cos"] / max(res["cos_diff"], 1e-300)
    res["ok"] = bool(res["same_masks"] and res["ratio"] >= 100.0)
    return res


def main():
    out = []
    for case in CASES:
        if "--search" in sys.argv:
            best = None
            for seed in range(1, int(os.environ.get("SEARCH_SEEDS", "400")) + 1):
                r = wellposed(case, seed)
                if best is None or r["ratio"] > best["ratio"]:
                    best = r
                if r["ok"]:
                    break
            print("search", case, "->", best, flush=True)
        out.append(wellposed(case))
        print(out[-1], flush=True)
    for case in GENERIC:
        out.append(wellposed(case, kind="generic"))
        print(out[-1], flush=True)
    d = os.path.join(ROOT, "profiles", "shape_encoder_train")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "wellposed.json"), "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
