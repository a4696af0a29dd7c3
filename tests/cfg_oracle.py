"""Test-local restatement of classifier-free guidance (models/molopt_score_model.py:616-642, threshold_CFG :116-151) in the
form the device computes it (shapemol_amd/csrc/sm_cfg.h): the combine with the scalars rounded to the working precision
once, the quantile as an order-statistic selection with torch.quantile's float32 rank rule and torch.lerp's two-branch
fused multiply-add, the standard deviations from float64 sums.  ``dtype=torch.float64`` runs the same steps in float64."""
import math

import numpy as np
import torch

DEFAULT_P = {"reference_threshold": 1.1, "dynamic_threshold": 0.995, "rescale": 0.7}


def combine(cond, uncond, w, dtype=torch.float32):
    """(1 + w) * cond - w * uncond, the Python scalars rounded to `dtype` as torch's wrapped numbers are."""
    c, u = cond.to(dtype), uncond.to(dtype)
    return torch.tensor(1.0 + w, dtype=dtype) * c - torch.tensor(w, dtype=dtype) * u


def quantile_rank(n, p):
    """torch.quantile's linear-interpolation rank: q rounded to float32, q * (n - 1) in float32; the ranks below and above
    and the float32 weight rank - below."""
    r = np.float32(np.float32(p) * np.float32(n - 1))
    lo, hi = int(r), int(math.ceil(float(r)))
    return lo, hi, np.float32(r - np.float32(lo))


def _fma32(a, b, c):
    """float32 fused multiply-add (the float64 product of two float32 values is exact)."""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def lerp32(a, b, w):
    """torch.lerp in float32, both branches as fused multiply-adds (as compiled for the device)."""
    a, b, w = np.float32(a), np.float32(b), np.float32(w)
    d = np.float32(b - a)
    return _fma32(w, d, a) if abs(w) < 0.5 else _fma32(-d, np.float32(1.0) - w, b)


def quantile(x, p, dtype=torch.float32):
    """torch.quantile(x, p) over the flattened tensor by selection of the two neighbouring order statistics."""
    flat = x.reshape(-1).to(dtype)
    n = flat.numel()
    srt = torch.sort(flat).values
    if dtype == torch.float64:
        r = p * (n - 1)
        lo, hi = int(math.floor(r)), int(math.ceil(r))
        a, b, w = float(srt[lo]), float(srt[hi]), r - lo
        return torch.tensor(a + w * (b - a) if abs(w) < 0.5 else b - (b - a) * (1 - w), dtype=dtype)
    lo, hi, w = quantile_rank(n, p)
    return torch.tensor(lerp32(srt[lo].item(), srt[hi].item(), w), dtype=dtype)


def std64(x):
    """Unbiased standard deviation from float64 sums (one pass), as the device's statistic stage."""
    d = x.reshape(-1).to(torch.float64)
    n = d.numel()
    s, ss = d.sum(), (d * d).sum()
    return torch.sqrt(torch.clamp((ss - s * s / n) / (n - 1), min=0.0))


def statistic(x, cond, threshold_type, p, dtype=torch.float32):
    """The batch statistic of one tensor: the clip bound s, or the rescale ratio r, or None."""
    if threshold_type == "reference_threshold":
        return cond.to(dtype).abs().max() * torch.tensor(p, dtype=dtype)
    if threshold_type == "dynamic_threshold":
        return quantile(x, p, dtype)
    if threshold_type == "rescale":
        return std64(cond).to(dtype) / std64(x).to(dtype)
    if threshold_type is None:
        return None
    raise ValueError("undefined thresholding strategy: expect one of (reference_threshold, dynamic_threshold, rescale, none) "
                     + "but get %s" % (threshold_type))


def threshold_cfg(x, cond, threshold_type, threshold_args, bounds=None, dtype=torch.float32):
    """threshold_CFG(x, cond, threshold_type, threshold_args, bounds) of the reference in the device's formulation."""
    x = x.to(dtype)
    p = threshold_args.get("p", DEFAULT_P.get(threshold_type, 0.0))
    st = statistic(x, cond, threshold_type, p, dtype)
    if threshold_type in ("reference_threshold", "dynamic_threshold"):
        x = torch.minimum(torch.maximum(x, -st), st)
    elif threshold_type == "rescale":
        x = torch.tensor(p, dtype=dtype) * (x * st) + torch.tensor(1.0 - p, dtype=dtype) * x
    if bounds is not None:
        b = torch.as_tensor(bounds).to(device=x.device, dtype=dtype)
        x = torch.minimum(torch.maximum(x, b[:, 0]), b[:, 1])
    return x


def guided(pos_c, pos_u, v_c, v_u, w, threshold_type, threshold_args, box, dtype=torch.float32):
    """One step's combined and thresholded positions and logits (the reference's :627-636 with bounds = box)."""
    pos = threshold_cfg(combine(pos_c, pos_u, w, dtype), pos_c.to(dtype), threshold_type, threshold_args, box, dtype)
    v = threshold_cfg(combine(v_c, v_u, w, dtype), v_c.to(dtype), threshold_type, threshold_args, None, dtype)
    return pos, v
