"""Classifier-free guidance, the parts that need no GPU: the restatement of threshold_CFG (tests/cfg_oracle.py) against the
reference's recorded calls, the quantile's rank rule against torch.quantile, the fixtures themselves, and the C ABI."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import cfg_oracle as O  # noqa: E402
from util import ROOT, golden  # noqa: E402

TYPES = ("none", "reference_threshold", "dynamic_threshold", "rescale")


def _calls(c):
    """The recorded threshold_CFG calls of a fixture: (x, cond, out) per call, positions then logits."""
    out, off = [], 0
    for size, cols in zip(c["call_sizes"], c["call_cols"]):
        sl = slice(off, off + int(size))
        out.append(tuple(torch.from_numpy(c[k][sl].reshape(-1, int(cols))) for k in ("call_x", "call_cond", "call_out")))
        off += int(size)
    return out


@pytest.mark.parametrize("tag", TYPES)
def test_restatement_matches_recorded_threshold_cfg(tag):
    """The device's formulation of threshold_CFG (float32) reproduces the reference's calls: bit for bit for the clip and
    clamp types, within float32 rounding of the ratio for rescale; the float64 form agrees to 1e-5."""
    c = golden(f"chain_cfg_{tag}.npz")
    ttype = None if tag == "none" else tag
    p = float(c["p"])
    args = {} if np.isnan(p) else {"p": p}
    box = c["bounds"][0]
    for k, (x, cond, out) in enumerate(_calls(c)):
        bounds = box if k == 0 else None
        got = O.threshold_cfg(x, cond, ttype, args, bounds)
        if tag == "rescale":
            assert float((got - out).abs().max()) <= 4e-6 * float(out.abs().max())
        else:
            assert torch.equal(got, out), float((got - out).abs().max())
        g64 = O.threshold_cfg(x, cond, ttype, args, bounds, dtype=torch.float64)
        assert float((g64 - out.double()).abs().max()) <= 1e-5


def test_restatement_unknown_type_raises():
    x = torch.zeros(3, 3)
    with pytest.raises(ValueError, match="undefined thresholding strategy"):
        O.threshold_cfg(x, x, "clip", {})


@pytest.mark.parametrize("n", [1, 2, 3, 10, 1001, 17157, 83000])
def test_quantile_rank_rule_equals_torch_quantile(n):
    """Selection of the two neighbouring order statistics with the float32 rank q * (n - 1) and torch.lerp's two fused
    branches equals torch.quantile bit for bit: distinct values, heavy duplicates, p at 0 and 1 and around half weights."""
    rng = np.random.default_rng(n)
    for dup in (False, True):
        x = rng.standard_normal(n).astype(np.float32) * 3
        if dup:
            x = np.round(x * 2) / 2
        t = torch.from_numpy(x)
        for p in (0.0, 1.0, 0.5, 0.995, 0.9, 0.1, 1 / 3, 0.7, 0.123456, 0.999999):
            assert O.quantile(t, p).item() == torch.quantile(t, p).item(), (n, dup, p)


def test_float64_rank_would_mismatch():
    """The float32 rank matters: a float64 rank q * (n - 1) picks different neighbours or weights for some (n, p)."""
    diff = 0
    for n in (1001, 17157, 83000, 333333):
        for p in (0.995, 0.9, 0.7, 0.123456):
            r32 = O.quantile_rank(n, p)
            r64 = p * (n - 1)
            diff += (r32[0] != int(r64)) or (abs(float(r32[2]) - (r64 - int(r64))) > 1e-9)
    assert diff > 0


@pytest.mark.parametrize("tag", TYPES)
def test_fixtures_show_guidance_biting(tag):
    """Every fixture clamps some atoms into the box of molecule 0; the clip types clip values; the unconditional predictions
    differ from the conditional ones; the box entries of the other molecules are wide (only bounds[0] is used)."""
    c = golden(f"chain_cfg_{tag}.npz")
    calls = _calls(c)
    box = c["bounds"][0]
    pos_out = calls[0][2].numpy()
    assert ((pos_out == box[:, 0].astype(np.float32)) | (pos_out == box[:, 1].astype(np.float32))).sum() > 0
    assert (np.abs(c["bounds"][1:]) >= 50).all()
    if tag in ("reference_threshold", "dynamic_threshold"):
        x, _, out = calls[1]
        assert int((x != out).sum()) > 0
    if tag == "rescale":
        x, _, out = calls[1]
        assert not torch.equal(x, out)
    assert np.abs(c["pos_cond_traj"] - c["pos_uncond_traj"]).max() > 1e-3
    assert np.abs(c["v_cond_traj"] - c["v_uncond_traj"]).max() > 1e-3


def test_c_abi_carries_set_cfg():
    """The header and _lib.EXPORTS gain shapemol_set_cfg together; the ABI version stays 5 and shapemol_traj keeps its six
    trajectories."""
    from shapemol_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "shapemol_hip.h")).read()
    assert re.search(r"\bint shapemol_set_cfg\(shapemol_ctx \*ctx, double guide_stren, int32_t threshold_type, double p,", hdr)
    assert "shapemol_set_cfg" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 5 and re.search(r"SHAPEMOL_ABI_VERSION\s+5", hdr)
    assert [f[0] for f in _lib.Traj._fields_] == ["pos_traj", "v_traj", "v0_traj", "vt_traj", "pos_cond_traj", "v_cond_traj"]
    assert _lib.CFG_THRESHOLDS == {None: 0, "reference_threshold": 1, "dynamic_threshold": 2, "rescale": 3}
