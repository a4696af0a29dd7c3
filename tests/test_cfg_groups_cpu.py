"""Classifier-free guidance per group of molecules, the parts that need no GPU: the per-group restatement
(tests/cfg_groups_oracle.py) against the reference's recorded per-group threshold_CFG calls, the host planning of
sample_diffusion's list form and of the multi-condition driver, and the C ABI."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import cfg_groups_oracle as GO  # noqa: E402
from util import ROOT, golden  # noqa: E402

TYPES = ("none", "reference_threshold", "dynamic_threshold", "rescale")


def _calls(c):
    out, off = [], 0
    for size, cols in zip(c["call_sizes"], c["call_cols"]):
        sl = slice(off, off + int(size))
        out.append(tuple(torch.from_numpy(c[k][sl].reshape(-1, int(cols))) for k in ("call_x", "call_cond", "call_out")))
        off += int(size)
    return out


def _boxes(c):
    mol_off = np.concatenate([[0], np.cumsum(c["groups"])])
    return [c["bounds"][int(m)] for m in mol_off[:-1]]


@pytest.mark.parametrize("tag", TYPES)
def test_per_group_restatement_matches_recorded_calls(tag):
    """cfg_oracle's functions applied per slice reproduce the reference's threshold_CFG called once per group: bit for bit
    (rescale included: the per-group ratio is the same float32 value in both)."""
    c = golden(f"chain_cfg_groups_{tag}_b6_s20.npz")
    ttype = None if tag == "none" else tag
    p = float(c["p"])
    args = {} if np.isnan(p) else {"p": p}
    for k, (x, cond, out) in enumerate(_calls(c)):
        got = GO.threshold_cfg_groups(x, cond, c["atom_off"], ttype, args, _boxes(c) if k == 0 else None)
        assert torch.equal(got, out), (k, float((got - out).abs().max()))


@pytest.mark.parametrize("tag", TYPES)
def test_fixture_groups_differ_and_clamp(tag):
    """Groups 0 and 2 clamp atoms into their tight boxes, group 1's box is wide; the groups' statistics differ, and the
    whole-batch statistic is not any group's (a whole-batch kernel cannot pass the chain test)."""
    c = golden(f"chain_cfg_groups_{tag}_b6_s20.npz")
    assert list(c["groups"]) == [2, 3, 1] and int(c["B"]) == 6 and int(c["S"]) == 20
    x, cond, out = _calls(c)[0]
    ao, boxes = c["atom_off"], _boxes(c)
    hits = [int(((out[ao[g]:ao[g + 1]].numpy() == boxes[g][:, 0].astype(np.float32)) |
                 (out[ao[g]:ao[g + 1]].numpy() == boxes[g][:, 1].astype(np.float32))).sum()) for g in range(3)]
    assert hits[0] > 0 and hits[2] > 0 and hits[1] == 0
    if tag != "none":
        import cfg_oracle as O
        for x, cond, _ in _calls(c):
            st = [float(s) for s in GO.statistic_groups(x, cond, ao, tag, float(c["p"]))]
            whole = float(O.statistic(x, cond, tag, float(c["p"])))
            assert len(set(st)) == 3 and sum(s != whole for s in st) >= 2, (st, whole)


def test_cfg_groups_host_arrays():
    from shapemol_amd.guidance import _cfg_groups
    bounds = np.arange(6 * 6, dtype=np.float64).reshape(6, 3, 2)
    off, w, boxes = _cfg_groups([(0.7, 2), (1.5, 3), (0.0, 1)], bounds, 6)
    assert off.dtype == np.int64 and list(off) == [0, 2, 5, 6] and list(w) == [0.7, 1.5, 0.0]
    assert np.array_equal(boxes, bounds[[0, 2, 5]])
    off, w, boxes = _cfg_groups([(0.7, 2), (1.5, 0), (0.3, 4)], bounds, 6)       # an empty group: a NaN row
    assert np.isnan(boxes[1]).all() and np.array_equal(boxes[2], bounds[2])
    _, _, boxes = _cfg_groups([(0.7, 6)], np.array([[-1.0, 1.0]] * 3), 6)
    assert boxes.shape == (1, 3, 2)
    assert _cfg_groups([(0.7, 6)], None, 6)[2] is None
    with pytest.raises(ValueError, match="hold 5 molecules, the batch has 6"):
        _cfg_groups([(0.7, 2), (1.5, 3)], None, 6)
    with pytest.raises(ValueError, match="finite"):
        _cfg_groups([(float("nan"), 6)], None, 6)
    with pytest.raises(ValueError, match="at most 256"):
        _cfg_groups([(0.5, 1)] * 257, None, 257)
    with pytest.raises(ValueError, match=r"\(B, 3, 2\) or \(3, 2\)"):
        _cfg_groups([(0.7, 6)], np.zeros((5, 3, 2)), 6)


def test_driver_planning():
    """plan_cfg / cfg_groups of the multi-condition driver: per-condition values, the bounds of a batch, the two ValueErrors."""
    from shapemol_amd.sampling import cfg_groups, plan_batches, plan_cfg
    box0, box2 = np.array([[-1.0, 1.0]] * 3), np.array([[-2.0, 2.0]] * 3)
    strens, boxes = plan_cfg(None, [None] * 3, [0.7, 0, 1.5], [box0, None, box2], 3)
    assert strens == [0.7, 0.0, 1.5] and boxes[1] is None
    plan = plan_batches(3, 4, 6)
    kw = cfg_groups(strens, boxes, plan[0])
    assert kw["guide_stren"] == [(0.7, 4), (0.0, 2)] and kw["bounds"].shape == (6, 3, 2)
    assert np.array_equal(kw["bounds"][:4], np.stack([box0] * 4)) and np.isnan(kw["bounds"][4:]).all()
    kw = cfg_groups(strens, boxes, plan[1])
    assert kw["guide_stren"] == [(0.0, 2), (1.5, 4)] and np.array_equal(kw["bounds"][2:], np.stack([box2] * 4))
    assert plan_cfg(None, [None] * 3, 0.5, box0, 3)[0] == [0.5] * 3          # one value for all conditions
    assert cfg_groups(*plan_cfg(None, [None] * 3, 0.5, None, 3), plan[0])["bounds"] is None
    assert plan_cfg(None, [None] * 3, 0, None, 3) == (None, None) and cfg_groups(None, None, plan[0]) == {}
    with pytest.raises(ValueError, match="2 entries for 3 conditions"):
        plan_cfg(None, [None] * 3, [0.5, 0.5], None, 3)
    cloud = (np.zeros((8, 3)), None, 0.2)
    assert plan_cfg("cloud", [cloud, None, cloud], [0.7, 0, 1.5], None, 3) == (None, None)     # carried clouds: CFG ignored
    with pytest.raises(ValueError, match="condition 1 has guide_stren > 0 but no mesh or point cloud.*two jobs"):
        plan_cfg("cloud", [cloud, None, cloud], 0.7, None, 3)


def test_c_abi_carries_set_cfg_groups():
    from shapemol_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "shapemol_hip.h")).read()
    assert re.search(r"\bint shapemol_set_cfg_groups\(shapemol_ctx \*ctx, int32_t n_groups, const int64_t \*h_mol_off, "
                     r"const double \*h_guide_stren,\s+int32_t threshold_type, double p, const double \*h_bounds", hdr)
    assert "shapemol_set_cfg_groups" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 5 and re.search(r"SHAPEMOL_ABI_VERSION\s+5", hdr)
    src = open(os.path.join(ROOT, "shapemol_amd", "csrc", "sm_cfg.h")).read()
    assert re.search(r"kCfgMaxGroups = (\d+)", src).group(1) == str(_lib.CFG_MAX_GROUPS)
