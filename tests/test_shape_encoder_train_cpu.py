"""The shape encoder's backward on the CPU (no GPU): the formulas the device runs (shape_encoder_train_f64.device_form) against float64
autograd of the reference's form, the well-posedness of the GPU cases, and the Python surface.

Well-posedness (profiles/shape_encoder_train/wellposed.json holds every figure).  On hash weights the cosines |dot| / (|q| |d|) spread
over [-1, 1]: the least of a case's 1e5 .. 1e7 lies under its own float32-vs-float64 difference, whatever the cloud -- no margin of 100
exists, and in the two larger cases some branches do differ.  So every case runs twice on the GPU: on hash weights with both references
forced onto the device's own branches (`test_forced_branches` checks that machinery here), and on the weights of TR.state_dict,
whose directions are aligned with the features, for which all three conditions are asserted below.
"""
import os
import re

import pytest
import torch
import torch.nn as nn

import shape_encoder_f64 as S
import shape_encoder_train_f64 as TR
from util import ROOT

CPU_CASES = [(1, 32, 1, 7), (3, 48, 2, 32)]


@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: "-".join(map(str, c)))
def test_device_form_is_the_references_gradient(case):
    B, N, L, LAT = case
    sd, pts = TR.state_dict(L, LAT), TR.points(B, N, TR.CASES[case])
    idx = torch.stack([s["idx"] for s in S.forward(sd, pts, L, S.F64)["stops"]])
    up = TR.upstream((B, LAT, 3))
    g, info = TR.device_form(sd, pts, L, idx, S.F64, g_out=up)
    r, out = TR.reference_autograd(sd, pts, L, idx, S.F64, g_out=up)
    assert TR.rel(info["out"], out) < 1e-12
    assert set(g) == set(TR.keys(L)) and len(g) == 4 * (L + 2)
    for k in g:
        assert g[k].shape == r[k].shape and TR.rel(g[k], r[k]) < 1e-12, (k, TR.rel(g[k], r[k]))
    uh = TR.upstream((B * N, L, 128, 3), seed=77)
    g, _ = TR.device_form(sd, pts, L, idx, S.F64, g_hcat=uh)
    r, _ = TR.reference_autograd(sd, pts, L, idx, S.F64, g_hcat=uh)
    for k in g:
        if not k.startswith("conv_c."):
            assert TR.rel(g[k], r[k]) < 1e-12, k


_WELL = {}


def _well(case, kind="aligned"):
    if (case, kind) not in _WELL:
        _WELL[case, kind] = TR.wellposed(case, kind=kind)
    return _WELL[case, kind]


@pytest.mark.parametrize("case", list(TR.CASES), ids=lambda c: "-".join(map(str, c)))
def test_gpu_cases_are_well_posed(case):
    w = _well(case)
    print(w)
    assert w["same_lists"], "float32 and float64 choose different neighbour lists"
    assert w["same_masks"], "float32 and float64 take different leaky-ReLU branches"
    assert w["ratio"] >= 100.0, f"least |cos| {w['least_cos']:.3e} is {w['ratio']:.3g} x the float32-vs-float64 difference {w['cos_diff']:.3e}"


def test_both_branches_are_taken_in_every_stage():
    """The aligned weights put even channels on dot >= 0 and odd ones on dot < 0: no stage is gated on one branch alone."""
    B, N, L, LAT = case = (3, 48, 2, 32)
    sd, pts = TR.state_dict(L, LAT), TR.points(B, N, TR.CASES[case])
    idx = torch.stack([s["idx"] for s in S.forward(sd, pts, L, S.F64)["stops"]])
    _, info = TR.device_form(sd, pts, L, idx, S.F64, g_out=TR.upstream((B, LAT, 3)))
    for k, m in info["masks"].items():
        frac = float(m.double().mean())
        assert 0.4 <= frac <= 0.6, (k, frac)


def test_forced_branches():
    """The references on given branches (what gates the hash-weight runs on the GPU): given float64's own branches they are the unforced
    ones exactly; with the elements of the least |cos| flipped, device form and autograd still agree (up to the flipped elements' own
    forward terms), while the gradient itself moves by far more than any gate allows -- why a branch must not differ inside a gate."""
    B, N, L, LAT = case = (3, 48, 2, 32)
    sd, pts = TR.state_dict(L, LAT, "generic"), TR.points(B, N, TR.HASH[case])
    idx = torch.stack([s["idx"] for s in S.forward(sd, pts, L, S.F64)["stops"]])
    up = TR.upstream((B, LAT, 3))
    g0, _ = TR.reference_autograd(sd, pts, L, idx, S.F64, g_out=up)
    _, info = TR.device_form(sd, pts, L, idx, S.F64, g_out=up)
    own = {k: ~v for k, v in info["masks"].items()}
    g1, _ = TR.reference_autograd(sd, pts, L, idx, S.F64, g_out=up, masks=own)
    assert all(torch.equal(g0[k], g1[k]) for k in g0)
    flipped = {k: own[k] ^ (info["cos"][k].abs() < 3e-4) for k in own}
    assert sum(int((flipped[k] != own[k]).sum()) for k in own) > 20
    gd, _ = TR.device_form(sd, pts, L, idx, S.F64, g_out=up, masks=flipped)
    gr, _ = TR.reference_autograd(sd, pts, L, idx, S.F64, g_out=up, masks=flipped)
    assert max(TR.rel(gd[k], gr[k]) for k in gd) < 1e-3
    assert max(TR.rel(gr[k], g0[k]) for k in g0) > 1e-2
    raw = torch.zeros((L + 2, B * N, 256), dtype=torch.int32)
    for i, name in enumerate(["conv_pos", "blocks.0", "blocks.1"]):
        raw[i, :, :128] = (flipped[name].permute(0, 2, 1).long() << torch.arange(S.K)).sum(-1).int()
    raw[L + 1, :, :LAT] = flipped["conv_c"].int()
    back = TR.device_masks(raw, L, LAT)
    assert all(torch.equal(back[k], flipped[k]) for k in flipped)


@pytest.mark.parametrize("case", list(TR.HASH), ids=lambda c: "-".join(map(str, c)))
def test_lists_of_the_hash_weight_runs(case):
    """On hash weights float32 and float64 choose the same neighbour lists in every case (the branches are the device's, see the GPU file)."""
    B, N, L, LAT = case
    sd, pts = TR.state_dict(L, LAT, "generic"), TR.points(B, N, TR.HASH[case])
    f32, f64 = S.forward(sd, pts, L, S.F32), S.forward(sd, pts, L, S.F64)
    assert all(torch.equal(a["idx"].sort(-1)[0], b["idx"].sort(-1)[0]) for a, b in zip(f32["stops"], f64["stops"]))


def test_golden_fixture_layout():
    from util import golden
    g = golden("shape_encoder_train.npz")
    assert list(g["enc_keys"]) == TR.keys(int(g["layers"])) and g["clouds"].shape == (3, 32, 3) and g["q"].shape == (3, 50, 3)
    assert all(g["grad." + k].dtype == "float32" and g["err." + k].shape == g["grad." + k].shape for k in g["enc_keys"])


def test_running_statistics_rule_is_batchnorms():
    """What VN_DGCNN_Encoder._update_running does with the saved batch mean and biased variance, against nn.BatchNorm on the same norms."""
    from shapemol_amd.shape_encoder import VN_DGCNN_Encoder
    B, N, L, LAT = 2, 32, 1, 7
    sd, pts = S.state_dict(L, LAT), TR.points(B, N, 3)
    f = S.forward(sd, pts, L, S.F64)
    P = B * N
    norms = []
    p, _ = S.edge_pd_pos(pts.reshape(P, 3), f["stops"][0]["idx"], N, sd["conv_pos.map_to_feat.weight"], sd["conv_pos.map_to_dir.weight"], S.F64)
    norms.append(p.norm(dim=-1) + S.EPS)                                          # (P, k, C)
    p, _ = S.edge_pd_block(f["stops"][1]["y"], f["stops"][1]["idx"], N, S.F64)
    norms.append(p.norm(dim=-1) + S.EPS)
    norms.append((f["final"]["pd"][:, :-1].norm(dim=-1) + S.EPS)[:, None])        # (P, 1, LAT)
    stats = torch.zeros((L + 2, 2, 256), dtype=S.F64)
    for i, n in enumerate(norms):
        flat = n.reshape(-1, n.shape[-1])
        stats[i, 0, :flat.shape[1]], stats[i, 1, :flat.shape[1]] = flat.mean(0), flat.var(0, unbiased=False)
    enc = VN_DGCNN_Encoder(128, LAT, L, S.K)
    enc._update_running(stats, P)
    for n, m in zip(norms, enc._stages()):
        bn = nn.BatchNorm2d(n.shape[-1]).double().train()
        bn(n.permute(2, 0, 1)[None])                                              # (1, C, P, k): B N k samples per channel (conv_c: B N)
        assert int(m.batchnorm.bn.num_batches_tracked) == 1
        torch.testing.assert_close(m.batchnorm.bn.running_mean.double(), bn.running_mean, rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(m.batchnorm.bn.running_var.double(), bn.running_var, rtol=1e-6, atol=1e-7)


def test_python_surface():
    from shapemol_amd import _lib
    from shapemol_amd.shape_autoencoder import PointCloud_AE
    cfg = dict(encoder="VN_DGCNN", hidden_dim=128, latent_dim=32, layer_num=2, num_k=20, point_dim=3, loss_type="signeddist")
    ae = PointCloud_AE(cfg)
    with pytest.raises(NotImplementedError, match="get_generator_train_loss") as e:
        ae.get_train_loss(None, None, None)
    assert "get_autoencoder_train_loss" in str(e.value)
    assert callable(ae.get_autoencoder_train_loss) and callable(ae.encoder.encode_train)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ae.encoder.encode_train(torch.zeros(1, 32, 3))
    assert len(ae.encoder._params()) == 4 * (2 + 2)
    header = open(os.path.join(ROOT, "include", "shapemol_hip.h")).read()
    declared = set(re.findall(r"\b(shapemol_[a-z_]+)\s*\(", header))
    new = {"shapemol_se_train_forward", "shapemol_se_train_backward", "shapemol_se_train_workspace", "shapemol_se_load_weights"}
    assert new <= declared and new <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 5 and re.search(r"#define SHAPEMOL_ABI_VERSION 5\b", header)
