"""The shape decoder's float64 / float32 recomposition (tests/shape_decoder_f64.py) and its fixture
(tests/golden/shape_decoder.npz) tested on the CPU: the recomposition must reproduce the reference's outputs, accept the
device's factored fc_in, and reject the faults the gate exists to find."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import shape_decoder_f64 as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_TYPES = ("signeddist", "occupancy")


@functools.lru_cache(maxsize=None)
def _fixture():
    g = np.load(D.GOLDEN)
    L, Z = int(g["layers"]), int(g["latent_dim"])
    sd = D.state_dict(L, Z, int(g["hidden"]), int(g["dec_seed"]))
    B, T = g["p"].shape[:2]
    p = torch.from_numpy(g["p"]).reshape(B * T, 3)
    shape_of = torch.arange(B).repeat_interleave(T)
    return g, sd, p, shape_of, torch.from_numpy(g["z"]), L


@functools.lru_cache(maxsize=None)
def _r64(loss_type):
    g, sd, p, s, z, L = _fixture()
    return D.decode(sd, p, s, z, L, loss_type, D.F64, taps=True)


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
def test_float32_recomposition_reproduces_the_fixture(loss_type):
    """e32 is the reference's own error against float64; the float32 recomposition passes the gate against it."""
    g, sd, p, s, z, L = _fixture()
    r64, r32 = _r64(loss_type), D.decode(sd, p, s, z, L, loss_type, D.F32)
    ref = g["out_" + loss_type].reshape(-1)
    eh, e32, ok = D.gate(r32["out"], ref, r64["out"])
    print(f"{loss_type}: eH {eh:.3e} e32 {e32:.3e} bound {D.bound(e32):.3e}")
    assert ok and e32 < 64 * D.U, (eh, e32)                     # and the reference itself is a float32 evaluation of that float64 value
    if loss_type == "signeddist":
        assert D.gate(r32["z_inv"], g["z_inv"], r64["z_inv"])[2]


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
def test_factored_fc_in_passes_the_gate(loss_type):
    g, sd, p, s, z, L = _fixture()
    r64 = _r64(loss_type)
    fac = D.decode(sd, p, s, z, L, loss_type, D.F32, form="factored")
    eh, e32, ok = D.gate(fac["out"], g["out_" + loss_type].reshape(-1), r64["out"])
    assert ok, (eh, e32)
    f64 = D.decode(sd, p, s, z, L, loss_type, D.F64, form="factored")      # the same function, not only close at float32
    assert D.rel_err(f64["out"], r64["out"]) < 1e-13


@pytest.mark.parametrize("fault", [f for f in D.FAULTS if f != "f16x2"])
def test_negative_controls_fail_the_gate(fault):
    g, sd, p, s, z, L = _fixture()
    r64 = _r64("signeddist")
    bad = D.decode(sd, p, s, z, L, "signeddist", D.F32, fault=fault)
    eh, e32, ok = D.gate(bad["out"], g["out_signeddist"].reshape(-1), r64["out"])
    assert not ok, (fault, eh, e32)


def test_two_piece_f16_operands_fail_the_gate():
    """Operands as two fp16 pieces, arithmetic in float64 after that: on the fixture's weights with fc_0 scaled by 2^-6 and
    fc_1 by 2^6, which leaves the decoder the same function (float32 agrees with the unscaled evaluation to the bit)."""
    g, sd, p, s, z, L = _fixture()
    small = D.state_dict(L, int(g["latent_dim"]), int(g["hidden"]), int(g["dec_seed"]), small_fc0=True)
    r64 = _r64("signeddist")
    assert torch.equal(D.decode(small, p, s, z, L, "signeddist", D.F32)["out"], D.decode(sd, p, s, z, L, "signeddist", D.F32)["out"])
    bad = D.decode(small, p, s, z, L, "signeddist", D.F64, fault="f16x2")
    eh, e32, ok = D.gate(bad["out"], g["out_signeddist"].reshape(-1), r64["out"])
    assert not ok, (eh, e32)
    exact = D.decode(small, p, s, z, L, "signeddist", D.F64)                # the exact split is the float32 operand itself
    assert D.gate(exact["out"], g["out_signeddist"].reshape(-1), r64["out"])[2]


def test_fixture_conditions_hold():
    """The conditions the generator asserted on the reference, recomputed here from the float64 recomposition."""
    g, sd, p, s, z, L = _fixture()
    r = _r64("signeddist")
    o = g["out_signeddist"]
    assert (o.max() - o.min()) / np.abs(o).max() > 0.10 and float(g["out_span"]) > 0.10
    frac = np.array([float((t > 0).double().mean()) for t in r["relu_in"]])
    assert len(frac) == 2 * L + 1 and frac.min() >= 0.10 and frac.max() <= 0.90, frac
    assert np.abs(frac - g["relu_positive"]).max() < 0.01
    occ = g["out_occupancy"]
    assert ((occ <= 0.02) | (occ >= 0.98)).mean() <= 0.10 and float(g["sigmoid_saturated"]) <= 0.10
    assert g["p"].shape == (3, 50, 3) and g["z"].shape == (3, 32, 3) and g["ae_clouds"].shape == (3, 64, 3)


def test_fixture_val_loss_follows_from_its_output():
    g = np.load(D.GOLDEN)
    loss, acc, rec = D.val_loss(torch.from_numpy(g["ae_out"]), torch.from_numpy(g["ae_values"]))
    assert abs(float(loss) - g["ae_val"][0]) < 1e-6 and float(acc) == pytest.approx(g["ae_val"][1], abs=1e-7)
    assert float(rec) == pytest.approx(g["ae_val"][2], abs=1e-7)


def test_auto_encoder_decodes_the_reference_latent():
    """The fixture's PointCloud_AE output is the decoder at the fixture's latent (occupancy)."""
    g, sd, _, _, _, L = _fixture()
    B, T = g["ae_q"].shape[:2]
    q, s, z = torch.from_numpy(g["ae_q"]).reshape(B * T, 3), torch.arange(B).repeat_interleave(T), torch.from_numpy(g["ae_z"])
    r64, r32 = D.decode(sd, q, s, z, L, "occupancy", D.F64), D.decode(sd, q, s, z, L, "occupancy", D.F32)
    assert D.gate(r32["out"], g["ae_out"].reshape(-1), r64["out"])[2]


def test_header_and_exports_agree():
    from shapemol_amd import _lib
    header = open(os.path.join(ROOT, "include", "shapemol_hip.h")).read()
    declared = {n for n in re.findall(r"\b(shapemol_[a-z_]+)\s*\(", header) if n.startswith("shapemol_sd_")}
    assert declared == {"shapemol_sd_weight_count", "shapemol_sd_create", "shapemol_sd_destroy", "shapemol_sd_decode",
                        "shapemol_sd_debug_read", "shapemol_sd_tile"}
    assert declared == {n for n in _lib.EXPORTS if n.startswith("shapemol_sd_")}
    assert _lib.ABI_VERSION == 5 and re.search(r"#define SHAPEMOL_ABI_VERSION 5\b", header)


def test_state_dict_keys_cover_the_references():
    """Every key the reference's PointCloud_AE saves exists here (so ckpt['model'] loads with strict=False and nothing saved is
    dropped); the blocks, which the reference keeps in plain lists, are extra keys here."""
    import shapemol_amd
    from shapemol_amd.shape_autoencoder import PointCloud_AE, DecoderInner
    assert shapemol_amd.PointCloud_AE is PointCloud_AE and shapemol_amd.DecoderInner is DecoderInner
    g = np.load(D.GOLDEN)
    cfg = dict(encoder="VN_DGCNN", hidden_dim=128, latent_dim=32, layer_num=4, num_k=20, point_dim=3, loss_type="signeddist")
    ae = PointCloud_AE(cfg)
    keys = set(ae.state_dict().keys())
    ref = set(str(k) for k in g["ae_keys"])
    assert ref and ref <= keys, sorted(ref - keys)
    assert {"generator.z_in.map_to_feat.weight", "generator.fc_in.weight", "generator.fc_out.bias"} <= ref
    assert {f"generator.blocks.{i}.{fc}.{w}" for i in range(4) for fc in ("fc_0", "fc_1") for w in ("weight", "bias")} <= keys - ref
    missing, unexpected = ae.load_state_dict({k: v for k, v in ae.state_dict().items() if k in ref}, strict=False)
    assert not unexpected and all(".blocks." in k for k in missing)
    assert float(ae.generator.blocks[0].fc_1.weight.detach().abs().max()) == 0.0          # the reference's initialisation
    with pytest.raises(NotImplementedError):
        PointCloud_AE(dict(cfg, encoder="VN_Resnet"))
    with pytest.raises(NotImplementedError):
        ae.get_train_loss(None, None, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ae.generator(torch.zeros(1, 4, 3), torch.zeros(1, 32, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ae.generator.decode_atoms(torch.zeros(4, 3), torch.zeros(4, dtype=torch.long), torch.zeros(1, 32, 3))


def test_synthetic_decoder_weights():
    from shapemol_amd import synth
    sd = synth.shape_decoder_state_dict(128, 32, 4, seed=19)
    from shapemol_amd.shape_autoencoder import DecoderInner
    dec = DecoderInner(3, 32, 128, 4, "signeddist")
    assert set(sd) == set(dec.state_dict().keys())
    assert all(tuple(sd[k].shape) == tuple(v.shape) for k, v in dec.state_dict().items())
    assert all(np.abs(sd[f"blocks.{i}.fc_1.weight"]).max() > 0 for i in range(4))
