"""The training oracle of the shape decoder (tests/shape_decoder_train_f64.py) and its fixture from the reference
(tests/golden/shape_decoder_train*.npz) on the CPU: the oracle reproduces the reference's float64 gradients, the device's
prologue-form backward equals autograd of the concatenated form, the gate rejects each wrong variant, the fragile caps hold for
every case the GPU tests use, and what needs no device of the new interface."""
import os
import re

import numpy as np
import pytest
import torch

import shape_decoder_train_f64 as DT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_TYPES = ("signeddist", "occupancy")


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
def test_oracle_reproduces_the_fixture(loss_type):
    """Float64 autograd of the recomposition against the reference's float64 gradients: agreement far below float32's
    resolution; and its float32 evaluation passes the gate with the reference's own float32 error as e32."""
    g, sd, p, z, v, L, r32, r64 = DT.fixture(loss_type)
    o64 = DT.autograd(sd, p, z, v, L, loss_type, DT.F64)
    for k in r64:
        assert DT.rel_err(o64[k].numpy(), r64[k].numpy()) < 1e-12, k
    o32 = DT.autograd(sd, p, z, v, L, loss_type, DT.F32)
    gates = DT.gate({**o32}, {**r32, "dp": o32["dp"]}, {**r64, "dp": o64["dp"]}, L)
    assert DT.report("oracle f32 " + loss_type, gates)


def test_fixture_conditions_hold():
    g = DT.golden()
    assert g["q"].shape == (3, 50, 3) and int(g["layers"]) == 2 and int(g["latent_dim"]) == 32 and int(g["hidden"]) == 128
    for loss_type in LOSS_TYPES:
        _, sd, p, z, v, L, _, _ = DT.fixture(loss_type)
        taps = DT.autograd(sd, p, z, v, L, loss_type, DT.F64)["relu_in"]
        assert not bool(DT.DG.fragile(taps).any())
        frac = np.array([float((t > 0).double().mean()) for t in taps])
        assert len(frac) == 2 * L + 1 and frac.min() >= 0.40 and frac.max() <= 0.60, frac
        assert np.abs(frac - g["relu_positive_" + loss_type]).max() < 1e-9
        assert all(np.abs(g[f"grad_{loss_type}.blocks.{i}.fc_1.weight"]).max() > 0 for i in range(L))    # the list-held blocks do get gradients
    assert set(str(k) for k in g["gen_keys"]) == set(DT.keys(2))


@pytest.mark.parametrize("loss_type", LOSS_TYPES)
def test_prologue_form_equals_autograd(loss_type):
    g, sd, p, z, v, L, r32, r64 = DT.fixture(loss_type)
    a, d = DT.autograd(sd, p, z, v, L, loss_type, DT.F64), DT.device_form(sd, p, z, v, L, loss_type, DT.F64)
    for k in DT.tensors(L):
        assert DT.rel_err(d[k].numpy(), a[k].numpy()) < 1e-12, k
    assert torch.equal(d["out"], a["out"]) or DT.rel_err(d["out"].numpy(), a["out"].numpy()) < 1e-13
    # and in float32 it passes the gate against the reference
    d32, a32 = DT.device_form(sd, p, z, v, L, loss_type, DT.F32), DT.autograd(sd, p, z, v, L, loss_type, DT.F32)
    assert DT.report("device form f32 " + loss_type, DT.gate(d32, {**r32, "dp": a32["dp"]}, {**r64, "dp": a["dp"]}, L))
    # with a weight: masked points give no gradient
    w = (torch.arange(150) % 7 != 0).float().view(3, 50)
    aw, dw = DT.autograd(sd, p, z, v, L, loss_type, DT.F64, w), DT.device_form(sd, p, z, v, L, loss_type, DT.F64, w)
    for k in DT.tensors(L):
        assert DT.rel_err(dw[k].numpy(), aw[k].numpy()) < 1e-12, k
    assert float(aw["dp"].view(-1, 3)[0].abs().max()) == 0.0


@pytest.mark.parametrize("fault", DT.FAULTS)
def test_negative_controls_fail_the_gate(fault):
    loss_type = "occupancy" if fault == "no_sigmoid_slope" else "signeddist"
    g, sd, p, z, v, L, r32, r64 = DT.fixture(loss_type)
    a32, a64 = DT.autograd(sd, p, z, v, L, loss_type, DT.F32), DT.autograd(sd, p, z, v, L, loss_type, DT.F64)
    bad = DT.device_form(sd, p, z, v, L, loss_type, DT.F32, fault=fault)
    gates = DT.gate(bad, {**r32, "dp": a32["dp"]}, {**r64, "dp": a64["dp"]}, L)
    failed = [k for k, r in gates.items() if not r[3]]
    print(fault, failed)
    assert failed, fault
    expect = {"no_mx": "w.blocks.0.fc_1.weight", "dw0_from_g": "w.blocks.1.fc_0.weight", "no_dzinv": "dz", "no_sigmoid_slope": "w.fc_out.bias",
              "other_shape": "w.fc_in.weight"}[fault]
    assert expect in failed, (fault, failed)


def test_gpu_cases_meet_the_fragile_cap():
    """The seeds of tests/test_gpu_shape_decoder_train.py are chosen here: DT.case asserts the cap from float64 alone."""
    import gpu_train_cases as GC
    for c in GC.all_cases():
        DT.case(*c)
    DT.case(*GC.STRIDE_CASE)


def test_header_and_exports_carry_the_new_names():
    from shapemol_amd import _lib
    header = open(os.path.join(ROOT, "include", "shapemol_hip.h")).read()
    declared = set(re.findall(r"\b(shapemol_[a-z_]+)\s*\(", header))
    new = {"shapemol_field_train", "shapemol_field_load_weights", "shapemol_field_train_tile"}
    assert new <= declared and new <= set(_lib.EXPORTS)
    assert {n for n in declared if n.startswith("shapemol_field_")} == {n for n in _lib.EXPORTS if n.startswith("shapemol_field_")}
    assert _lib.ABI_VERSION == 5 and re.search(r"#define SHAPEMOL_ABI_VERSION 5\b", header)


def test_no_cpu_path():
    from shapemol_amd.shape_autoencoder import PointCloud_AE
    cfg = dict(encoder="VN_DGCNN", hidden_dim=128, latent_dim=32, layer_num=2, num_k=20, point_dim=3, loss_type="signeddist")
    ae = PointCloud_AE(cfg)
    p, z, v = torch.zeros(1, 4, 3), torch.zeros(1, 32, 3, requires_grad=True), torch.zeros(1, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ae.generator.train_field(p, z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ae.get_generator_train_loss(None, p, v, z_vector=z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ae.get_generator_train_loss(torch.zeros(1, 64, 3), p, v)
    with pytest.raises(NotImplementedError, match="get_generator_train_loss"):
        ae.get_train_loss(None, None, None)
    with pytest.raises(RuntimeError, match="p only"):
        ae.generator.field(p, z)
