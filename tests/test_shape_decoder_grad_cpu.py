"""The gradient helper of the shape decoder (tests/shape_decoder_grad_f64.py) on the CPU: it agrees with the reference's fixture
and with central differences, the device's reverse-mode form passes the gate in float32, the gate rejects each wrong variant,
the fragile caps hold for every case the GPU tests use, and the host-side refusals that need no device."""
import numpy as np
import pytest
import torch

import shape_decoder_f64 as D
import shape_decoder_grad_f64 as DG


def _fixture(loss_type):
    g = np.load(DG.GOLDEN)
    p, s, z = torch.from_numpy(g["p"]), torch.from_numpy(g["batch"]), torch.from_numpy(g["z"])
    sd = D.state_dict(int(g["layers"]), int(g["latent_dim"]))
    ref = DG.reference(sd, p, s, z, 4, loss_type)
    assert DG.cap_ok(ref["fragile"])
    return g, sd, p, s, z, ref


@pytest.mark.parametrize("loss_type", ("signeddist", "occupancy"))
def test_helper_agrees_with_the_fixture(loss_type):
    g, sd, p, s, z, ref = _fixture(loss_type)
    k, lr = ref["keep"], float(g["grad_lr"])
    assert (g["out_" + loss_type] < 0.5).any() and (g["out_" + loss_type] >= 0.5).any()
    assert D.rel_err(g["out_" + loss_type], ref["out64"].numpy()) <= D.bound(0.0)
    cnt = torch.bincount(s)[s].double()
    w64 = ((ref["out64"] < 0.5).double() / cnt)[:, None] * ref["grad64"]
    assert D.rel_err(g["grad_" + loss_type][k.numpy()], w64[k].numpy()) <= D.bound(0.0)
    new64 = DG.guide(p, ref["out64"], ref["grad64"], s, z.shape[0], lr)
    assert D.rel_err(g["pos_" + loss_type][k.numpy()], new64[k].numpy()) <= D.bound(0.0)
    loop = DG.guide_reference_loop(sd, p, s, z, 4, loss_type, lr)
    assert D.rel_err(loop.numpy(), new64.numpy()) <= 2.0 ** -40


@pytest.mark.parametrize("loss_type", ("signeddist", "occupancy"))
def test_gradient_agrees_with_central_differences(loss_type):
    _g, sd, p, s, z, ref = _fixture(loss_type)
    cd = DG.central_differences(sd, p, s, z, 4, loss_type)
    k = ref["keep"]
    assert D.rel_err(cd[k].numpy(), ref["grad64"][k].numpy()) <= 1e-7


@pytest.mark.parametrize("loss_type", ("signeddist", "occupancy"))
def test_device_form_passes_and_faults_fail(loss_type):
    g, sd, p, s, z, ref = _fixture(loss_type)
    out, grad = DG.device_form(sd, p, s, z, 4, loss_type)
    assert D.gate(out, ref["out32"], ref["out64"])[2]
    eh, e32, ok = DG.grad_gate(grad, ref)
    assert ok, (eh, e32)
    for fault in DG.GRAD_FAULTS:
        if fault == "no_sigmoid_slope" and loss_type != "occupancy":
            continue
        _, bad = DG.device_form(sd, p, s, z, 4, loss_type, fault=fault)
        assert not DG.grad_gate(bad, ref)[2], fault
    lr, k = float(g["grad_lr"]), ref["keep"]
    new64 = DG.guide(p, ref["out64"], ref["grad64"], s, z.shape[0], lr)
    new32 = DG.guide(p, ref["out32"], ref["grad32"], s, z.shape[0], lr)
    e32p = D.rel_err(new32[k].numpy(), new64[k].numpy())
    assert D.rel_err(DG.guide(p, out, grad, s, z.shape[0], lr)[k].numpy(), new64[k].numpy()) <= D.bound(e32p)
    for fault in DG.GUIDE_FAULTS:
        bad = DG.guide(p, out, grad, s, z.shape[0], lr, fault=fault)
        assert D.rel_err(bad[k].numpy(), new64[k].numpy()) > D.bound(e32p), fault


def test_fragile_caps_of_the_gpu_cases():
    sd = D.state_dict(4, 32)
    tile = DG.DECODE_TILE
    for Tn in (1, 15, 16, 17, tile - 1, tile, tile + 1, 2 * tile + 1):
        p, s, z = D.inputs(2, Tn, 32, DG.edge_seed(Tn))
        assert DG.cap_ok(DG.reference(sd, p, s, z, 4, "signeddist")["fragile"]), Tn
    for (L, Z, lt), seed in DG.SIZE_SEEDS.items():
        p, s, z = D.inputs(3, 50, Z, seed, z_scale=DG.size_z_scale(Z))
        assert DG.cap_ok(DG.reference(D.state_dict(L, Z), p, s, z, L, lt)["fragile"]), (L, Z, lt)
    for kind in ("ragged5", "small40"):
        c = DG.ragged_counts(kind)
        p, s, z = D.inputs(len(c), c, 32, 31)
        for lt in ("signeddist", "occupancy"):
            assert DG.cap_ok(DG.reference(sd, p, s, z, 4, lt)["fragile"]), (kind, lt)
    p, s, z = D.inputs(5, DG.DECODE_TILE // 2 + 3, 32, 57)
    assert DG.cap_ok(DG.reference(sd, p, s, z, 4, "signeddist")["fragile"])
    p, s, z, totals = DG.tail_case(256)                      # the launch tails on a device of 256 compute units (an MI355X)
    ref = DG.reference(sd, p, s, z, 4, "signeddist")
    for n in totals:
        assert DG.cap_ok(DG.prefix(ref, n)["fragile"]), n


def test_host_side_refusals():
    from shapemol_amd.guidance import _field_decoder
    from shapemol_amd.shape_autoencoder import DecoderInner
    with pytest.raises(ValueError, match="shape_AE"):
        _field_decoder(None)
    with pytest.raises(TypeError, match="shapemol_amd.shape_autoencoder.PointCloud_AE"):
        _field_decoder(torch.nn.Linear(3, 3))
    dec = DecoderInner(3, 32, 128, 4, "signeddist")
    assert _field_decoder(dec) is dec
    p, z = torch.zeros(1, 4, 3), torch.zeros(1, 32, 3)
    for call in (lambda: dec.decode_grad(p, z), lambda: dec.decode_atoms_grad(p[0], torch.zeros(4, dtype=torch.int64), z),
                 lambda: dec.guide_atoms(p[0], torch.zeros(4, dtype=torch.int64), z, 1.0), lambda: dec.field(p, z)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    with pytest.raises(RuntimeError, match="p only"):
        dec.field(p, z.clone().requires_grad_(True))
