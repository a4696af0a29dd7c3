"""The device shape decoder (shapemol_sd_*, csrc/sm_shape_dec.h) against float64 (tests/shape_decoder_f64.py) under the
project's gate eH <= 4 e32 + 16 * 2^-24: the reference's fixture, the tile and launch edges, the ragged form and its
column independence, the sizes, a stress profile, the refusals, PointCloud_AE and streams."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import shape_decoder_f64 as D
from vocab import RAGGED_COUNTS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _decoder(L=4, Z=32, loss_type="signeddist", fc1_zero=False):
    from shapemol_amd.shape_autoencoder import DecoderInner
    dec = DecoderInner(3, Z, 128, L, loss_type)
    dec.load_state_dict(D.state_dict(L, Z, fc1_zero=fc1_zero), strict=True)
    return dec.to(DEV)


def _tile():
    return _decoder().tile(DEV)


def _gate(name, res, r32, r64):
    eh, e32, ok = D.gate(res, r32, r64)
    print(f"{name}: eH {eh:.3e} e32 {e32:.3e} bound {D.bound(e32):.3e} {'ok' if ok else 'FAIL'}")
    return ok


def _check(name, dec, out, p, s, z, r32_out=None, fc1_zero=False, prologue=True):
    """Gate the device's output (and the prologue of that call) against float64 on the same inputs."""
    sd = D.state_dict(dec.layer_num, dec.z_dim, fc1_zero=fc1_zero)
    r64 = D.decode(sd, p, s, z, dec.layer_num, dec.loss_type, D.F64)
    r32 = D.decode(sd, p, s, z, dec.layer_num, dec.loss_type, D.F32)
    oks = [_gate(name + " out", out.cpu().reshape(-1), r32["out"] if r32_out is None else r32_out, r64["out"])]
    if prologue:
        B = z.shape[0]
        for key in ("z_inv", "G", "c"):
            oks.append(_gate(f"{name} {key}", dec.debug_read(DEV, key, B), r32[key], r64[key]))
    assert all(oks), name


def _dense(dec, B, T, seed, **kw):
    p, s, z = D.inputs(B, T, dec.z_dim, seed, **kw)
    out = dec(p.view(B, T, 3).to(DEV), z.to(DEV))
    assert tuple(out.shape) == (B, T)
    return out, p, s, z


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_type", ("signeddist", "occupancy"))
def test_fixture_parity(loss_type):
    g = np.load(D.GOLDEN)
    dec = _decoder(int(g["layers"]), int(g["latent_dim"]), loss_type)
    p, z = torch.from_numpy(g["p"]), torch.from_numpy(g["z"])
    B, T = p.shape[:2]
    out = dec(p.to(DEV), z.to(DEV))
    s = torch.arange(B).repeat_interleave(T)
    _check("fixture " + loss_type, dec, out, p.reshape(-1, 3), s, z, r32_out=g["out_" + loss_type].reshape(-1))
    r64 = D.decode(D.state_dict(4, 32), p.reshape(-1, 3), s, z, 4, loss_type, D.F64)
    assert _gate("fixture z_inv vs the reference's", dec.debug_read(DEV, "z_inv", B), g["z_inv"], r64["z_inv"])


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_tile_edges():
    dec, tile = _decoder(), _tile()
    assert tile >= 16 and tile % 16 == 0
    for T in (1, 15, 16, 17, tile - 1, tile, tile + 1, 2 * tile + 1):
        out, p, s, z = _dense(dec, 2, T, 100 + T)
        _check(f"T={T}", dec, out, p, s, z)


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_launch_tails():
    """Totals around one and two tiles per compute unit: the last workgroup's tail, and the first second iteration."""
    dec, tile = _decoder(), _tile()
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    full = 2 * cus * tile + 1
    p, _, z = D.inputs(2, [full, 0], dec.z_dim, 7)
    s = torch.from_numpy((np.arange(full) * 7 // 5) % 2)                       # both shapes inside every tile
    sd = D.state_dict(4, 32)
    r64 = D.decode(sd, p, s, z, 4, "signeddist", D.F64)["out"]
    r32 = D.decode(sd, p, s, z, 4, "signeddist", D.F32)["out"]
    pd, sdv, zd = p.to(DEV), s.to(DEV), z.to(DEV)
    oks = []
    for n in (cus * tile - 1, cus * tile, cus * tile + 1, 2 * cus * tile - 1, 2 * cus * tile, 2 * cus * tile + 1):
        out = dec.decode_atoms(pd[:n], sdv[:n], zd).cpu()
        assert out.shape == (n,)
        oks.append(_gate(f"n={n}", out, r32[:n], r64[:n]))
    assert all(oks)


# 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", (tuple(int(c) for c in RAGGED_COUNTS), tuple(1 + (i * 7) % 3 for i in range(40))), ids=("ragged5", "small40"))
def test_ragged_gate(counts):
    dec = _decoder()
    p, s, z = D.inputs(len(counts), counts, dec.z_dim, 31)
    out = dec.decode_atoms(p.to(DEV), s.to(DEV), z.to(DEV))
    _check(f"ragged {len(counts)}", dec, out, p, s, z)


# 5 ------------------------------------------------------------------------------------------------------------------------
def test_ragged_independence():
    dec, tile = _decoder(), _tile()
    B, T = 5, tile // 2 + 3
    out, p, s, z = _dense(dec, B, T, 57)
    pd, sdv, zd = p.to(DEV), s.to(DEV), z.to(DEV)
    flat = dec.decode_atoms(pd, sdv, zd)
    assert torch.equal(flat, out.reshape(-1))
    perm = torch.from_numpy(np.random.RandomState(3).permutation(B * T)).to(DEV)
    shuffled = dec.decode_atoms(pd[perm], sdv[perm], zd)
    back = torch.empty_like(shuffled)
    back[perm] = shuffled
    assert torch.equal(back, flat)
    assert torch.equal(dec.decode_atoms(pd[:7], sdv[:7], zd), flat[:7])        # nor on what else is in the launch


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (1, 4, 8))
@pytest.mark.parametrize("Z", (1, 32, 48))
def test_sizes(L, Z):
    dec = _decoder(L, Z)
    out, p, s, z = _dense(dec, 3, 70, 10 * L + Z)
    _check(f"L={L} Z={Z}", dec, out, p, s, z)


# 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fc1_zero", (False, True), ids=("hash", "fc1zero"))
@pytest.mark.parametrize("loss_type", ("signeddist", "occupancy"))
def test_stress(loss_type, fc1_zero):
    """Points up to 12 A from the origin and latents times 4: |p|^2 and p.z dominate fc_in.  fc_1 = 0 is the reference's
    initialisation: a block adds its bias only."""
    dec = _decoder(4, 32, loss_type, fc1_zero)
    B, T = 3, 300
    p, s, z = D.inputs(B, T, 32, 77, z_scale=2.0)
    u = torch.from_numpy(D.synth.hash_uniform((B * T, 1), 613, 77))
    p = (p / p.norm(dim=1, keepdim=True).clamp(min=1e-3) * (12.0 * u)).float()  # radii uniform in [0, 12)
    out = dec(p.view(B, T, 3).to(DEV), z.to(DEV))
    _check(f"stress {loss_type} fc1_zero={fc1_zero}", dec, out, p, s, z, fc1_zero=fc1_zero)


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from shapemol_amd import _lib
    from shapemol_amd.shape_autoencoder import DecoderInner
    lib = _lib.load()
    E = _lib.ShapeMolLibraryError
    p1, z1 = torch.zeros(1, 4, 3, device=DEV), torch.zeros(1, 32, 3, device=DEV)
    for kw, word in ((dict(hidden_size=64), "128"), (dict(z_dim=257), "1..256"), (dict(layer_num=9), "1..8")):
        args = dict(dict(dim=3, z_dim=32, hidden_size=128, layer_num=4, loss_type="signeddist"), **kw)
        bad = DecoderInner(**args).to(DEV)
        with pytest.raises(E, match=word):
            bad(p1, torch.zeros(1, args["z_dim"], 3, device=DEV))
    w = np.zeros(lib.shapemol_sd_weight_count(128, 32, 4) + 1, np.float32)
    ctx = C.c_void_p()
    assert lib.shapemol_sd_create(128, 32, 4, 0, w.ctypes.data_as(C.c_void_p), w.size, 0, C.byref(ctx)) != 0 and not ctx.value
    assert b"weight count" in lib.shapemol_last_error()
    assert lib.shapemol_sd_create(128, 0, 4, 0, w.ctypes.data_as(C.c_void_p), w.size, 0, C.byref(ctx)) != 0 and b"1..256" in lib.shapemol_last_error()
    assert lib.shapemol_sd_create(128, 32, 0, 0, w.ctypes.data_as(C.c_void_p), w.size, 0, C.byref(ctx)) != 0 and b"1..8" in lib.shapemol_last_error()
    dec = _decoder()
    with pytest.raises(E, match="65535"):
        dec(torch.zeros(65536, 1, 3, device=DEV), torch.zeros(65536, 32, 3, device=DEV))
    c = dec._context(torch.device(DEV))
    # n_points = 2^31 and n_shapes = 0 on the C ABI itself: refused on the counts alone, no pointer is touched
    dummy = C.c_void_p(p1.data_ptr())
    assert lib.shapemol_sd_decode(c, dummy, dummy, 2 ** 31, 0, C.c_void_p(z1.data_ptr()), 1, dummy, None) != 0
    assert b"2^31" in lib.shapemol_last_error()
    assert lib.shapemol_sd_decode(c, dummy, dummy, 4, 0, C.c_void_p(z1.data_ptr()), 0, dummy, None) != 0
    assert b"1..65535" in lib.shapemol_last_error()
    pos, z = torch.zeros(6, 3, device=DEV), torch.zeros(2, 32, 3, device=DEV)
    for bad in (2, -1):
        b = torch.tensor([0, 1, 0, bad, 1, 0], device=DEV)
        with pytest.raises(ValueError, match=r"\[0, 2\)"):
            dec.decode_atoms(pos, b, z)
    assert dec.decode_atoms(pos[:0], torch.zeros(0, dtype=torch.long, device=DEV), z).shape == (0,)
    assert dec(torch.zeros(2, 0, 3, device=DEV), z).shape == (2, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dec(torch.zeros(1, 4, 3), z1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dec(p1, torch.zeros(1, 32, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dec.decode_atoms(pos.cpu(), torch.zeros(6, dtype=torch.long), z)
    assert dec.tile("cuda") == dec.tile(DEV)
    out = dec(p1, z1)                                                           # the context still works after the refusals
    assert dec.debug_read("cuda", "c", 1).shape == (1, 128)                     # 'cuda' is the current device's context, not a new one
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_point_cloud_ae():
    from shapemol_amd.shape_autoencoder import PointCloud_AE
    import shape_encoder_f64 as S
    g = np.load(D.GOLDEN)
    L, Z = int(g["layers"]), int(g["latent_dim"])
    ae = PointCloud_AE(dict(encoder="VN_DGCNN", hidden_dim=128, latent_dim=Z, layer_num=L, num_k=int(g["k"]), point_dim=3, loss_type="occupancy"))
    ae.encoder.load_state_dict(S.state_dict(L, Z), strict=False)
    ae.generator.load_state_dict(D.state_dict(L, Z), strict=True)
    ae = ae.to(DEV)
    clouds, q, vals = (torch.from_numpy(g[k]) for k in ("ae_clouds", "ae_q", "ae_values"))
    B, T = q.shape[:2]
    s = torch.arange(B).repeat_interleave(T)
    zv, out = ae(clouds.unsqueeze(1).to(DEV), None, q.to(DEV))
    assert torch.equal(out, ae.generator(q.to(DEV), ae.encoder(clouds.unsqueeze(1).to(DEV)))) and tuple(zv.shape) == (B, Z, 3)
    # the decoder on the device's own latent against float64 on that same latent
    _check("ae own latent", ae.generator, out, q.reshape(-1, 3), s, zv.cpu())
    # the fixture's forward: the decoder at the reference's latent against the reference's output
    z_ref = torch.from_numpy(g["ae_z"])
    z2, out_ref = ae(None, z_ref.to(DEV), q.to(DEV))
    assert torch.equal(z2.cpu(), z_ref)
    _check("ae fixture latent", ae.generator, out_ref, q.reshape(-1, 3), s, z_ref, r32_out=g["ae_out"].reshape(-1))
    assert ae(None, z_ref.to(DEV), None) [1] is None
    # get_val_loss: the reference's formulas on the device's output
    loss, acc, rec = ae.get_val_loss(clouds.to(DEV), q.to(DEV), vals.to(DEV))
    l2, a2, r2 = D.val_loss(out, vals.to(DEV))
    assert torch.equal(loss, l2) and torch.equal(acc, a2) and torch.equal(rec, r2)
    # the fixture's triple: the loss at the reference's latent under the gate (a scalar: eH and e32 against the float64 loss of the
    # float64 decoder on that latent, e32 the reference's own loss); accuracy and recall exactly, no output being near 0.5
    l3, a3, r3 = D.val_loss(out_ref.cpu(), vals)
    o64 = D.decode(D.state_dict(L, Z), q.reshape(-1, 3), s, z_ref, L, "occupancy", D.F64)["out"].view(B, T)
    l64 = float(D.val_loss(o64, vals.double())[0])
    assert _gate("val loss", float(l3), g["ae_val"][0], l64)
    margin = float((torch.from_numpy(g["ae_out"]) - 0.5).abs().min())
    print(f"least |out - 0.5| = {margin:.2e}")
    assert margin > 1e-4 and float(a3) == pytest.approx(g["ae_val"][1], abs=1e-7) and float(r3) == pytest.approx(g["ae_val"][2], abs=1e-7)
    # and get_val_loss itself from the clouds, whose latent is the device encoder's: against float64 on that same latent
    o64 = D.decode(D.state_dict(L, Z), q.reshape(-1, 3), s, zv.cpu(), L, "occupancy", D.F64)["out"].view(B, T)
    o32 = D.decode(D.state_dict(L, Z), q.reshape(-1, 3), s, zv.cpu(), L, "occupancy", D.F32)["out"].view(B, T)
    assert _gate("val loss, own latent", float(loss), float(D.val_loss(o32, vals)[0]), float(D.val_loss(o64, vals.double())[0]))
    with pytest.raises(NotImplementedError):
        ae.get_train_loss(clouds.to(DEV), q.to(DEV), vals.to(DEV))


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_streams_and_parameter_edits():
    from shapemol_amd.shape_autoencoder import DecoderInner
    dec = DecoderInner(3, 32, 128, 2, "signeddist")
    dec.load_state_dict(D.state_dict(2, 32), strict=True)
    dec = dec.to(DEV)
    p, s, z = D.inputs(2, 333, 32, 91)
    pd, zd = p.view(2, 333, 3).to(DEV), z.to(DEV)
    ref = dec(pd, zd)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        out = dec(pd, zd)
    side.synchronize()
    assert torch.equal(out, ref)
    with torch.no_grad():
        dec.fc_out.bias.add_(1.0)
        dec.blocks[1].fc_1.weight.mul_(0.5)
    new = dec(pd, zd)
    sd = D.state_dict(2, 32)
    sd["fc_out.bias"] = sd["fc_out.bias"] + 1.0
    sd["blocks.1.fc_1.weight"] = sd["blocks.1.fc_1.weight"] * 0.5
    r64, r32 = D.decode(sd, p, s, z, 2, "signeddist", D.F64), D.decode(sd, p, s, z, 2, "signeddist", D.F32)
    assert not torch.equal(new, ref) and _gate("edited", new.cpu().reshape(-1), r32["out"], r64["out"])
