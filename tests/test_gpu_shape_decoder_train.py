"""Training the shape decoder on the device (shapemol_field_train, csrc/sm_shape_dec_train.h) against the float64 oracle
(tests/shape_decoder_train_f64.py) under the project's gate eH <= 4 e32 + 16 * 2^-24 per tensor: every parameter gradient, dz,
dp and the loss, on the reference's fixture and at the tile, chunk, depth and latent edges (tests/gpu_train_cases.py); bit
equality with forward and between calls; weights repacked on the device after optimiser steps; the captured chain's key."""
import ctypes as C

import numpy as np
import pytest
import torch

import gpu_train_cases as GC
import shape_decoder_f64 as D
import shape_decoder_grad_f64 as DG
import shape_decoder_train_f64 as DT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _decoder(L=4, Z=32, loss_type="signeddist", sd=None, **kw):
    from shapemol_amd.shape_autoencoder import DecoderInner
    dec = DecoderInner(3, Z, 128, L, loss_type)
    dec.load_state_dict(sd if sd is not None else D.state_dict(L, Z, **kw), strict=True)
    return dec.to(DEV)


def _run(dec, p, z, v, w=None, chunk=0, p_grad=True):
    """One forward + backward of the weighted loss through train_field -> the gate's dict (CPU tensors)."""
    pd, zd = p.to(DEV).requires_grad_(p_grad), z.to(DEV).requires_grad_(True)
    for q in dec.parameters():
        q.grad = None
    out = dec.train_field(pd, zd, chunk_points=chunk)
    wt = torch.ones_like(out) if w is None else w.to(DEV)
    loss = (wt * (out - v.to(DEV)) ** 2).sum() / out.numel()
    loss.backward()
    res = {"loss": loss.detach().cpu(), "out": out.detach().cpu(), "dz": zd.grad.cpu()}
    if p_grad:
        res["dp"] = pd.grad.cpu()
    res.update({"w." + k: q.grad.cpu() for k, q in dec.named_parameters()})
    return res


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("case", GC.all_cases(), ids=lambda c: "B{}_T{}_Z{}_L{}_{}".format(*c[:5]))
def test_gate_at_the_edges(case):
    B, T, Z, L, loss_type, seed = case
    sd, p, z, v, w, r32, r64 = DT.case(*case)
    dec = _decoder(L, Z, loss_type)
    tile = dec.train_tile(DEV)
    assert tile == GC.TILE
    fwd = dec(p.to(DEV), z.to(DEV)).cpu()
    assert D.gate(fwd.reshape(-1), r32["out"].reshape(-1), r64["out"].reshape(-1))[2]
    for chunk_tiles in GC.CASES[case]:
        res = _run(dec, p, z, v, w, chunk_tiles * tile)
        assert torch.equal(res["out"], fwd)                                   # the value is forward's, bit for bit
        assert all(bool(torch.isfinite(t).all()) for t in res.values())
        assert DT.report(f"{case} chunk {chunk_tiles}", DT.gate(res, r32, r64, L)), (case, chunk_tiles)
        assert _same(res, _run(dec, p, z, v, w, chunk_tiles * tile))          # two calls: identical bits


@pytest.mark.parametrize("chunk_tiles", (0, 2))
@pytest.mark.parametrize("loss_type", ("signeddist", "occupancy"))
def test_training_sweep_is_the_gradient_sweep(loss_type, chunk_tiles):
    """With the upstream gradient all ones the training kernel and the value-and-gradient kernel do the same operations on the
    same operands (w * 1 and 1 * (s (1 - s)) are exact): value and point gradient are the same bits.  B = 3, T = 183: 16-point
    groups and tiles mix shapes, and with chunks of two tiles a shape spans chunks."""
    case = next(c for c in GC.all_cases() if c[:2] == (3, 183) and c[4] == loss_type)
    sd, p, z = DT.case(*case)[:3]
    dec = _decoder(case[3], case[2], loss_type, sd=sd)
    pd, zd = p.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
    out = dec.train_field(pd, zd, chunk_points=chunk_tiles * GC.TILE)
    out.sum().backward()
    val, grad = dec.decode_grad(p.to(DEV), z.to(DEV))
    assert torch.equal(out.detach(), val)
    assert torch.equal(pd.grad, grad)


def test_workgroups_stride_over_tiles():
    """One chunk of more tiles than the device has compute units: every workgroup takes several tiles, the last of one point."""
    case = GC.STRIDE_CASE
    if torch.cuda.get_device_properties(0).multi_processor_count > GC.CUS:
        pytest.fail("gpu_train_cases.CUS is below this device's compute units: the case would not stride")
    sd, p, z, v, w, r32, r64 = DT.case(*case)
    dec = _decoder(case[3], case[2], case[4])
    fwd = dec(p.to(DEV), z.to(DEV)).cpu()
    res = _run(dec, p, z, v, w, GC.STRIDE_CHUNK_TILES * GC.TILE)
    assert torch.equal(res["out"], fwd)
    assert DT.report("stride", DT.gate(res, r32, r64, case[3]))
    # the default chunking of the same points (two chunks, another order of the sums) passes the gate too
    assert DT.report("stride, default chunks", DT.gate(_run(dec, p, z, v, w, 0), r32, r64, case[3]))


@pytest.mark.parametrize("loss_type", ("signeddist", "occupancy"))
def test_fixture_through_get_generator_train_loss(loss_type):
    """The reference's loss.backward(): its own float32 gradients give e32 (dp, which it does not form, from the recomposition)."""
    from shapemol_amd.shape_autoencoder import PointCloud_AE
    g, sd, p, z, v, L, r32, r64 = DT.fixture(loss_type)
    ae = PointCloud_AE(dict(encoder="VN_DGCNN", hidden_dim=128, latent_dim=32, layer_num=L, num_k=int(g["k"]), point_dim=3, loss_type=loss_type))
    ae.generator.load_state_dict(sd, strict=True)
    ae = ae.to(DEV)
    pd, zd = p.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
    loss = ae.get_generator_train_loss(None, pd, v.to(DEV), z_vector=zd)
    loss.backward()
    assert all(q.grad is None for q in ae.encoder.parameters())
    res = {"loss": loss.detach().cpu(), "dz": zd.grad.cpu(), "dp": pd.grad.cpu()}
    res.update({"w." + k: q.grad.cpu() for k, q in ae.generator.named_parameters()})
    a32, a64 = DT.autograd(sd, p, z, v, L, loss_type, DT.F32), DT.autograd(sd, p, z, v, L, loss_type, DT.F64)
    assert DT.report("fixture " + loss_type, DT.gate(res, {**r32, "dp": a32["dp"]}, {**r64, "dp": a64["dp"]}, L))
    # and with the latent from the device encoder the loss is differentiable in the generator alone
    for q in ae.generator.parameters():
        q.grad = None
    ae.get_generator_train_loss(torch.from_numpy(g["clouds"]).to(DEV), p.to(DEV), v.to(DEV)).backward()
    assert all(q.grad is not None for q in ae.generator.parameters()) and all(q.grad is None for q in ae.encoder.parameters())


def test_reference_initialisation():
    """fc_1.weight == 0: nothing flows back through a block's second Linear, so fc_0 gets exact zeros; fc_1 does not."""
    L, Z = 4, 32
    dec = _decoder(L, Z, fc1_zero=True)
    p, _, z = D.inputs(2, 77, Z, 41)
    v = torch.zeros(2, 77)
    res = _run(dec, p.view(2, 77, 3), z, v)
    for i in range(L):
        assert float(res[f"w.blocks.{i}.fc_0.weight"].abs().max()) == 0.0 and float(res[f"w.blocks.{i}.fc_0.bias"].abs().max()) == 0.0
        assert float(res[f"w.blocks.{i}.fc_1.weight"].abs().max()) > 0.0 and float(res[f"w.blocks.{i}.fc_1.bias"].abs().max()) > 0.0


def test_optimizer_steps_repack_on_the_device():
    L, Z = 2, 32
    dec = _decoder(L, Z)
    p, _, z = D.inputs(3, 50, Z, 42)
    pd, zd = p.view(3, 50, 3).to(DEV), z.to(DEV)
    v = (0.3 * pd[..., 0]).contiguous()
    dec(pd, zd)
    handle = dec._ctx.value
    losses = []
    for opt in (torch.optim.SGD(dec.parameters(), lr=1e-2), torch.optim.Adam(dec.parameters(), lr=1e-3)):
        for _ in range(1 if isinstance(opt, torch.optim.SGD) else 10):
            opt.zero_grad()
            loss = torch.mean((dec.train_field(pd, zd) - v) ** 2)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        out = dec(pd, zd)
        assert dec._ctx.value == handle                                       # no new context
        fresh = _decoder(L, Z, sd={k: t.detach().cpu() for k, t in dec.state_dict().items()})
        assert torch.equal(out, fresh(pd, zd))
    final = float(torch.mean((dec(pd, zd) - v) ** 2))
    print("losses", losses, final)
    assert final < losses[1] and losses[-1] < losses[1]                       # ten Adam steps on a fixed batch


def test_latent_only_fit():
    L, Z = 2, 32
    dec = _decoder(L, Z)
    before = {k: t.detach().clone() for k, t in dec.state_dict().items()}
    for q in dec.parameters():
        q.requires_grad_(False)
    p, _, z = D.inputs(2, 60, Z, 43)
    pd = p.view(2, 60, 3).to(DEV)
    target = dec(pd, (1.2 * z).to(DEV))
    zd = z.to(DEV).requires_grad_(True)
    opt = torch.optim.Adam([zd], lr=1e-2)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = torch.mean((dec.train_field(pd, zd) - target) ** 2)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("latent fit", losses)
    assert losses[-1] < losses[0]
    assert all(torch.equal(before[k], t) for k, t in dec.state_dict().items()) and all(q.grad is None for q in dec.parameters())


def test_chain_follows_load_weights():
    """A captured field-guided chain is keyed on the decoder's identity, which a load of weights advances: the same values give
    the same chain, other values the chain of a fresh decoder with them."""
    from util import T, hip_model, maxabs, oracle_model
    m = hip_model()
    _sd, dm, _cfg, _ = oracle_model()
    bb, eps, u = DG.chain_inputs(DG.CHAIN_SEED)
    args = (T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(DG.CHAIN_B, -1))
    kw = dict(num_steps=DG.CHAIN_STEPS, center_pos_mode="none", noise=(T(eps, DEV), T(u, DEV)))
    gk = dict(use_grad=True, grad_lr=DG.CHAIN_LR, grad_step=dm.T - 1 - 10)
    dec = _decoder(4, 32)
    a = m.sample_diffusion(*args, **kw, **gk, shape_AE=dec)
    handle = dec._ctx.value
    flat = torch.cat([q.detach().reshape(-1) for q in dec._params()])
    dec._load_weights(dec._ctx, flat, torch.device(DEV))
    b = m.sample_diffusion(*args, **kw, **gk, shape_AE=dec)
    assert torch.equal(a["pos"], b["pos"]) and torch.equal(a["v"], b["v"])
    other = D.state_dict(4, 32, seed=23)
    with torch.no_grad():
        for k, q in dec.named_parameters():
            q.copy_(other[k].to(DEV))
    c = m.sample_diffusion(*args, **kw, **gk, shape_AE=dec)
    assert dec._ctx.value == handle
    ref = m.sample_diffusion(*args, **kw, **gk, shape_AE=_decoder(4, 32, sd=other), use_graph=False)
    assert torch.equal(c["pos"], ref["pos"]) and torch.equal(c["v"], ref["v"])
    assert maxabs(c["pos"], a["pos"]) > 1e-4


def test_refusals():
    from shapemol_amd import _lib
    dec = _decoder(2, 32)
    lib, ctx = _lib.load(), dec._context(DEV)
    tile = dec.train_tile(DEV)
    n_w = int(lib.shapemol_sd_weight_count(128, 32, 2))
    p, z, up = torch.zeros(4, 3, device=DEV), torch.zeros(1, 32, 3, device=DEV), torch.zeros(4, device=DEV)
    gz, gw = torch.zeros(1, 32, 3, device=DEV), torch.zeros(n_w, device=DEV)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(n_shapes=1, per=4, upstream=up, chunk=0):
        return lib.shapemol_field_train(ctx, vp(p), n_shapes, per, vp(z), vp(upstream) if upstream is not None else None, None, None, vp(gz), vp(gw), chunk, None)
    assert call() == 0
    for bad, word in ((dict(upstream=None), "upstream"), (dict(chunk=tile + 1), "multiple of the tile"), (dict(chunk=-tile), "multiple of the tile"),
                      (dict(n_shapes=0), "n_shapes"), (dict(n_shapes=65536), "n_shapes"), (dict(per=-1), "points_per_shape")):
        assert call(**bad) == 1 and word in lib.shapemol_last_error().decode(), bad
    assert lib.shapemol_field_load_weights(ctx, vp(gw), n_w - 1, None) == 1 and "mismatch" in lib.shapemol_last_error().decode()
    torch.cuda.synchronize()
    cpu = _decoder(2, 32).cpu()
    with pytest.raises(RuntimeError, match="no CPU path"):
        cpu.train_field(torch.zeros(1, 4, 3, device=DEV), z)
