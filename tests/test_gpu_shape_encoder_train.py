"""The device shape encoder's training path (shapemol_se_train_*, csrc/sm_shape_train.h): VN_DGCNN_Encoder.encode_train and
PointCloud_AE.get_autoencoder_train_loss.

Per case (B, N, layer_num, latent_dim) of shape_encoder_train_f64.CASES, with a fixed random upstream gradient: the latent passes the
head's stage gate next to ``forward``'s; the saved neighbour lists are the float64 oracle's; every parameter gradient satisfies
eH <= 4 e32 + 16 * 2^-24 against float64 autograd of the reference's form on the device's own neighbour lists (normalised by the
largest entry of the float64 tensor, e32 the float32 device-form error computed here, no element left out); a second run over
NaN-poisoned workspaces is bit-identical.  Staged: the same gate with the upstream gradient injected at hcat (conv_c skipped), for
block L - 1 alone.  Then: the device repack after an SGD step against a fresh context, the running statistics, the refusals.

Every case runs twice.  On the hash weights of synth: there float32 and float64 take different leaky-ReLU branches at a few of the 1e5 ..
1e7 elements whose cosine lies under its own rounding error (one flipped element moves a gradient by 1e-4 of its largest entry), so
both references are evaluated on the branches the DEVICE took, which its backward reports -- as they are on its neighbour lists; a
difference that comes from a branch then drops out and every element is gated.  And on the weights of
shape_encoder_train_f64.state_dict (directions aligned with the features), the only inputs with the cosine margin of 100
(tests/test_shape_encoder_train_cpu.py asserts it), where no branch can differ.  End to end: get_autoencoder_train_loss against the
reference's own loss.backward() (tests/golden/shape_encoder_train.npz).  Measured figures: profiles/shape_encoder_train/gate_results.md.
"""
import functools

import pytest
import torch

import shape_encoder_f64 as S
import shape_encoder_train_f64 as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RUNS = [(c, "generic") for c in TR.HASH] + [(c, "aligned") for c in TR.CASES]
IDS = ["-".join(map(str, c)) + "-" + k for c, k in RUNS]


def _encoder(L, LAT, kind="aligned"):
    import shapemol_amd
    enc = shapemol_amd.VN_DGCNN_Encoder(128, LAT, L, S.K)
    enc.load_state_dict(TR.state_dict(L, LAT, kind), strict=False)
    return enc.to(DEV)


@functools.lru_cache(maxsize=None)
def _run(case, kind="aligned"):
    """One forward and backward of the case on the device, and its float64 / float32 references (shared by the tests of the case)."""
    B, N, L, LAT = case
    sd, pts = TR.state_dict(L, LAT, kind), TR.points(B, N, (TR.CASES if kind == "aligned" else TR.HASH)[case])
    enc = _encoder(L, LAT, kind)
    x = pts.to(DEV)
    up = TR.upstream((B, LAT, 3))
    out, saved = enc._train_forward(x)
    raw = torch.full((L + 2, B * N, 256), -1, dtype=torch.int32, device=DEV)
    gw = enc._train_backward(saved, grad_out=up.float().to(DEV), masks=raw)
    idx, masks = saved["idx"].cpu(), TR.device_masks(raw.cpu(), L, LAT)
    r64, z64 = TR.reference_autograd(sd, pts, L, idx, S.F64, g_out=up, masks=masks)
    r32, _ = TR.device_form(sd, pts, L, idx, S.F32, g_out=up, masks=masks)
    return dict(enc=enc, sd=sd, pts=pts, x=x, up=up, out=out, saved=saved, gw=gw, idx=idx, r64=r64, r32=r32, z64=z64, masks=masks, raw=raw)


def _gates(dev, r32, r64, only=None):
    res = {k: S.gate(dev[k], r32[k], r64[k]) for k in r64 if only is None or k.startswith(only)}
    for k, (eh, e32, ok) in res.items():
        print(f"  {k}: eH {eh:.3e} e32 {e32:.3e} eH/bound {eh / (4 * e32 + 16 * S.U):.3f}")
    return res


@pytest.mark.parametrize("case,kind", RUNS, ids=IDS)
def test_latent_lists_and_gradients(case, kind):
    B, N, L, LAT = case
    r = _run(case, kind)
    sv = r["saved"]
    f64 = S.forward(r["sd"], r["pts"], L, S.F64)
    for l, stop in enumerate(f64["stops"]):
        assert torch.equal(r["idx"][l].long().sort(-1)[0], stop["idx"].sort(-1)[0]), f"neighbour lists of stage {l}"
    hcat = sv["hcat"].cpu().reshape(B * N, -1, 3)
    ev = lambda dt: S.head_stage(hcat, r["sd"]["conv_c.map_to_feat.weight"], r["sd"]["conv_c.map_to_dir.weight"],  # noqa: E731
                                 r["sd"]["conv_c.batchnorm.bn.weight"], r["sd"]["conv_c.batchnorm.bn.bias"], B, dt)[1]
    z32, z64 = ev(S.F32), ev(S.F64)
    assert S.gate(r["out"].cpu(), z32, z64)[2], "latent of encode_train"
    assert S.gate(r["enc"](r["x"]).cpu(), z32, z64)[2], "latent of forward"
    # the branches the device reports against the float64 evaluation's (they differ where dot is within rounding of zero: a cosine
    # near zero, or s = gamma xh + beta near zero); on the aligned weights none may differ
    _, i64 = TR.device_form(r["sd"], r["pts"], L, r["idx"], S.F64, g_out=r["up"])
    for k, neg in r["masks"].items():
        differ = neg != ~i64["masks"][k]
        print(f"  {k}: {int(differ.sum())} of {differ.numel()} branches differ from float64's")
        if kind == "aligned":
            assert not differ.any(), k
    dev = TR.unflatten(r["gw"].cpu(), r["sd"], L)
    res = _gates(dev, r["r32"], r["r64"])
    assert all(v[2] for v in res.values()), {k: v for k, v in res.items() if not v[2]}


@pytest.mark.parametrize("case,kind", RUNS, ids=IDS)
def test_bit_identical_over_poisoned_workspaces(case, kind):
    r = _run(case, kind)
    enc = r["enc"]
    poison = lambda: torch.full_like(enc._workspace(enc._context(DEV), case[0], case[1], r["x"].device), 0xFF)      # noqa: E731
    out, saved = enc._train_forward(r["x"], workspace=poison())
    gw = enc._train_backward(saved, grad_out=r["up"].float().to(DEV), workspace=poison())
    assert torch.equal(out, r["out"]) and torch.equal(gw, r["gw"])
    assert bool(torch.isfinite(gw).all())


@pytest.mark.parametrize("case,kind", RUNS, ids=IDS)
def test_staged_block_gate_from_hcat(case, kind):
    B, N, L, LAT = case
    r = _run(case, kind)
    uh = TR.upstream((B * N, L, 128, 3), seed=77)
    gw = r["enc"]._train_backward(r["saved"], grad_hcat=uh.float().to(DEV))
    dev = TR.unflatten(gw.cpu(), r["sd"], L)
    r64, _ = TR.reference_autograd(r["sd"], r["pts"], L, r["idx"], S.F64, g_hcat=uh, masks=r["masks"])
    r32, _ = TR.device_form(r["sd"], r["pts"], L, r["idx"], S.F32, g_hcat=uh, masks=r["masks"])
    res = _gates(dev, r32, r64, only=f"blocks.{L - 1}.")
    assert len(res) == 4 and all(v[2] for v in res.values()), res
    assert all(float(dev[k].abs().max()) == 0.0 for k in dev if k.startswith("conv_c."))


def test_encode_train_autograd_and_running_statistics():
    case = (3, 48, 2, 32)
    B, N, L, LAT = case
    r = _run(case)
    enc = _encoder(L, LAT)
    with pytest.raises(RuntimeError, match="must not require grad"):
        enc.encode_train(r["x"].clone().requires_grad_(True))
    enc.eval()
    before = {k: v.clone() for k, v in enc.state_dict().items() if "running" in k or "tracked" in k}
    z = enc.encode_train(r["x"][:, None])
    assert all(torch.equal(v, enc.state_dict()[k]) for k, v in before.items()), "eval() must leave the running statistics alone"
    (z * r["up"].float().to(DEV)).sum().backward()
    flat = torch.cat([p.grad.reshape(-1) for p in enc._params()])
    assert torch.equal(z.detach(), r["out"]) and torch.equal(flat, r["gw"])
    enc.train()
    enc.encode_train(r["x"])
    st = r["saved"]["stats"].cpu()
    for i, m in enumerate(enc._stages()):
        bn, cnt = m.batchnorm.bn, B * N * (S.K if i < L + 1 else 1)
        nch = bn.running_mean.numel()
        assert int(bn.num_batches_tracked) == 1
        torch.testing.assert_close(bn.running_mean.cpu().double(), 0.1 * st[i, 0, :nch], rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(bn.running_var.cpu().double(), 0.9 + 0.1 * st[i, 1, :nch] * cnt / (cnt - 1), rtol=1e-6, atol=1e-7)


def test_sgd_step_uses_the_device_repack_and_matches_a_fresh_context():
    case = (3, 48, 2, 32)
    B, N, L, LAT = case
    r = _run(case)
    enc = _encoder(L, LAT)
    opt = torch.optim.SGD(enc.parameters(), lr=1e-2)
    (enc.encode_train(r["x"]) * r["up"].float().to(DEV)).sum().backward()
    handle = enc._ctx.value
    opt.step()
    z = enc.encode_train(r["x"]).detach()
    assert enc._ctx.value == handle, "a changed parameter version must not build a new context"
    fresh = _encoder(L, LAT)
    fresh.load_state_dict(enc.state_dict())
    assert fresh._ctx is None
    assert torch.equal(fresh.encode_train(r["x"]).detach(), z)
    assert torch.equal(fresh(r["x"]), enc(r["x"]))
    assert not torch.equal(z, r["out"])


def test_debug_stop_after_is_the_frozen_forwards_alone():
    """The two paths share one sweep; shapemol_se_debug_stop_after belongs to shapemol_se_encode: the training forward stays full."""
    case = (3, 48, 2, 32)
    B, N, L, LAT = case
    r = _run(case)
    enc = _encoder(L, LAT)
    full = enc(r["x"])
    enc.debug_stop_after(DEV, 1)
    out, saved = enc._train_forward(r["x"])
    assert torch.equal(out, r["out"]), "the training forward must not stop early"
    for k in ("idx", "h0", "hcat", "pd"):
        assert torch.equal(saved[k], r["saved"][k]), k
    st, ref = saved["stats"], r["saved"]["stats"]          # (a stage writes its own channels: 128 of the edge stages, LAT of conv_c)
    assert torch.equal(st[:L + 1, :, :128], ref[:L + 1, :, :128]) and torch.equal(st[L + 1, :, :LAT], ref[L + 1, :, :LAT]), "stats"
    # forward honours the stop: the head has not run (the output is untouched) and the one neighbour list is block 0's, not block 1's
    from shapemol_amd import _lib
    from shapemol_amd._native import ptr, stream_ptr
    z = torch.full((B, LAT, 3), 7.0, device=DEV)
    _lib.check(_lib.load().shapemol_se_encode(enc._context(DEV), ptr(r["x"]), B, N, ptr(z), stream_ptr(r["x"].device)), "shapemol_se_encode")
    lists = torch.from_numpy(enc.debug_read(DEV, "idx", B * N)).sort(-1)[0]
    assert bool((z == 7.0).all()), "a stopped forward must leave the output alone"
    assert torch.equal(lists, r["idx"][1].sort(-1)[0]) and not torch.equal(lists, r["idx"][2].sort(-1)[0])
    enc.debug_stop_after(DEV, -1)
    assert torch.equal(enc(r["x"]), full)


def test_backward_of_a_graph_older_than_a_parameter_change():
    """Forward, an in-place change of every parameter, backward: the gradient is the one taken before the change (the node loads its
    own weights into the context), and the module then goes on with the changed ones."""
    case = (3, 48, 2, 32)
    B, N, L, LAT = case
    r = _run(case)
    enc = _encoder(L, LAT)
    up = r["up"].float().to(DEV)
    z = enc.encode_train(r["x"])
    with torch.no_grad():
        for p in enc.parameters():
            p.mul_(1.25)
    z2 = enc.encode_train(r["x"])                           # a second forward on the changed weights repacks the context
    (z * up).sum().backward()
    stale = torch.cat([p.grad.reshape(-1) for p in enc._params()])
    assert torch.equal(stale, r["gw"]), "the older graph's backward ran on the changed weights"
    enc.zero_grad(set_to_none=True)
    (z2 * up).sum().backward()
    moved = torch.cat([p.grad.reshape(-1) for p in enc._params()])
    fresh = _encoder(L, LAT)
    fresh.load_state_dict(enc.state_dict())
    (fresh.encode_train(r["x"]) * up).sum().backward()
    assert torch.equal(moved, torch.cat([p.grad.reshape(-1) for p in fresh._params()])) and not torch.equal(moved, stale)


def test_autoencoder_train_loss_against_the_references_backward():
    """get_autoencoder_train_loss(...).backward() on B = 3, N = 32, T = 50 against the reference's own loss.backward() gradients of the
    encoder keys (tests/golden/shape_encoder_train.npz): the same gate, e32 from the reference's float32 run against its float64 run."""
    import shapemol_amd
    from shapemol_amd import synth
    from util import golden
    g = golden("shape_encoder_train.npz")
    L, LAT = int(g["layers"]), int(g["latent_dim"])
    cfg = dict(encoder="VN_DGCNN", hidden_dim=int(g["hidden"]), latent_dim=LAT, layer_num=L, num_k=int(g["k"]), point_dim=3, loss_type="signeddist")
    ae = shapemol_amd.PointCloud_AE(cfg)
    ae.encoder.load_state_dict({k: torch.from_numpy(v) for k, v in synth.shape_encoder_state_dict(128, LAT, L, int(g["enc_seed"])).items()}, strict=False)
    ae.generator.load_state_dict({k: torch.from_numpy(v) for k, v in synth.shape_decoder_state_dict(128, LAT, L, int(g["dec_seed"])).items()}, strict=False)
    ae = ae.to(DEV)
    T = lambda k: torch.from_numpy(g[k]).to(DEV)      # noqa: E731
    loss = ae.get_autoencoder_train_loss(T("clouds"), T("q"), T("values"))
    loss.backward()
    assert abs(float(loss) - float(g["loss64"])) <= 4 * abs(float(g["loss"]) - float(g["loss64"])) + 16 * S.U * abs(float(g["loss64"]))
    sd = dict(ae.encoder.named_parameters())
    res = {}
    for k in g["enc_keys"]:
        g32 = torch.from_numpy(g["grad." + k]).double()
        res[k] = S.gate(sd[k].grad.cpu(), g32, g32 - torch.from_numpy(g["err." + k]).double())
        print(f"  {k}: eH {res[k][0]:.3e} e32 {res[k][1]:.3e} eH/bound {res[k][0] / (4 * res[k][1] + 16 * S.U):.3f}")
    assert all(v[2] for v in res.values()), {k: v for k, v in res.items() if not v[2]}


def test_autoencoder_train_loss_reaches_every_parameter():
    import shapemol_amd
    from shapemol_amd import synth
    cfg = dict(encoder="VN_DGCNN", hidden_dim=128, latent_dim=32, layer_num=2, num_k=20, point_dim=3, loss_type="signeddist")
    ae = shapemol_amd.PointCloud_AE(cfg)
    ae.encoder.load_state_dict(TR.state_dict(2, 32), strict=False)
    ae.generator.load_state_dict({k: torch.from_numpy(v) for k, v in synth.shape_decoder_state_dict(128, 32, 2).items()}, strict=False)
    ae = ae.to(DEV)
    pts = TR.points(3, 32, 5).to(DEV)
    q, v = TR.upstream((3, 50, 3), 9).float().to(DEV), TR.upstream((3, 50), 10).float().to(DEV)
    runs = []
    for _ in range(2):
        ae.zero_grad(set_to_none=True)
        loss = ae.get_autoencoder_train_loss(pts, q, v)
        loss.backward()
        runs.append([loss.detach().clone()] + [p.grad.clone() for p in ae.parameters()])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in ae.parameters())
    assert all(float(p.grad.abs().max()) > 0 for p in ae.encoder.parameters())
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    with pytest.raises(NotImplementedError, match="get_generator_train_loss"):
        ae.get_train_loss(pts, q, v)


def test_refusals_come_before_any_launch():
    from shapemol_amd._lib import ShapeMolLibraryError
    enc = _encoder(1, 7)
    for n in (16, 40):
        with pytest.raises(ShapeMolLibraryError, match=f"shapemol_se_train_forward: need .*N = {n}"):
            enc.encode_train(torch.zeros((1, n, 3), device=DEV))
    handle = enc._context(DEV)
    flat = enc._flat(enc._params())
    with pytest.raises(ShapeMolLibraryError, match="shapemol_se_load_weights: weight count mismatch"):
        enc._load_weights(handle, flat[:-1], torch.device(DEV))
    x = torch.zeros((1, 32, 3), device=DEV)
    with pytest.raises(ShapeMolLibraryError, match="workspace has 256 bytes"):
        enc._train_forward(x, workspace=torch.zeros(256, dtype=torch.uint8, device=DEV))
