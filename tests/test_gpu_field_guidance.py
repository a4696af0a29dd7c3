"""The shape decoder's value-and-gradient kernel (shapemol_field_decode_grad, csrc/sm_shape_dec_grad.h) and the gradient shape
guidance built on it (shapemol_field_guide, shapemol_set_field_guidance; the reference's `use_grad` branch,
models/molopt_score_model.py:592-615) against float64 (tests/shape_decoder_grad_f64.py) under the project's gate
eH <= 4 e32 + 16 * 2^-24 on the non-fragile points, and inside the sampling chain against a float64-guided oracle chain."""
import functools

import numpy as np
import pytest
import torch

import shape_decoder_f64 as D
import shape_decoder_grad_f64 as DG
from util import T, hip_model, maxabs, oracle_model, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POS_TOL = 1e-4          # coordinates of a chain (as the other chain parity tests)


@functools.lru_cache(maxsize=None)
def _decoder(L=4, Z=32, loss_type="signeddist"):
    from shapemol_amd.shape_autoencoder import DecoderInner
    dec = DecoderInner(3, Z, 128, L, loss_type)
    dec.load_state_dict(D.state_dict(L, Z), strict=True)
    return dec.to(DEV)


def _gates(name, dec, out, grad, p, s, z, ref=None):
    """Gate a device value and gradient against float64; the fragile cap is asserted first, from the float64 data alone."""
    sd = D.state_dict(dec.layer_num, dec.z_dim)
    ref = ref or DG.reference(sd, p, s, z, dec.layer_num, dec.loss_type)
    n = len(ref["keep"])
    assert DG.cap_ok(ref["fragile"]), f"{name}: {int(ref['fragile'].sum())} of {n} points fragile"
    out, grad = out.cpu().reshape(-1), grad.cpu().reshape(-1, 3)
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(out).all()), name
    eo, e32o, oko = D.gate(out, ref["out32"], ref["out64"])
    eg, e32g, okg = DG.grad_gate(grad, ref)
    print(f"{name}: out eH {eo:.3e} e32 {e32o:.3e} | grad eH {eg:.3e} e32 {e32g:.3e} bound {D.bound(e32g):.3e} "
          f"left out {int(ref['fragile'].sum())}/{n} {'ok' if oko and okg else 'FAIL'}")
    return oko and okg


def _dense(dec, B, Tn, seed, **kw):
    p, s, z = D.inputs(B, Tn, dec.z_dim, seed, **kw)
    out, grad = dec.decode_grad(p.view(B, Tn, 3).to(DEV), z.to(DEV))
    assert tuple(out.shape) == (B, Tn) and tuple(grad.shape) == (B, Tn, 3)
    return out, grad, p, s, z


# 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_type", ("signeddist", "occupancy"))
def test_fixture_parity(loss_type):
    """out, the gradient and the updated positions of the reference's own DecoderInner and autograd (float32, CPU)."""
    g = np.load(DG.GOLDEN)
    dec = _decoder(int(g["layers"]), int(g["latent_dim"]), loss_type)
    p, s, z = torch.from_numpy(g["p"]), torch.from_numpy(g["batch"]), torch.from_numpy(g["z"])
    sd = D.state_dict(dec.layer_num, dec.z_dim)
    ref = DG.reference(sd, p, s, z, dec.layer_num, loss_type)
    assert DG.cap_ok(ref["fragile"])
    k = ref["keep"]
    out, grad = dec.decode_atoms_grad(p.to(DEV), s.to(DEV), z.to(DEV))
    assert _gates("fixture " + loss_type, dec, out, grad, p, s, z, ref)
    # against the reference's own float32 numbers: its error is the e32 of the gate
    lr = float(g["grad_lr"])
    eo, e32o, oko = D.gate(out.cpu(), g["out_" + loss_type], ref["out64"])
    assert oko, (eo, e32o)
    # the reference's gradient is that of the clipped mean: (1[d < 0.5] / T_j) grad
    cnt = torch.bincount(s)[s].double()
    w64 = ((ref["out64"] < 0.5).double() / cnt)[:, None] * ref["grad64"]
    wdev = ((out.cpu() < 0.5).float() / cnt.float())[:, None] * grad.cpu()
    eg = D.rel_err(wdev[k].numpy(), w64[k].numpy())
    e32 = D.rel_err(g["grad_" + loss_type][k.numpy()], w64[k].numpy())
    print(f"fixture {loss_type} clipped-mean grad: eH {eg:.3e} e32 {e32:.3e}")
    assert eg <= D.bound(e32)
    new64 = DG.guide(p, ref["out64"], ref["grad64"], s, z.shape[0], lr)
    new = dec.guide_atoms(p.to(DEV), s.to(DEV), z.to(DEV), lr).cpu()
    ep = D.rel_err(new[k].numpy(), new64[k].numpy())
    e32p = D.rel_err(g["pos_" + loss_type][k.numpy()], new64[k].numpy())
    print(f"fixture {loss_type} update: eH {ep:.3e} e32 {e32p:.3e}")
    assert ep <= D.bound(e32p)


# 2 ------------------------------------------------------------------------------------------------------------------------
def test_tile_edges():
    dec, tile = _decoder(), _decoder().tile(DEV)
    gt = dec.grad_tile(DEV)
    assert gt >= 16 and gt % 16 == 0 and tile % gt == 0      # every edge of the decode tile is one of the gradient kernel's
    oks = []
    for Tn in (1, 15, 16, 17, tile - 1, tile, tile + 1, 2 * tile + 1):
        out, grad, p, s, z = _dense(dec, 2, Tn, DG.edge_seed(Tn))
        oks.append(_gates(f"T={Tn}", dec, out, grad, p, s, z))
    assert all(oks)


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_launch_tails():
    """Totals around one and two decode tiles per compute unit (two and four of the gradient kernel's): the last workgroup's
    tail and the first extra iteration; both shapes inside every tile."""
    dec, tile = _decoder(), _decoder().tile(DEV)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    p, s, z, totals = DG.tail_case(cus, tile)
    ref = DG.reference(D.state_dict(4, 32), p, s, z, 4, "signeddist")
    pd, sdv, zd = p.to(DEV), s.to(DEV), z.to(DEV)
    oks = []
    for n in totals:
        out, grad = dec.decode_atoms_grad(pd[:n], sdv[:n], zd)
        assert out.shape == (n,) and grad.shape == (n, 3)
        sub = DG.prefix(ref, n)                                 # (the fragile set of the n points, maxima over those n)
        oks.append(_gates(f"n={n}", dec, out, grad, p[:n], s[:n], z, sub))
    assert all(oks)


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_bit_equality():
    """The value is the decode kernel's; a point's result depends neither on the other points nor on the launch."""
    dec, tile = _decoder(), _decoder().tile(DEV)
    B, Tn = 5, tile // 2 + 3
    p, s, z = D.inputs(B, Tn, dec.z_dim, 57)
    pd, sdv, zd = p.to(DEV), s.to(DEV), z.to(DEV)
    out, grad = dec.decode_grad(pd.view(B, Tn, 3), zd)
    assert torch.equal(out, dec(pd.view(B, Tn, 3), zd))
    out2, grad2 = dec.decode_grad(pd.view(B, Tn, 3), zd)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)
    fo, fg = dec.decode_atoms_grad(pd, sdv, zd)
    assert torch.equal(fo, out.reshape(-1)) and torch.equal(fg, grad.reshape(-1, 3))
    perm = torch.from_numpy(np.random.RandomState(3).permutation(B * Tn)).to(DEV)
    so, sg = dec.decode_atoms_grad(pd[perm], sdv[perm], zd)
    bo, bg = torch.empty_like(so), torch.empty_like(sg)
    bo[perm], bg[perm] = so, sg
    assert torch.equal(bo, fo) and torch.equal(bg, fg)
    occ = _decoder(4, 32, "occupancy")
    oo, _ = occ.decode_grad(pd.view(B, Tn, 3), zd)
    assert torch.equal(oo, occ(pd.view(B, Tn, 3), zd))


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,Z,loss_type", ((1, 32, "signeddist"), (8, 32, "signeddist"), (4, 1, "signeddist"), (4, 256, "signeddist"),
                                          (4, 32, "occupancy"), (8, 256, "occupancy")))
def test_sizes_and_loss_type(L, Z, loss_type):
    dec = _decoder(L, Z, loss_type)
    out, grad, p, s, z = _dense(dec, 3, 50, DG.SIZE_SEEDS[(L, Z, loss_type)], z_scale=DG.size_z_scale(Z))
    assert torch.equal(out, dec(p.view(3, 50, 3).to(DEV), z.to(DEV)))
    assert _gates(f"L={L} Z={Z} {loss_type}", dec, out, grad, p, s, z)


# 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("ragged5", "small40"))
@pytest.mark.parametrize("loss_type", ("signeddist", "occupancy"))
def test_guide_atoms(kind, loss_type):
    """The stand-alone update against float64, with a grad_lr at which the update is a quarter of the positions' size."""
    dec = _decoder(4, 32, loss_type)
    counts = DG.ragged_counts(kind)
    p, s, z = D.inputs(len(counts), counts, dec.z_dim, 31)
    sd = D.state_dict(4, 32)
    ref = DG.reference(sd, p, s, z, 4, loss_type)
    assert DG.cap_ok(ref["fragile"])
    unit = DG.guide(p, ref["out64"], ref["grad64"], s, len(counts), 1.0) - p.double()
    assert float(unit.abs().max()) > 0
    lr = 0.25 * float(p.abs().max()) / float(unit.abs().max())
    new64 = DG.guide(p, ref["out64"], ref["grad64"], s, len(counts), lr)
    assert float((new64 - p.double()).abs().max()) >= 0.25 * float(p.abs().max()) * (1 - 1e-9)
    new32 = DG.guide(p, ref["out32"], ref["grad32"], s, len(counts), lr)
    pd = p.to(DEV)
    keep0 = pd.clone()
    new = dec.guide_atoms(pd, s.to(DEV), z.to(DEV), lr)
    assert torch.equal(pd, keep0) and new.data_ptr() != pd.data_ptr()
    k = ref["keep"]
    eh, e32 = D.rel_err(new.cpu()[k].numpy(), new64[k].numpy()), D.rel_err(new32[k].numpy(), new64[k].numpy())
    print(f"guide_atoms {kind} {loss_type}: lr {lr:.3g} eH {eh:.3e} e32 {e32:.3e} bound {D.bound(e32):.3e}")
    assert bool(torch.isfinite(new).all())
    assert eh <= D.bound(e32)
    stay = (ref["out64"] >= 0.5 + 1e-3)
    assert torch.equal(new.cpu()[stay], p[stay])           # atoms outside the clip do not move


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_autograd_function():
    """field(p, z).clamp(max=0.5).sub(0.5).mean() differentiated per molecule, as the reference's block: the same update."""
    dec = _decoder()
    counts = DG.ragged_counts("ragged5")
    p, s, z = D.inputs(len(counts), counts, dec.z_dim, 31)
    sd = D.state_dict(4, 32)
    ref = DG.reference(sd, p, s, z, 4, "signeddist")
    lr = 2.0
    new64 = DG.guide(p, ref["out64"], ref["grad64"], s, len(counts), lr)
    new32 = DG.guide(p, ref["out32"], ref["grad32"], s, len(counts), lr)
    pd, zd = p.to(DEV), z.to(DEV)
    got = pd.clone()
    for j in range(len(counts)):
        idx = torch.where(s == j)[0].to(DEV)
        q = pd[idx].unsqueeze(0).clone().requires_grad_(True)
        d = dec.field(q, zd[j:j + 1]).clamp(max=0.5).sub(0.5)
        g, = torch.autograd.grad(d.mean(), q)
        got[idx] = (q.detach() - lr * d.detach().unsqueeze(2) * g)[0]
    k = ref["keep"]
    eh, e32 = D.rel_err(got.cpu()[k].numpy(), new64[k].numpy()), D.rel_err(new32[k].numpy(), new64[k].numpy())
    print(f"autograd: eH {eh:.3e} e32 {e32:.3e}")
    assert eh <= D.bound(e32)
    direct = dec.guide_atoms(pd, s.to(DEV), zd, lr)
    assert D.rel_err(got.cpu()[k].numpy(), direct.cpu()[k].numpy()) <= 16 * D.U
    with pytest.raises(RuntimeError, match="p only"):
        dec.field(pd.view(1, -1, 3), zd[:1].clone().requires_grad_(True))
    q = pd[:4].view(1, 4, 3).clone().requires_grad_(True)
    g, = torch.autograd.grad(dec.field(q, zd[:1]).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# 8 ------------------------------------------------------------------------------------------------------------------------
CHAIN_B, CHAIN_STEPS, CHAIN_LR = DG.CHAIN_B, DG.CHAIN_STEPS, DG.CHAIN_LR


def _chain_args(bb, eps, u):
    args = (T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(CHAIN_B, -1))
    return args, dict(num_steps=CHAIN_STEPS, center_pos_mode="none", noise=(T(eps, DEV), T(u, DEV)))


def test_chain():
    """20 steps, 10 of them guided: types exact, positions within 1e-4 of the float64-guided oracle chain; graph replay and
    eager launches bit-identical; grad_step >= T - 1 is the unguided chain."""
    m, dec = hip_model(), _decoder()
    sd, dm, _cfg, _ = oracle_model()
    bb, eps, u = DG.chain_inputs(DG.CHAIN_SEED)
    grad_step = dm.T - 1 - 10                                         # t = T-1 .. T-10 guided, the ten below not
    pos, v, preds, least = DG.oracle_chain(bb, eps, u, CHAIN_LR, grad_step)
    pos0, v0, _, _ = DG.oracle_chain(bb, eps, u, None, 0)
    assert maxabs(pos, pos0) > 1e-3                                   # the guidance matters
    assert least >= 2.0 ** -21, least                                 # no device mask flip can occur
    args, kw = _chain_args(bb, eps, u)
    runs = [m.sample_diffusion(*args, **kw, use_grad=True, shape_AE=dec, grad_lr=CHAIN_LR, grad_step=grad_step, use_graph=ug) for ug in (True, False)]
    for r in runs:
        assert np.array_equal(r["v"].cpu().numpy(), v.numpy())
        e = maxabs(r["pos"], pos)
        ec = max(maxabs(r["pos_cond_traj"][i], preds[i]) for i in range(CHAIN_STEPS))
        print(f"chain: pos {e:.3e} guided predictions {ec:.3e}")
        assert e <= POS_TOL and ec <= POS_TOL
    a, b = runs
    assert torch.equal(a["pos"], b["pos"]) and torch.equal(a["v"], b["v"])
    assert torch.equal(torch.stack(a["pos_cond_traj"]), torch.stack(b["pos_cond_traj"]))
    plain = m.sample_diffusion(*args, **kw)
    off = m.sample_diffusion(*args, **kw, use_grad=True, shape_AE=dec, grad_lr=CHAIN_LR, grad_step=dm.T - 1)
    assert torch.equal(off["pos"], plain["pos"]) and torch.equal(off["v"], plain["v"])
    assert maxabs(a["pos"], plain["pos"]) > 1e-3
    again = m.sample_diffusion(*args, **kw)                           # a guided chain leaves no trace on the context
    assert torch.equal(again["pos"], plain["pos"])


def test_chain_follows_the_decoder():
    """A captured step holds the decoder's device memory.  New weights in the same module (a new library context, often at the
    old one's host address) and a grown per-shape workspace must both be seen: each chain equals the eager one of a fresh
    decoder in that state."""
    from shapemol_amd.shape_autoencoder import DecoderInner
    m = hip_model()
    sd, dm, _cfg, _ = oracle_model()
    bb, eps, u = DG.chain_inputs(DG.CHAIN_SEED)
    args, kw = _chain_args(bb, eps, u)
    gk = dict(use_grad=True, grad_lr=CHAIN_LR, grad_step=dm.T - 1 - 10)

    def fresh(seed):
        d = DecoderInner(3, 32, 128, 4, "signeddist")
        d.load_state_dict(D.state_dict(4, 32, seed=seed), strict=True)
        return d.to(DEV)
    dec = fresh(19)
    a = m.sample_diffusion(*args, **kw, **gk, shape_AE=dec)                       # captures
    # a decode with more shapes than the chain's: the workspace moves
    p, _, z = D.inputs(CHAIN_B + 5, 3, 32, 77)
    dec(p.view(CHAIN_B + 5, 3, 3).to(DEV), z.to(DEV))
    b = m.sample_diffusion(*args, **kw, **gk, shape_AE=dec)
    assert torch.equal(a["pos"], b["pos"]) and torch.equal(a["v"], b["v"])
    ref_a = m.sample_diffusion(*args, **kw, **gk, shape_AE=fresh(19), use_graph=False)
    assert torch.equal(a["pos"], ref_a["pos"])
    # other weights in the same module
    dec.load_state_dict({k: v.to(DEV) for k, v in D.state_dict(4, 32, seed=23).items()}, strict=True)
    c = m.sample_diffusion(*args, **kw, **gk, shape_AE=dec)
    ref_c = m.sample_diffusion(*args, **kw, **gk, shape_AE=fresh(23), use_graph=False)
    assert torch.equal(c["pos"], ref_c["pos"]) and torch.equal(c["v"], ref_c["v"])
    assert maxabs(c["pos"], a["pos"]) > 1e-4                                      # the weights matter


# 9 ------------------------------------------------------------------------------------------------------------------------
def test_multi_conditions():
    """Two conditions in one chain are the two conditions run alone, molecule by molecule (evaluation-mode batch norm: molecules
    are independent)."""
    from shapemol_amd.sampling import sample_diffusion_ligand_multi
    m, dec = hip_model(), _decoder()
    was_training = m.training
    m.eval()
    try:
        shapes = synth.synthetic_batch(2, seed=5)["shape"].reshape(2, 32, 3)
        conds = [(shapes[0], None), (shapes[1], None)]
        kw = dict(num_steps=6, sample_num_atoms="ref", host_rng=True, grad_step=0, use_grad=True, grad_lr=CHAIN_LR, shape_AE=dec,
                  device=DEV)

        def run(cs, refs):
            np.random.seed(3)
            torch.manual_seed(3)
            return sample_diffusion_ligand_multi(m, cs, 2, batch_size=4, ref_num_atoms=refs, **kw)
        both = run(conds, [6, 7])
        plain = sample_diffusion_ligand_multi(m, conds, 2, batch_size=4, ref_num_atoms=[6, 7], **dict(kw, use_grad=False))
        assert any(not np.array_equal(a, b) for a, b in zip(both[0][0] + both[1][0], plain[0][0] + plain[1][0]))
        # the same per-molecule random numbers: each condition alone, fed the slice of the draws it had in the mixed chain
        n0, n1 = 2 * 6, 2 * 7
        np.random.seed(3)
        torch.manual_seed(3)
        init = torch.randn(n0 + n1, 3)
        state = torch.get_rng_state()
        for c, (lo, hi) in enumerate(((0, n0), (n0, n0 + n1))):
            bl = torch.repeat_interleave(torch.arange(2), torch.tensor([hi - lo]) // 2).to(DEV)
            torch.set_rng_state(state)
            from shapemol_amd.sampling import _host_noise, _initial_types
            v_all = _initial_types(m, n0 + n1, DEV, True)
            noise = _host_noise(m, 6, n0 + n1, DEV, True)
            r = m.sample_diffusion(init[lo:hi].to(DEV), v_all[lo:hi], bl, torch.from_numpy(shapes[c]).reshape(1, -1).repeat(2, 1).to(DEV),
                                   num_steps=6, center_pos_mode="none", noise=(noise[0][:, lo:hi].contiguous(), noise[1][:, lo:hi].contiguous()),
                                   use_grad=True, grad_lr=CHAIN_LR, shape_AE=dec, grad_step=0)
            per = (hi - lo) // 2
            for k in range(2):
                assert np.array_equal(r["pos"][k * per:(k + 1) * per].cpu().numpy().astype(np.float64), both[c][0][k])
                assert np.array_equal(r["v"][k * per:(k + 1) * per].cpu().numpy(), both[c][1][k])
    finally:
        m.train(was_training)


# 10 -----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_precedence():
    import ctypes as C
    from shapemol_amd import _lib
    from shapemol_amd.shape_autoencoder import DecoderInner, PointCloud_AE
    m, dec = hip_model(), _decoder()
    lib = _lib.load()
    bb, eps, u = DG.chain_inputs(DG.CHAIN_SEED)
    args, kw = _chain_args(bb, eps, u)
    with pytest.raises(ValueError, match="shape_AE"):
        m.sample_diffusion(*args, **kw, use_grad=True)
    with pytest.raises(TypeError, match="shapemol_amd.shape_autoencoder.PointCloud_AE"):
        m.sample_diffusion(*args, **kw, use_grad=True, shape_AE=torch.nn.Linear(3, 3))
    with pytest.raises(ValueError, match="grad_lr"):
        m.sample_diffusion(*args, **kw, use_grad=True, shape_AE=dec, grad_lr=float("nan"))
    with pytest.raises(_lib.ShapeMolLibraryError, match="shape_dim"):
        m.sample_diffusion(*args, **kw, use_grad=True, shape_AE=_decoder(4, 1))
    ctx = m._context(torch.device(DEV))
    assert lib.shapemol_set_field_guidance(ctx, dec._context(DEV), float("inf"), 0) != 0
    assert b"finite" in lib.shapemol_last_error()
    assert lib.shapemol_set_field_guidance(ctx, None, 0.0, 0) == 0
    # PointCloud_AE: its generator is used
    cfg = dict(encoder="VN_DGCNN", hidden_dim=128, latent_dim=32, layer_num=4, num_k=20, point_dim=3, loss_type="signeddist")
    ae = PointCloud_AE(cfg)
    ae.generator.load_state_dict(D.state_dict(4, 32), strict=True)
    ae = ae.to(DEV)
    gs = 1000 - 1 - 10
    a = m.sample_diffusion(*args, **kw, use_grad=True, shape_AE=ae, grad_lr=CHAIN_LR, grad_step=gs)
    b = m.sample_diffusion(*args, **kw, use_grad=True, shape_AE=dec, grad_lr=CHAIN_LR, grad_step=gs)
    assert torch.equal(a["pos"], b["pos"])
    # precedence: a point cloud wins over use_grad (silently, shape_AE is not even looked at), use_grad over CFG
    cloud = (synth.hash_normal((64, 3), 71, 3) * 2.0).astype(np.float64)
    pc = dict(use_pointcloud_data=(cloud, None, 0.5), grad_step=gs, seed=9)
    c1 = m.sample_diffusion(*args, **kw, **pc)
    c2 = m.sample_diffusion(*args, **kw, **pc, use_grad=True, shape_AE=None)
    assert torch.equal(c1["pos"], c2["pos"])
    # a mesh wins over use_grad too
    from util import golden
    cm, mf = golden("chain_mesh_guided_b4_s20.npz"), golden("mesh_fixture.npz")
    bm = synth.synthetic_batch(int(cm["B"]), seed=int(cm["seed"]))
    from util import hash_noise
    em, um = hash_noise(len(bm["batch"]), int(cm["S"]), int(cm["seed"]))
    margs = (T(bm["init_pos"], DEV), T(bm["init_v"], DEV), T(bm["batch"], DEV), T(bm["shape"], DEV).view(int(cm["B"]), -1))
    mkw = dict(num_steps=int(cm["S"]), center_pos_mode="none", noise=(T(em, DEV), T(um, DEV)), grad_step=int(cm["grad_step"]),
               use_mesh_data=((mf["verts"], mf["faces"]), mf["cloud"], None), guide_draws=T(cm["draws"], DEV))
    m1 = m.sample_diffusion(*margs, **mkw)
    m2 = m.sample_diffusion(*margs, **mkw, use_grad=True, shape_AE=None)
    assert torch.equal(m1["pos"], m2["pos"]) and maxabs(m1["pos"], cm["pos"]) < POS_TOL
    mc = hip_model(cond_mask_prob=0.1)
    f1 = mc.sample_diffusion(*args, **kw, use_grad=True, shape_AE=dec, grad_lr=CHAIN_LR, grad_step=gs)
    f2 = mc.sample_diffusion(*args, **kw, use_grad=True, shape_AE=dec, grad_lr=CHAIN_LR, grad_step=gs, guide_stren=2.0, threshold_type="none")
    assert torch.equal(f1["pos"], f2["pos"]) and f2["pos_uncond_traj"] == []
    # the C entry points' own refusals
    z = torch.zeros((1, 32, 3), device=DEV)
    p = torch.zeros((4, 3), device=DEV)
    g = torch.zeros((4, 3), device=DEV)
    sdc = dec._context(DEV)
    vp = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    assert lib.shapemol_field_decode_grad(sdc, vp(p), None, 4, 3, vp(z), 1, None, vp(g), None) != 0
    assert b"points_per_shape" in lib.shapemol_last_error()
    assert lib.shapemol_field_decode_grad(sdc, vp(p), None, 4, 4, vp(z), 0, None, vp(g), None) != 0
    assert lib.shapemol_field_decode_grad(sdc, vp(p), None, 4, 4, vp(z), 1, None, None, None) != 0
    assert lib.shapemol_field_decode_grad(sdc, vp(p), None, 0, 0, vp(z), 1, None, None, None) == 0
    bt = torch.zeros(4, dtype=torch.int64, device=DEV)
    assert lib.shapemol_field_guide(sdc, vp(p), vp(bt), 4, vp(z), 1, float("nan"), None) != 0
    assert lib.shapemol_field_guide(sdc, vp(p), vp(bt), 4, vp(z), 0, 1.0, None) != 0
    with pytest.raises(ValueError, match="sorted"):
        dec.guide_atoms(p, torch.tensor([1, 0, 0, 0], device=DEV), torch.zeros((2, 32, 3), device=DEV), 1.0)
    with pytest.raises(ValueError, match="finite"):
        dec.guide_atoms(p, bt, z, float("inf"))
    with pytest.raises(ValueError, match=r"\(B, T, 3\)"):
        dec.decode_grad(p, z)
    with pytest.raises(ValueError, match="must lie in"):
        dec.decode_atoms_grad(p, bt + 1, z)
    with pytest.raises(RuntimeError, match="HIP device"):
        dec.decode_grad(p.cpu().view(1, 4, 3), z)

