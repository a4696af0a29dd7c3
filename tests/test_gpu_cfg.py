"""Classifier-free guidance on the device (the reference's sample_diffusion with guide_stren > 0,
models/molopt_score_model.py:616-642, threshold_CFG :116-151) against the reference's own chains
(tests/golden/make_golden_cfg.py) and a host recomposition of each step (tests/cfg_oracle.py).
Run on the GPU box:  pytest tests/test_gpu_cfg.py -m gpu"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import cfg_oracle as O  # noqa: E402
from util import T, golden, hash_noise, hip_model, maxabs, record, synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POS_TOL = 1e-4      # coordinates of a chain (as the other chain parity tests)
TRAJ_TOL = 2e-5     # raw predictions and logits of the recorded steps
STEP_TOL = 1e-5     # one step recomposed on the host from the chain's own state
TYPES = ("none", "reference_threshold", "dynamic_threshold", "rescale")


def _ttype(tag):
    return None if tag == "none" else tag


def _batch(B, seed, steps, C=15):
    bb = synth.synthetic_batch(B, seed=seed, num_classes=C)
    if C != 15:          # another vocabulary: every class, C - 1 included, among the atom types
        from vocab import all_classes
        bb["init_v"] = all_classes(len(bb["batch"]), C, 102, seed)
    eps, u = hash_noise(len(bb["batch"]), steps, seed, c=C)
    args = (T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1))
    return args, dict(num_steps=steps, center_pos_mode="none", noise=(T(eps, DEV), T(u, DEV)))


def _fixture(tag):
    c = golden(f"chain_cfg_{tag}.npz")
    args, kw = _batch(int(c["B"]), int(c["seed"]), int(c["S"]))
    p = float(c["p"])
    cfg = dict(threshold_type=_ttype(tag), threshold_args={} if np.isnan(p) else {"p": p},
               guide_stren=float(c["guide_stren"]), bounds=torch.from_numpy(c["bounds"]).float())
    return c, args, kw, cfg


@pytest.mark.parametrize("tag", TYPES)
def test_cfg_chain_golden(tag):
    """B = 4, 50 steps from t = 999 against the reference's chain with the recorded draws: atom types exact, positions
    within 1e-4, the raw conditional / unconditional predictions and the logits of the recorded steps within 2e-5 (1e-4 at
    the last step, after the chain's drift); graph replay and eager launches bit-identical."""
    m = hip_model(cond_mask_prob=0.1)
    c, args, kw, cfg = _fixture(tag)
    steps = c["traj_steps"]
    runs = []
    for use_graph in (True, False):
        r = m.sample_diffusion(*args, **kw, **cfg, use_graph=use_graph)
        runs.append(r)
        assert np.array_equal(r["v"].cpu().numpy(), c["v"])
        assert np.array_equal(torch.stack(r["v_traj"]).numpy(), c["v_traj"].astype(np.int64))
        errs = {"pos_end": maxabs(r["pos"], c["pos"])}
        for name in ("pos_traj", "pos_cond_traj", "pos_uncond_traj", "v0_traj", "vt_traj", "v_cond_traj", "v_uncond_traj"):
            got = torch.stack([r[name][int(s)].cpu() for s in steps]).numpy()
            e = [maxabs(got[i], c[name][i]) for i in range(len(steps))]
            errs[name] = max(e)
            assert max(e[:-1]) <= TRAJ_TOL, (name, e)
            assert e[-1] <= POS_TOL, (name, e)
        record("cfg_chain_golden", tag=tag, use_graph=use_graph, **errs)
        assert errs["pos_end"] <= POS_TOL
        assert len(r["pos_uncond_traj"]) == int(c["S"]) and len(r["v_uncond_traj"]) == int(c["S"])
    a, b = runs
    for k in ("pos", "v"):
        assert torch.equal(a[k], b[k])
    for k in ("pos_traj", "v0_traj", "vt_traj", "pos_cond_traj", "v_cond_traj", "pos_uncond_traj", "v_uncond_traj"):
        assert torch.equal(torch.stack(a[k]).cpu(), torch.stack(b[k]).cpu()), k


def test_cfg_threshold_type_error_before_launch():
    m = hip_model(cond_mask_prob=0.1)
    c, args, kw, cfg = _fixture("none")
    with pytest.raises(ValueError, match="undefined thresholding strategy"):
        m.sample_diffusion(*args, **kw, **dict(cfg, threshold_type="clip"))
    base = m.sample_diffusion(*args, **kw, **cfg)       # the context is unchanged
    assert np.array_equal(base["v"].cpu().numpy(), c["v"])


def test_cfg_off_is_the_unguided_chain():
    """guide_stren = 0 on a cond_mask_prob > 0 model is bit-identical to the same chain on a cond_mask_prob = 0 model, and a
    guided chain in between leaves no trace on the next unguided one."""
    m1, m0 = hip_model(cond_mask_prob=0.1), hip_model()
    _, args, kw, cfg = _fixture("rescale")
    ref = m0.sample_diffusion(*args, **kw)
    a = m1.sample_diffusion(*args, **kw, **dict(cfg, guide_stren=0))
    g = m1.sample_diffusion(*args, **kw, **cfg)
    b = m1.sample_diffusion(*args, **kw)
    for r in (a, b):
        assert torch.equal(r["pos"], ref["pos"]) and torch.equal(r["v"], ref["v"])
        assert torch.equal(torch.stack(r["v0_traj"]), torch.stack(ref["v0_traj"]))
        assert r["pos_uncond_traj"] == [] and r["v_uncond_traj"] == []
    assert maxabs(g["pos"], ref["pos"]) > 1e-3


def test_cfg_ignored_under_shape_guidance():
    """With a point cloud (or a mesh) given, the reference's if / elif never reaches CFG: bit-identical with and without
    guide_stren."""
    m = hip_model(cond_mask_prob=0.1)
    _, args, kw, cfg = _fixture("dynamic_threshold")
    cloud = synth.hash_normal((256, 3), 501, 3) * 2.0
    gk = dict(use_pointcloud_data=(cloud, None, 0.2), grad_step=990, seed=5)
    a = m.sample_diffusion(*args, **kw, **gk)
    b = m.sample_diffusion(*args, **kw, **gk, **cfg)
    assert torch.equal(a["pos"], b["pos"]) and torch.equal(a["v"], b["v"])
    assert b["pos_uncond_traj"] == []
    m_, c = golden("mesh_fixture.npz"), golden("chain_mesh_guided_b4_s20.npz")       # the mesh fixture's own chain
    args, kw = _batch(int(c["B"]), int(c["seed"]), int(c["S"]))
    mk = dict(use_mesh_data=((m_["verts"], m_["faces"]), m_["cloud"], None), grad_step=int(c["grad_step"]),
              guide_draws=T(c["draws"], DEV))
    a = m.sample_diffusion(*args, **kw, **mk)
    b = m.sample_diffusion(*args, **kw, **mk, **cfg)
    assert torch.equal(a["pos"], b["pos"]) and torch.equal(a["v"], b["v"])


def _cfg_stat(m):
    from shapemol_amd import _lib
    out = (C.c_float * 2)()
    n = _lib.load().shapemol_debug_read(m._context(torch.device(DEV)), b"cfg_stat", out, 8)
    assert n == 8
    return np.array([out[0], out[1]], dtype=np.float32)


@pytest.mark.parametrize("B,C", [(4, 15), (256, 15), (1024, 15), (4, 10), (4, 23)], ids=["4", "256", "1024", "4-c10", "4-c23"])
def test_cfg_quantile_equals_torch_quantile(B, C):
    """The device's radix-select quantile of the combined positions (N*3) and logits (N*C) of a step is torch.quantile's value
    bit for bit, at several p (ranks on both sides of a half weight, the ends); C = 10 and 23 change the number of logits, their
    quantile ranks and the block counts of the statistics kernels."""
    m = hip_model(cond_mask_prob=0.1, num_classes=C)
    args, kw = _batch(B, 21, 1, C)
    assert len(torch.unique(args[1])) == C
    for p in (0.995, 0.5, 0.3, 0.0, 1.0, 0.123456):
        r = m.sample_diffusion(*args, **kw, threshold_type="dynamic_threshold", threshold_args={"p": p}, guide_stren=0.7,
                               bounds=None)
        stat = _cfg_stat(m)
        got = []
        for i, (cn, un) in enumerate((("pos_cond_traj", "pos_uncond_traj"), ("v_cond_traj", "v_uncond_traj"))):
            x = O.combine(r[cn][0], r[un][0], 0.7)
            q = torch.quantile(x.reshape(-1), p).item()
            got.append((q, float(stat[i])))
            assert np.float32(q) == stat[i], (p, i, q, stat[i])
        record("cfg_quantile_exact", B=B, C=C, p=p, values=got)


def recomposed_step_errors(tag, B, S, seed, C=15, p=None, quantiles=None):
    """A CFG chain of S steps with every step recomposed on the host from the device chain's own state -- the model's forward
    with the shape and with zeros, the restated threshold_CFG (torch.quantile on the device), the posterior with the fed noise
    -- against the chain's v0_traj, vt_traj and positions: (worst absolute differences, atoms).  p: instead of the tag's own;
    quantiles: a list that receives every step's (positions', logits') host quantile (dynamic_threshold)."""
    m = hip_model(cond_mask_prob=0.1, num_classes=C)
    args, kw = _batch(B, seed, S, C)
    pos0, v0, batch, shape = args
    if p is None:
        p = {"none": None, "reference_threshold": 1.05, "dynamic_threshold": 0.99, "rescale": 0.6}[tag]
    targs = {} if p is None else {"p": p}
    box = np.array([[-3.0, 3.5], [-2.5, 3.0], [-3.5, 2.5]])
    r = m.sample_diffusion(*args, **kw, threshold_type=_ttype(tag), threshold_args=targs, guide_stren=1.5,
                           bounds=np.stack([box] * B))
    eps, u = kw["noise"]
    c0, ct, logvar = (m._table(k) for k in ("posterior_mean_c0_coef", "posterior_mean_ct_coef", "posterior_logvar"))
    worst = {"pos": 0.0, "v0": 0.0, "vt": 0.0}
    for s in range(S):
        t = 999 - s
        xt = pos0 if s == 0 else r["pos_traj"][s - 1].to(DEV)
        vt = v0 if s == 0 else r["v_traj"][s - 1].to(DEV)
        ts = torch.full((B,), t, dtype=torch.int64, device=DEV)
        pc = m(xt, vt, batch, shape, time_step=ts)
        pu = m(xt, vt, batch, torch.zeros_like(shape), time_step=ts)
        gp = O.combine(pc["pred_ligand_pos"], pu["pred_ligand_pos"], 1.5)
        gv = O.combine(pc["pred_ligand_v"], pu["pred_ligand_v"], 1.5)
        if tag == "dynamic_threshold":       # the statistic exactly as the reference takes it (torch.quantile on the device)
            sp, sv = torch.quantile(gp.reshape(-1), p), torch.quantile(gv.reshape(-1), p)
            if quantiles is not None:
                quantiles.append((sp.item(), sv.item()))
            gp = torch.minimum(torch.maximum(gp, -sp), sp)
            gv = torch.minimum(torch.maximum(gv, -sv), sv)
            bx = torch.as_tensor(box, dtype=torch.float32, device=DEV)
            gp = torch.minimum(torch.maximum(gp, bx[:, 0]), bx[:, 1])
        else:
            gp = O.threshold_cfg(gp, pc["pred_ligand_pos"], _ttype(tag), targs, box)
            gv = O.threshold_cfg(gv, pc["pred_ligand_v"], _ttype(tag), targs, None)
        xn = c0[t] * gp + ct[t] * xt + (torch.exp(0.5 * logvar[t]) if t else 0.0) * eps[s]
        lv0 = torch.log_softmax(gv, dim=-1)
        lvt = torch.log(torch.nn.functional.one_hot(vt, m.num_classes).float().clamp(min=1e-30))
        lp = m._q_v_posterior(lv0, lvt, ts, batch)
        worst["pos"] = max(worst["pos"], maxabs(xn, r["pos_traj"][s]))
        worst["v0"] = max(worst["v0"], maxabs(lv0, r["v0_traj"][s]))
        worst["vt"] = max(worst["vt"], maxabs(lp, r["vt_traj"][s]))
    return worst, int(len(batch))


@pytest.mark.parametrize("tag", TYPES)
def test_cfg_step_recomposed_at_size(tag):
    """B = 256 (about 5.5k atoms), 10 steps: every step recomposed on the host (recomposed_step_errors)."""
    worst, n = recomposed_step_errors(tag, 256, 10, 31)
    record("cfg_step_recomposed_at_size", tag=tag, n=n, **worst)
    assert worst["pos"] <= STEP_TOL and worst["v0"] <= STEP_TOL and worst["vt"] <= STEP_TOL, worst


def test_cfg_step_recomposed_negative_quantile():
    """dynamic_threshold with p = 0.02 at B = 4, 3 steps: the quantile of both tensors is negative in every step, so clip(x, -s, s)
    has -s > s and collapses every value to s, as torch.clamp with min > max does -- cfg_apply (sm_cfg.h) with a negative
    statistic, recomposed on the host like the steps above."""
    quantiles = []
    worst, n = recomposed_step_errors("dynamic_threshold", 4, 3, 31, p=0.02, quantiles=quantiles)
    record("cfg_step_recomposed_negative_quantile", n=n, quantiles=quantiles, **worst)
    assert len(quantiles) == 3 and all(sp < 0 and sv < 0 for sp, sv in quantiles), quantiles
    assert worst["pos"] <= STEP_TOL and worst["v0"] <= STEP_TOL and worst["vt"] <= STEP_TOL, worst


def test_cfg_driver_matches_model():
    """sample_diffusion_ligand forwards guide_stren, threshold_CFG and the per-batch bounds to the model: every batch's result
    equals model.sample_diffusion called by hand with the arguments the driver passed (recorded), and differs from the
    unguided run of the same draws."""
    from shapemol_amd.sampling import sample_diffusion_ligand
    m = hip_model(cond_mask_prob=0.1)
    shape_emb = torch.from_numpy(synth.synthetic_batch(1, seed=3)["shape"].reshape(-1, 3).astype(np.float32))
    kw = dict(num_steps=6, center_pos_mode="none", threshold_type="rescale", threshold_args={"p": 0.7}, guide_stren=1.0,
              bounds=np.array([[[-2.0, 2.0]] * 3] * 3), sample_num_atoms="ref", ref_num_atoms=12)
    seen = []
    real = type(m).sample_diffusion

    def spy(self, *a, **k):
        seen.append(({n: (v.clone() if torch.is_tensor(v) else v) for n, v in k.items()}))
        return real(self, *a, **k)
    torch.manual_seed(4); np.random.seed(4)
    m.sample_diffusion = spy.__get__(m)
    try:
        out = sample_diffusion_ligand(m, shape_emb, 6, batch_size=3, host_rng=True, **kw)
    finally:
        del m.sample_diffusion
    torch.manual_seed(4); np.random.seed(4)
    plain = sample_diffusion_ligand(m, shape_emb, 6, batch_size=3, host_rng=True, **dict(kw, guide_stren=0))
    assert len(seen) == 2
    for i, k in enumerate(seen):
        assert k["guide_stren"] == 1.0 and k["threshold_type"] == "rescale" and k["bounds"] is kw["bounds"]
        k = {n: v for n, v in k.items() if not n.startswith("_")}
        r = m.sample_diffusion(**k)
        got = r["pos"].cpu().numpy().astype(np.float64)
        want = np.concatenate(out[0][3 * i:3 * i + 3])
        assert np.array_equal(got, want)
        assert np.array_equal(r["v"].cpu().numpy(), np.concatenate(out[1][3 * i:3 * i + 3]))
    assert not np.array_equal(np.concatenate(out[0]), np.concatenate(plain[0]))
