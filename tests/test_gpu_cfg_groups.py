"""Classifier-free guidance with one strength, one threshold statistic and one box per group of molecules on the device:
sample_diffusion(guide_stren=[(w, n_mols), ...]), shapemol_set_cfg_groups and sample_diffusion_ligand_multi against the
reference's per-group chains (tests/golden/make_golden_cfg_groups.py), against the scalar form on each group's slice, and
against a host recomposition of each step.  Run on the GPU box:  pytest tests/test_gpu_cfg_groups.py -m gpu"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import cfg_groups_oracle as GO  # noqa: E402
import cfg_oracle as O  # noqa: E402
from util import T, golden, hash_noise, hip_model, maxabs, model_cfg, record, synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POS_TOL = 1e-4      # the tolerances of tests/test_gpu_cfg.py
TRAJ_TOL = 2e-5
STEP_TOL = 1e-5
TYPES = ("none", "reference_threshold", "dynamic_threshold", "rescale")
P = {"none": None, "reference_threshold": 1.05, "dynamic_threshold": 0.99, "rescale": 0.6}
TRAJS = ("pos_traj", "v0_traj", "vt_traj", "pos_cond_traj", "v_cond_traj", "pos_uncond_traj", "v_uncond_traj")
BOXES3 = np.array([[[-2.0, 2.5], [-1.5, 2.0], [-2.5, 1.5]], [[-3.0, 3.5], [-2.5, 3.0], [-3.5, 2.5]], [[-1.0, 1.5], [-2.0, 1.0], [-1.5, 2.0]]])


def _ttype(tag):
    return None if tag == "none" else tag


def _targs(tag):
    return {} if P[tag] is None else {"p": P[tag]}


_eval = {}


def eval_model(num_classes=15):
    """Evaluation mode with non-trivial running statistics (molecules of a batch are then independent), cond_mask_prob > 0."""
    if num_classes not in _eval:
        import shapemol_amd
        cfg = model_cfg(cond_mask_prob=0.1)
        m = shapemol_amd.ScorePosNet3D(cfg, num_classes)
        sdn = synth.synthetic_state_dict(cfg, seed=7, num_classes=num_classes)
        sdn.update(synth.running_stats(m.dims.L, m.dims.heads, 23))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=True)
        _eval[num_classes] = m.to(DEV).eval()
    return _eval[num_classes]


def _inputs(B, seed, steps, C=15, counts=None):
    """(bb, eps, u): a synthetic batch, or one with the given atom counts, and its fed noise."""
    bb = synth.synthetic_batch(B, seed=seed, num_classes=C)
    if counts is not None:
        counts = np.asarray(counts, dtype=np.int64)
        n = int(counts.sum())
        bb = dict(counts=counts, batch=np.repeat(np.arange(len(counts), dtype=np.int64), counts),
                  init_pos=synth.hash_normal((n, 3), 101, seed), init_v=(np.arange(n) % C).astype(np.int64),
                  shape=synth.hash_normal((len(counts), 32, 3), 103, seed))
    elif C != 15:
        from vocab import all_classes
        bb["init_v"] = all_classes(len(bb["batch"]), C, 102, seed)
    eps, u = hash_noise(len(bb["batch"]), steps, seed, c=C)
    return bb, eps, u


def run(m, bb, eps, u, **kw):
    B = len(bb["counts"])
    return m.sample_diffusion(T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1),
                              num_steps=len(eps), center_pos_mode="none", noise=(T(eps, DEV), T(u, DEV)), **kw)


def offsets(bb, group_mols):
    mol_off = np.concatenate([[0], np.cumsum(group_mols)]).astype(int)
    return mol_off, np.concatenate([[0], np.cumsum(bb["counts"])])[mol_off].astype(int)


def sub_batch(bb, eps, u, mol_lo, mol_hi, lo, hi):
    sub = dict(init_pos=bb["init_pos"][lo:hi], init_v=bb["init_v"][lo:hi], batch=bb["batch"][lo:hi] - mol_lo,
               shape=bb["shape"][mol_lo:mol_hi], counts=bb["counts"][mol_lo:mol_hi])
    return sub, eps[:, lo:hi], u[:, lo:hi]


def group_stat(m, n_groups):
    from shapemol_amd import _lib
    out = (C.c_float * (2 * n_groups))()
    n = _lib.load().shapemol_debug_read(m._context(torch.device(DEV)), b"cfg_group_stat", out, 8 * n_groups)
    assert n == 8 * n_groups
    return np.array(list(out), dtype=np.float32).reshape(n_groups, 2)


def assert_same(a, b, sl=slice(None), what=""):
    assert torch.equal(a["pos"], b["pos"][sl]) and torch.equal(a["v"], b["v"][sl]), what
    assert torch.equal(torch.stack(a["v_traj"]), torch.stack(b["v_traj"])[:, sl]), what
    for k in TRAJS:
        assert len(a[k]) == len(b[k]), (what, k)
        if a[k]:
            assert torch.equal(torch.stack(a[k]), torch.stack(b[k])[:, sl]), (what, k)


# ---------------------------------------------------------------------------------------------- golden chains
@pytest.mark.parametrize("tag", TYPES)
def test_cfg_groups_chain_golden(tag):
    """B = 6 in groups of 2 / 3 / 1, 20 steps from t = 999, train mode, against the reference's chain whose threshold_CFG ran
    once per group: atom types exact, positions within POS_TOL, the recorded trajectories within TRAJ_TOL (POS_TOL at the last
    step); graph replay and eager launches bit-identical."""
    m = hip_model(cond_mask_prob=0.1)
    c = golden(f"chain_cfg_groups_{tag}_b6_s20.npz")
    bb, eps, u = _inputs(int(c["B"]), int(c["seed"]), int(c["S"]))
    p = float(c["p"])
    kw = dict(threshold_type=_ttype(tag), threshold_args={} if np.isnan(p) else {"p": p},
              guide_stren=[(float(c["guide_stren"]), int(n)) for n in c["groups"]], bounds=torch.from_numpy(c["bounds"]).float())
    steps, runs = c["traj_steps"], []
    for use_graph in (True, False):
        r = run(m, bb, eps, u, use_graph=use_graph, **kw)
        runs.append(r)
        assert np.array_equal(r["v"].cpu().numpy(), c["v"])
        assert np.array_equal(torch.stack(r["v_traj"]).numpy(), c["v_traj"].astype(np.int64))
        errs = {"pos_end": maxabs(r["pos"], c["pos"])}
        for name in TRAJS:
            got = torch.stack([r[name][int(s)].cpu() for s in steps]).numpy()
            e = [maxabs(got[i], c[name][i]) for i in range(len(steps))]
            errs[name] = max(e)
            assert max(e[:-1]) <= TRAJ_TOL, (name, e)
            assert e[-1] <= POS_TOL, (name, e)
        print("cfg_groups_chain_golden", tag, use_graph, errs)
        record("cfg_groups_chain_golden", tag=tag, use_graph=use_graph, **errs)
        assert errs["pos_end"] <= POS_TOL
    assert_same(runs[0], runs[1], what="graph vs eager")


# ---------------------------------------------------------------------------------------------- eval-mode equality
def _mixed_and_alone(m, C, B, group_mols, strens, boxes, tag, seed, steps=20):
    bb, eps, u = _inputs(B, seed, steps, C)
    mol_off, atom_off = offsets(bb, group_mols)
    bounds = np.concatenate([np.stack([boxes[g]] * n) for g, n in enumerate(group_mols)])
    kw = dict(threshold_type=_ttype(tag), threshold_args=_targs(tag))
    mixed = run(m, bb, eps, u, guide_stren=list(zip(strens, group_mols)), bounds=bounds, **kw)
    alone = []
    for g in range(len(group_mols)):
        lo, hi = atom_off[g], atom_off[g + 1]
        sub, e_, u_ = sub_batch(bb, eps, u, mol_off[g], mol_off[g + 1], lo, hi)
        alone.append((slice(lo, hi), run(m, sub, e_, u_, guide_stren=strens[g], bounds=bounds[mol_off[g]:mol_off[g + 1]], **kw)))
    return bb, eps, u, bounds, kw, mixed, alone


@pytest.mark.parametrize("tag", TYPES)
def test_mixed_chain_equals_single_condition_chains(tag):
    """model.eval(): B = 6 in groups 2 / 3 / 1 with strengths 0.7 / 1.5 / 0.3 and three boxes, 20 steps -- the mixed chain is
    torch.equal to the three single-condition chains run through the scalar form on their slices of the inputs and the
    noise: pos, v and every trajectory."""
    _, _, _, _, _, mixed, alone = _mixed_and_alone(eval_model(), 15, 6, (2, 3, 1), (0.7, 1.5, 0.3), BOXES3, tag, 13)
    for g, (sl, r) in enumerate(alone):
        assert_same(r, mixed, sl, what=f"group {g}")


@pytest.mark.parametrize("tag", TYPES)
def test_mixed_chain_serial_kernel_and_negative_control(tag):
    """The same with 23 atom types (the serial posterior kernel) on B = 4 in groups 1 / 3; giving every group group 0's strength
    and box moves the other group by more than 1e-3."""
    m = eval_model(23)
    bb, eps, u, bounds, kw, mixed, alone = _mixed_and_alone(m, 23, 4, (1, 3), (0.7, 1.5), BOXES3[[2, 1]], tag, 17)
    for g, (sl, r) in enumerate(alone):
        assert_same(r, mixed, sl, what=f"group {g}")
    flat = run(m, bb, eps, u, guide_stren=[(0.7, 1), (0.7, 3)], bounds=np.stack([bounds[0]] * 4), **kw)
    sl = alone[1][0]
    assert torch.equal(flat["pos"][alone[0][0]], mixed["pos"][alone[0][0]])
    assert maxabs(flat["pos"][sl], mixed["pos"][sl]) > 1e-3


# ---------------------------------------------------------------------------------------------- statistic exactness
COUNTS = [1] + [5, 5, 4] + [20] * 6 + [17] + [23] * 29 + [16] + [23] * 7        # 48 molecules, 996 atoms
GROUP_MOLS = (1, 3, 7, 30, 7)          # 1 | 14 | 137 (2055 logits) | 683 (2049 coordinates) | 161 atoms: boundaries 1, 15, 152, 835


def test_group_statistics_are_exact_at_the_boundaries():
    """One step on a hand-built batch whose groups are a single-atom molecule, a group of fewer than 256 values, one whose
    logits just cross 2048 values, one whose coordinates just cross 2048 values, with no boundary on a multiple of 16 atoms:
    every group's statistic equals torch.quantile of its own combined slice bit for bit at six p; float32(max|cond_g|) *
    float32(p) for reference_threshold; the statistic of the one-group chain of the slice for rescale."""
    m = eval_model()
    bb, eps, u = _inputs(len(COUNTS), 21, 1, counts=COUNTS)
    mol_off, atom_off = offsets(bb, GROUP_MOLS)
    assert list(np.diff(atom_off)) == [1, 14, 137, 683, 161] and all(a % 16 for a in atom_off[1:-1])
    assert 136 * 15 <= 2048 < 137 * 15 and 682 * 3 <= 2048 < 683 * 3
    strens = (0.7, 1.5, 0.3, 0.9, 1.1)
    G = len(GROUP_MOLS)
    groups = list(zip(strens, GROUP_MOLS))
    pairs = (("pos_cond_traj", "pos_uncond_traj"), ("v_cond_traj", "v_uncond_traj"))
    for p in (0.995, 0.5, 0.3, 0.0, 1.0, 0.123456):
        r = run(m, bb, eps, u, threshold_type="dynamic_threshold", threshold_args={"p": p}, guide_stren=groups, bounds=None)
        stat = group_stat(m, G)
        for g in range(G):
            sl = slice(atom_off[g], atom_off[g + 1])
            for i, (cn, un) in enumerate(pairs):
                q = torch.quantile(O.combine(r[cn][0][sl], r[un][0][sl], strens[g]).reshape(-1), p).item()
                assert np.float32(q) == stat[g, i], (p, g, i, q, stat[g, i])
    r = run(m, bb, eps, u, threshold_type="reference_threshold", threshold_args={"p": 1.05}, guide_stren=groups, bounds=None)
    stat = group_stat(m, G)
    for g in range(G):
        sl = slice(atom_off[g], atom_off[g + 1])
        for i, (cn, _) in enumerate(pairs):
            want = np.float32(r[cn][0][sl].abs().max().item()) * np.float32(1.05)
            assert want == stat[g, i], (g, i, want, stat[g, i])
    r = run(m, bb, eps, u, threshold_type="rescale", threshold_args={"p": 0.6}, guide_stren=groups, bounds=None)
    stat = group_stat(m, G)
    for g in range(G):
        sub, e_, u_ = sub_batch(bb, eps, u, mol_off[g], mol_off[g + 1], atom_off[g], atom_off[g + 1])
        run(m, sub, e_, u_, threshold_type="rescale", threshold_args={"p": 0.6}, guide_stren=[(strens[g], GROUP_MOLS[g])], bounds=None)
        one = group_stat(m, 1)[0]
        assert np.array_equal(one, stat[g]), (g, one, stat[g])
    record("cfg_group_stat_exact", rescale=stat.tolist())


# ---------------------------------------------------------------------------------------------- train mode, recomposed
@pytest.mark.parametrize("tag", TYPES)
def test_cfg_groups_step_recomposed_train_mode(tag):
    """Train mode (batch statistics over the whole mixed batch), B = 8 in three groups with one strength 0, 5 steps: every step
    recomposed on the host from the chain's own state with per-group thresholds (the scheme of tests/test_gpu_cfg.py)."""
    m = hip_model(cond_mask_prob=0.1)
    B, S, group_mols, strens = 8, 5, (3, 2, 3), (1.5, 0.0, 0.7)
    bb, eps, u = _inputs(B, 31, S)
    mol_off, atom_off = offsets(bb, group_mols)
    boxes = [BOXES3[1], BOXES3[0], BOXES3[2]]
    bounds = np.concatenate([np.stack([boxes[g]] * n) for g, n in enumerate(group_mols)])
    r = run(m, bb, eps, u, threshold_type=_ttype(tag), threshold_args=_targs(tag), guide_stren=list(zip(strens, group_mols)), bounds=bounds)
    pos0, v0, batch, shape = T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1)
    e_d = T(eps, DEV)
    c0, ct, logvar = (m._table(k) for k in ("posterior_mean_c0_coef", "posterior_mean_ct_coef", "posterior_logvar"))
    worst = {"pos": 0.0, "v0": 0.0, "vt": 0.0}
    for s in range(S):
        t = 999 - s
        xt = pos0 if s == 0 else r["pos_traj"][s - 1].to(DEV)
        vt = v0 if s == 0 else r["v_traj"][s - 1].to(DEV)
        ts = torch.full((B,), t, dtype=torch.int64, device=DEV)
        pc = m(xt, vt, batch, shape, time_step=ts)
        pu = m(xt, vt, batch, torch.zeros_like(shape), time_step=ts)
        gp = GO.combine_groups(pc["pred_ligand_pos"], pu["pred_ligand_pos"], atom_off, strens)
        gv = GO.combine_groups(pc["pred_ligand_v"], pu["pred_ligand_v"], atom_off, strens)
        if tag == "dynamic_threshold":       # the statistic exactly as the reference takes it (torch.quantile on the device)
            outs_p, outs_v = [], []
            for g in range(len(group_mols)):
                sl = slice(atom_off[g], atom_off[g + 1])
                if strens[g] == 0:
                    outs_p.append(pc["pred_ligand_pos"][sl]), outs_v.append(pc["pred_ligand_v"][sl])
                    continue
                sp, sv = torch.quantile(gp[sl].reshape(-1), P[tag]), torch.quantile(gv[sl].reshape(-1), P[tag])
                bx = torch.as_tensor(boxes[g], dtype=torch.float32, device=DEV)
                x = torch.minimum(torch.maximum(gp[sl], -sp), sp)
                outs_p.append(torch.minimum(torch.maximum(x, bx[:, 0]), bx[:, 1]))
                outs_v.append(torch.minimum(torch.maximum(gv[sl], -sv), sv))
            gp, gv = torch.cat(outs_p), torch.cat(outs_v)
        else:
            gp = GO.threshold_cfg_groups(gp, pc["pred_ligand_pos"], atom_off, _ttype(tag), _targs(tag), boxes, strens)
            gv = GO.threshold_cfg_groups(gv, pc["pred_ligand_v"], atom_off, _ttype(tag), _targs(tag), None, strens)
        xn = c0[t] * gp + ct[t] * xt + (torch.exp(0.5 * logvar[t]) if t else 0.0) * e_d[s]
        lv0 = torch.log_softmax(gv, dim=-1)
        lvt = torch.log(torch.nn.functional.one_hot(vt, m.num_classes).float().clamp(min=1e-30))
        lp = m._q_v_posterior(lv0, lvt, ts, batch)
        worst["pos"] = max(worst["pos"], maxabs(xn, r["pos_traj"][s]))
        worst["v0"] = max(worst["v0"], maxabs(lv0, r["v0_traj"][s]))
        worst["vt"] = max(worst["vt"], maxabs(lp, r["vt_traj"][s]))
    print("cfg_groups_step_recomposed", tag, worst)
    record("cfg_groups_step_recomposed", tag=tag, **worst)
    assert worst["pos"] <= STEP_TOL and worst["v0"] <= STEP_TOL and worst["vt"] <= STEP_TOL, worst


# ---------------------------------------------------------------------------------------------- strength 0
def test_strength_zero_group_and_all_zero():
    """model.eval(): the molecules of a group with strength 0 inside a guided chain equal the unguided chain -- types exact,
    positions within POS_TOL (the unfolded coordinate update of a CFG chain is not bit-equal to the folded one of the unguided
    chain; the test prints and records the measured value; none has been taken on an MI355X yet) -- while the guided groups differ.  With every strength 0 the chain IS the
    unguided chain (torch.equal) and the uncond lists are empty."""
    m = eval_model()
    bb, eps, u = _inputs(6, 13, 20)
    _, atom_off = offsets(bb, (2, 3, 1))
    kw = dict(threshold_type="rescale", threshold_args={"p": 0.7}, bounds=np.concatenate([np.stack([BOXES3[g]] * n) for g, n in enumerate((2, 3, 1))]))
    plain = run(m, bb, eps, u)
    mixed = run(m, bb, eps, u, guide_stren=[(1.5, 2), (0.0, 3), (0.7, 1)], **kw)
    sl = slice(atom_off[1], atom_off[2])
    assert torch.equal(mixed["v"][sl], plain["v"][sl])
    assert torch.equal(torch.stack(mixed["v_traj"])[:, sl], torch.stack(plain["v_traj"])[:, sl])
    d = maxabs(mixed["pos"][sl], plain["pos"][sl])
    print(f"strength_zero_group: max |dpos| {d:.3e}")
    record("cfg_strength_zero_group", max_dpos=d)
    assert d <= POS_TOL
    assert maxabs(mixed["pos"][:atom_off[1]], plain["pos"][:atom_off[1]]) > 1e-3
    assert len(mixed["pos_uncond_traj"]) == 20 and mixed["pos_uncond_traj"][0].shape[0] == len(bb["batch"])
    zero = run(m, bb, eps, u, guide_stren=[(0.0, 2), (0.0, 3), (0, 1)], **kw)
    assert_same(zero, plain, what="all strengths 0")
    assert zero["pos_uncond_traj"] == [] and zero["v_uncond_traj"] == []


# ---------------------------------------------------------------------------------------------- stale state, refusals
def test_no_stale_state_between_layouts():
    """Layout A, layout B with the same (N, B), A again: both A runs are equal and B differs (the captured step is shared; the
    groups live in device memory).  A scalar-form chain and an unguided chain afterwards equal their runs on a fresh model."""
    import shapemol_amd
    m = eval_model()
    bb, eps, u = _inputs(6, 13, 8)
    kw = dict(threshold_type="dynamic_threshold", threshold_args={"p": 0.99}, bounds=np.stack([BOXES3[0]] * 6))
    A, Bl = [(0.7, 2), (1.5, 3), (0.3, 1)], [(0.7, 3), (1.5, 1), (0.3, 2)]
    cap0 = _captures(m)
    a1, b, a2 = run(m, bb, eps, u, guide_stren=A, **kw), run(m, bb, eps, u, guide_stren=Bl, **kw), run(m, bb, eps, u, guide_stren=A, **kw)
    assert _captures(m) - cap0 <= 2           # one executable pair serves both layouts
    assert_same(a1, a2, what="layout A twice")
    assert maxabs(a1["pos"], b["pos"]) > 1e-3
    scalar, plain = run(m, bb, eps, u, guide_stren=0.7, **kw), run(m, bb, eps, u)
    cfg = model_cfg(cond_mask_prob=0.1)
    fresh = shapemol_amd.ScorePosNet3D(cfg, 15)
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(DEV).eval()
    assert_same(scalar, run(fresh, bb, eps, u, guide_stren=0.7, **kw), what="scalar form after groups")
    assert_same(plain, run(fresh, bb, eps, u), what="unguided after groups")


def _captures(m):
    from shapemol_amd import _lib
    out = C.c_int64(0)
    assert _lib.load().shapemol_debug_read(m._context(torch.device(DEV)), b"captures", C.byref(out), 8) == 8
    return out.value


def test_refusals_before_launch_leave_the_context_usable():
    from shapemol_amd import _lib
    m = eval_model()
    bb, eps, u = _inputs(6, 13, 4)
    kw = dict(threshold_type="rescale", threshold_args={"p": 0.7}, bounds=None)
    good = [(0.7, 2), (1.5, 3), (0.3, 1)]
    base = run(m, bb, eps, u, guide_stren=good, **kw)
    with pytest.raises(ValueError, match="hold 5 molecules, the batch has 6"):
        run(m, bb, eps, u, guide_stren=[(0.7, 2), (1.5, 3)], **kw)
    with pytest.raises(ValueError, match="finite"):
        run(m, bb, eps, u, guide_stren=[(float("nan"), 2), (1.5, 3), (0.3, 1)], **kw)
    with pytest.raises(ValueError, match="at most 256"):
        run(m, bb, eps, u, guide_stren=[(0.5, 0)] * 251 + [(0.5, 1)] * 6, **kw)
    # the library's own checks (the message names the group, or the cap)
    lib, ctx = _lib.load(), m._context(torch.device(DEV))
    off = (C.c_int64 * 4)(0, 2, 1, 6)
    w = (C.c_double * 3)(0.7, 1.5, 0.3)
    assert lib.shapemol_set_cfg_groups(ctx, 3, off, w, 3, 0.7, None, None, None) != 0
    assert b"group 1" in lib.shapemol_last_error()
    w_nan = (C.c_double * 3)(0.7, 1.5, float("nan"))
    off = (C.c_int64 * 4)(0, 2, 5, 6)
    assert lib.shapemol_set_cfg_groups(ctx, 3, off, w_nan, 3, 0.7, None, None, None) != 0
    assert b"group 2" in lib.shapemol_last_error()
    assert lib.shapemol_set_cfg_groups(ctx, 257, None, None, 3, 0.7, None, None, None) != 0
    assert b"at most 256" in lib.shapemol_last_error()
    assert lib.shapemol_set_cfg_groups(ctx, 2, (C.c_int64 * 3)(0, 2, 5), (C.c_double * 2)(0.7, 1.5), 3, 0.7, None, None, None) == 0
    with pytest.raises(RuntimeError, match="classifier-free guidance groups cover 5 molecules"):
        run(m, bb, eps, u)                 # the installed set does not fit the batch
    assert lib.shapemol_set_cfg_groups(ctx, 0, None, None, 0, 0.0, None, None, None) == 0
    assert_same(base, run(m, bb, eps, u, guide_stren=good, **kw), what="after the refusals")


def test_list_ignored_under_point_cloud_guidance():
    m = eval_model()
    bb, eps, u = _inputs(6, 13, 6)
    cloud = synth.hash_normal((256, 3), 501, 3) * 2.0
    gk = dict(use_pointcloud_data=(cloud, None, 0.2), grad_step=990, seed=5)
    a = run(m, bb, eps, u, **gk)
    b = run(m, bb, eps, u, **gk, guide_stren=[(0.7, 2), (1.5, 3), (0.3, 1)], threshold_type="rescale", bounds=None)
    assert_same(a, b, what="list under a point cloud")
    assert b["pos_uncond_traj"] == []


# ---------------------------------------------------------------------------------------------- driver
N_COND, N_SAMPLES, STEPS = 3, 4, 6


def _tape():
    rs = np.random.RandomState(5)
    counts = rs.randint(12, 28, size=(N_COND, N_SAMPLES))
    mol = {}
    for c in range(N_COND):
        for k in range(N_SAMPLES):
            n, seed = int(counts[c, k]), 1000 * c + k
            eps, u = hash_noise(n, STEPS, seed)
            mol[c, k] = dict(pos=synth.hash_normal((n, 3), 701, seed), u0=synth.hash_uniform((n, 15), 702, seed), eps=eps, u=u)
    return counts, mol


def _install(mp, mol, batches):
    """torch.randn / torch.rand replay the per-molecule numbers in the driver's draw order for chains that hold `batches`."""
    cat = lambda mols, key, axis=0: np.concatenate([mol[m][key] for m in mols], axis=axis)      # noqa: E731
    normal, uniform = [], []
    for mols in batches:
        normal.append(cat(mols, "pos")), uniform.append(cat(mols, "u0"))
        normal += list(cat(mols, "eps", 1))
        uniform += list(cat(mols, "u", 1))

    def pop(queue, shape):
        a = queue.pop(0)
        assert tuple(a.shape) == tuple(shape), (a.shape, shape)
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    mp.setattr(torch, "randn", lambda *shape: pop(normal, shape))
    mp.setattr(torch, "rand", lambda *shape: pop(uniform, shape))
    return normal, uniform


def test_driver_per_condition_cfg(monkeypatch):
    """sample_diffusion_ligand_multi, 3 conditions x 4 samples, model.eval(), per-condition strengths and boxes.  batch_size 8
    (no condition straddles): every condition equals sample_diffusion_ligand(batch_size = 4) for it alone on the same
    per-molecule numbers -- types exact, positions within POS_TOL (about 1e-7 expected; recorded).  batch_size 6 (condition 1
    straddles): every recorded sample_diffusion call replayed by hand gives the driver's output exactly."""
    from shapemol_amd.sampling import plan_batches, sample_diffusion_ligand, sample_diffusion_ligand_multi
    m = eval_model()
    counts, mol = _tape()
    shapes = synth.hash_normal((N_COND, 32, 3), 103, 77)
    conds = [(shapes[c], None) for c in range(N_COND)]
    strens, boxes = [0.7, 1.5, 0.3], [BOXES3[0], None, BOXES3[2]]
    funcs = lambda: [lambda n, it=iter(counts[c].tolist()): [next(it) for _ in range(n)] for c in range(N_COND)]      # noqa: E731
    kw = dict(num_steps=STEPS, sample_num_atoms="size", host_rng=True, threshold_type="dynamic_threshold", threshold_args={"p": 0.99})
    batches = lambda bs: [[(c, f + k) for c, f, n in segs for k in range(n)] for segs in plan_batches(N_COND, N_SAMPLES, bs)]      # noqa: E731
    with monkeypatch.context() as mp:
        left = _install(mp, mol, batches(8))
        multi = sample_diffusion_ligand_multi(m, conds, N_SAMPLES, batch_size=8, sample_func=funcs(), guide_stren=strens, bounds=boxes, **kw)
        assert left == ([], [])
    worst = 0.0
    for c in range(N_COND):
        with monkeypatch.context() as mp:
            left = _install(mp, mol, [[(c, k) for k in range(N_SAMPLES)]])
            alone = sample_diffusion_ligand(m, conds[c][0], N_SAMPLES, batch_size=N_SAMPLES, sample_func=funcs()[c], guide_stren=strens[c],
                                            bounds=None if boxes[c] is None else np.stack([boxes[c]] * N_SAMPLES), **kw)
            assert left == ([], [])
        for k in range(N_SAMPLES):
            assert np.array_equal(multi[c][1][k], alone[1][k]), (c, k)
            worst = max(worst, float(np.abs(multi[c][0][k] - alone[0][k]).max()))
    print(f"driver_per_condition_cfg: max |dpos| {worst:.3e}")
    record("cfg_groups_driver", max_dpos=worst)
    assert worst <= POS_TOL
    # batch_size 6: the recorded calls, replayed
    seen, real = [], type(m).sample_diffusion

    def spy(self, *a, **k):
        seen.append({n: (v.clone() if torch.is_tensor(v) else v) for n, v in k.items()})
        return real(self, *a, **k)
    with monkeypatch.context() as mp:
        _install(mp, mol, batches(6))
        mp.setattr(m, "sample_diffusion", spy.__get__(m), raising=False)
        out = sample_diffusion_ligand_multi(m, conds, N_SAMPLES, batch_size=6, sample_func=funcs(), guide_stren=strens, bounds=boxes, **kw)
    assert len(seen) == 2
    assert seen[0]["guide_stren"] == [(0.7, 4), (1.5, 2)] and seen[1]["guide_stren"] == [(1.5, 2), (0.3, 4)]
    assert np.isnan(seen[0]["bounds"][4:]).all() and np.array_equal(seen[1]["bounds"][2:], np.stack([BOXES3[2]] * 4))
    flat_pos = [p for c in range(N_COND) for p in out[c][0]]
    flat_v = [v for c in range(N_COND) for v in out[c][1]]
    for i, k in enumerate(seen):
        r = m.sample_diffusion(**{n: v for n, v in k.items() if not n.startswith("_")})
        assert np.array_equal(r["pos"].cpu().numpy().astype(np.float64), np.concatenate(flat_pos[6 * i:6 * i + 6]))
        assert np.array_equal(r["v"].cpu().numpy(), np.concatenate(flat_v[6 * i:6 * i + 6]))
