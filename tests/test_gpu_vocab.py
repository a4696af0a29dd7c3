"""The library at class counts other than the 15 of `add_aromatic`: 10 (`basic`), 23 (`full`, what the sampling script falls
back to) and the boundaries of what the class count selects -- ddpm_step16_kernel (C <= 16) or the serial ddpm_step_kernel<32>,
the fold of the last coordinate update into it (C <= 16 only), one or two output tiles of the atom-type head, and every
class-sized array (embedding, per-(timestep, type) tables, CFG statistics).  Against the reference's own runs
(tests/golden/make_golden_vocab.py), the CPU oracle (pinned to them by tests/test_vocab_cpu.py) and float64 recompositions.
Every bound is a constant the suite already uses or precision.bound of a float32 error measured on the CPU.
Run on the GPU box:  pytest tests/test_gpu_vocab.py -m gpu"""
import ctypes as C_

import numpy as np
import pytest
import torch

import vocab as V
from util import O, T, golden, hash_noise, hip_model, maxabs, model_cfg, oracle_model, record, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL = 2e-5      # one forward (the gate of tests/test_gpu_parity.py)
POS_TOL = 1e-4      # coordinates of a chain (the gate of the chain parity tests)
FOLD_TOL = 2e-5     # a folded coordinate update against its separate launch (test_folded_coordinate_update_equals_separate_launch)
STEP_TOL = 1e-5     # one CFG step recomposed on the host (tests/test_gpu_cfg.py)
PRE_REL = 2.0 ** -22      # tests/test_gpu_prologue_table.py
MODES = {"exact": {"edge_bf16": 2, "node_f16": 0}, "f16x2": {"edge_bf16": 3, "node_f16": 1}}
OUTS = ("pred_ligand_pos", "pred_ligand_h", "pred_ligand_v")


def set_mode(m, mode):
    for k in ("edge_bf16", "node_f16"):
        m.set_option(k, MODES[mode][k])
    return m


@pytest.fixture(params=list(MODES))
def mode(request):
    return request.param


@pytest.fixture(autouse=True)
def _restore_options():
    """Every test leaves the cached models on the library defaults."""
    yield
    import util
    from shapemol_amd.molopt_score_model import DEFAULT_OPTIONS
    defaults = dict(DEFAULT_OPTIONS, prologue_tab=1, stop_layer=-1, ddpm_fold=1, vn_fold=1)
    for key, m in list(util._cache.items()):
        if key[0] != "h":
            continue
        opts = m.__dict__.get("_options", {})
        for k in ("feat_f16", "node_f16", "edge_bf16", "prologue_tab", "stop_layer", "ddpm_fold", "vn_fold"):
            if k in opts and opts[k] != defaults[k]:
                m.set_option(k, defaults[k])


def _forward(m, bb, t, pos="init_pos"):
    with torch.no_grad():
        out = m(T(bb[pos], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV), T(t, DEV))
    m.check_status()
    return {k: out[k].cpu().numpy() for k in OUTS}


def _chain(m, bb, steps, eps, u, **kw):
    b = len(bb["shape"])
    return m.sample_diffusion(T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(b, -1),
                              num_steps=steps, center_pos_mode="none", noise=(T(eps, DEV), T(u, DEV)), **kw)


def _fixture_batch(f):
    C = int(f["num_classes"])
    bb = synth.synthetic_batch(int(f["B"]), seed=int(f["seed"]), num_classes=C)
    assert set(bb["init_v"].tolist()) == set(range(C))
    return C, bb


# ------------------------------------------------------------------------------------------------------------------------
# one forward
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [10, 23])
def test_forward_vocab_golden(C, mode):
    """The reference's forward with 10 and 23 atom types (B = 4, t = 0 / 999 / mixed): six and nine padding rows of the head,
    two output tiles at 23.  Both precision modes."""
    f = golden(f"forward_vocab_c{C}.npz")
    _, bb = _fixture_batch(f)
    out = _forward(set_mode(hip_model(num_classes=C), mode), bb, f["t"])
    errs = {k: maxabs(out[k], f[k]) for k in OUTS}
    record("vocab_forward_golden", C=C, mode=mode, **errs)
    assert out["pred_ligand_v"].shape == (len(bb["batch"]), C)
    assert max(errs.values()) < FWD_TOL, errs


_oracle_fwd = {}


@pytest.mark.parametrize("C", [2, 16, 17, 32])
def test_forward_boundary_class_counts_vs_oracle(C, mode):
    """The smallest and largest class counts and both sides of the 16 | 17 boundary (one full head tile, no padding row | two
    tiles, fifteen padding rows) on a ragged batch of 1, 2, 9, 17 and 30 atoms (N = 59), t = 0 among the timesteps, against the
    CPU oracle.  Both precision modes."""
    bb, t = V.counts_batch(V.RAGGED_COUNTS, C, 5), V.ragged_timesteps()
    assert len(bb["batch"]) == 59 and set(bb["init_v"].tolist()) == set(range(C))
    if C not in _oracle_fwd:
        sd, dm, _, _ = oracle_model(num_classes=C)
        ref = O.score(sd, dm, T(bb["init_pos"]), T(bb["init_v"]), T(bb["batch"]), T(bb["shape"]), T(t))
        _oracle_fwd[C] = {k: ref[k].numpy() for k in OUTS}
    out = _forward(set_mode(hip_model(num_classes=C), mode), bb, t)
    errs = {k: maxabs(out[k], _oracle_fwd[C][k]) for k in OUTS}
    record("vocab_forward_boundary", C=C, mode=mode, **errs)
    assert max(errs.values()) < FWD_TOL, errs


@pytest.mark.parametrize("style", ["one_t", "mixed_t"])
@pytest.mark.parametrize("C", [10, 23])
def test_table_prologue_equals_per_atom_mlp(C, style):
    """The per-(timestep, type) tables (T * C rows) against the per-atom MLP prologue they replace, as
    tests/test_gpu_prologue_table.py at 15: h0 and the layer-0 queries bit-identical, the per-molecule term identical, pre0
    within one doubled fp32 rounding, the forward inside its gate.  Exact mode."""
    from test_gpu_prologue_table import _timesteps
    m = hip_model(num_classes=C)
    _, bb = _fixture_batch(golden(f"forward_vocab_c{C}.npz"))
    n, b, H = len(bb["batch"]), len(bb["counts"]), m.dims.H
    t = _timesteps(style, b)
    got, out = {}, {}
    for tab in (0, 1):
        m.set_option("prologue_tab", tab)
        m.set_option("stop_layer", 1)
        try:
            _forward(m, bb, t)
            got[tab] = {"h0": m.debug_read("h0", (n, H), np.float32), "q_x": m.debug_read("q_x", (n, H), np.float32),
                        "pre0": m.debug_read("pre0", (n, 4 * H), np.float32), "add0": m.debug_read("add0", (b, 4 * H), np.float32)}
        finally:
            m.set_option("stop_layer", -1)
        out[tab] = _forward(m, bb, t)
    a, p = got[1], got[0]
    assert np.array_equal(a["h0"], p["h0"]) and np.array_equal(a["q_x"], p["q_x"]) and np.array_equal(a["add0"], p["add0"])
    d = np.abs(a["pre0"].astype(np.float64) - p["pre0"].astype(np.float64))
    bound = PRE_REL * (np.abs(p["pre0"].astype(np.float64)) + np.abs(p["add0"].astype(np.float64)[bb["batch"]]))
    assert int((d > bound).sum()) == 0
    assert max(maxabs(out[1][k], out[0][k]) for k in OUTS) < FWD_TOL


# ------------------------------------------------------------------------------------------------------------------------
# the posterior step
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", V.POSTERIOR_CLASSES)
def test_posterior_step_recomposed(C):
    """Three reverse steps t = 2, 1, 0 (sig = 0 and the clamp of t - 1 in the last) of N = 131 atoms -- the tail of a 16-lane
    group, of a 256-thread block of ddpm_step16_kernel and of a 128-thread block of ddpm_step_kernel<32> -- each recomposed in
    float64 from the kernel's own recorded raw predictions: x_next, log v0 and the posterior log-probabilities within
    precision.bound(e32), e32 the error of oracle.posterior_step (float32) on the same inputs; the sampled types equal the
    float64 arg-max wherever its top-two gap clears that bound (at most 1 % of the pairs excluded:
    test_vocab_cpu.test_posterior_step_gate_holds_for_the_float32_oracle).  The step's arithmetic does not depend on the precision
    mode of the matrix products: exact mode."""
    bb = V.counts_batch(V.POSTERIOR_COUNTS, C, V.POSTERIOR_SEED, V.POSTERIOR_STEPS)
    S, n, b = V.POSTERIOR_STEPS, len(bb["batch"]), len(bb["counts"])
    m = hip_model(num_classes=C)
    r = _chain(m, bb, S, bb["eps"], bb["u"], first_step=m.num_timesteps - S)
    sd, dm, _, _ = oracle_model(num_classes=C)
    batch = T(bb["batch"])
    worst, wrong, excluded = {}, 0, 0
    for s in range(S):
        t = torch.full((b,), S - 1 - s, dtype=torch.long)
        pos = bb["init_pos"] if s == 0 else r["pos_traj"][s - 1].numpy()
        v = bb["init_v"] if s == 0 else r["v_traj"][s - 1].numpy()
        args = (pos, v, r["pos_cond_traj"][s].cpu().numpy(), r["v_cond_traj"][s].cpu().numpy(), batch, t, bb["eps"][s], bb["u"][s])
        r32, r64 = V.posterior_step32(sd, dm, *args), V.posterior_step64(sd, C, *args)
        got = {"x": r["pos_traj"][s].numpy(), "v0": r["v0_traj"][s].numpy(), "vt": r["vt_traj"][s].numpy(), "v": r["v_traj"][s].numpy()}
        g, w, ex = V.step_gate(got, r32, r64)
        record("vocab_posterior_step", C=C, step=s, t=S - 1 - s, excluded=ex, wrong=w,
               **{f"{k}_{name}": val for k, tup in g.items() for name, val in zip(("eH", "e32", "over_bound"), tup)})
        print(C, s, g, w, ex)
        wrong, excluded = wrong + w, excluded + ex
        for k, tup in g.items():
            worst[k] = max(worst.get(k, 0.0), tup[2])
    assert np.array_equal(r["v"].cpu().numpy(), r["v_traj"][-1].numpy()) and torch.equal(r["pos"].cpu(), r["pos_traj"][-1])
    assert max(worst.values()) <= 1.0, worst
    assert wrong == 0
    assert excluded <= 0.01 * S * n


def _zero_head_model(C):
    """A model whose atom-type head predicts exactly zero for every class (second Linear zeroed)."""
    import shapemol_amd
    cfg = model_cfg()
    sdn = synth.synthetic_state_dict(cfg, seed=7, num_classes=C)
    for k in ("v_inference.2.weight", "v_inference.2.bias"):
        sdn[k] = np.zeros_like(sdn[k])
    m = shapemol_amd.ScorePosNet3D(cfg, C)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=True)
    return m.to(DEV), O.state_dict_from_numpy(sdn)


@pytest.mark.parametrize("C", [16, 17, 23, 32])
def test_posterior_step_ties_take_the_first_index(C):
    """Exactly tied Gumbel scores inside the posterior kernels (ddpm_step16_kernel at C = 16, the serial arg-max of
    ddpm_step_kernel<32> above): with equal logits for every class and equal uniforms for all but the atom's own type, whose
    uniform is the smallest, the C - 1 other classes tie to the bit, and torch's arg-max takes the first.  One step from
    t = T - 1; exact mode."""
    bb = V.counts_batch(V.POSTERIOR_COUNTS, C, V.POSTERIOR_SEED, 1)
    n, b = len(bb["batch"]), len(bb["counts"])
    u = np.full((1, n, C), 1.0 - 2.0 ** -24, np.float32)
    u[0, np.arange(n), bb["init_v"]] = 0.0
    m, sd = _zero_head_model(C)
    try:
        r = _chain(m, bb, 1, bb["eps"], u)
        assert not r["v_cond_traj"][0].cpu().numpy().any()
        t = torch.full((b,), m.num_timesteps - 1, dtype=torch.long)
        r64 = V.posterior_step64(sd, C, bb["init_pos"], bb["init_v"], r["pos_cond_traj"][0].cpu().numpy(), np.zeros((n, C), np.float32),
                                 T(bb["batch"]), t, bb["eps"][0], u[0])
        want = np.where(bb["init_v"] == 0, 1, 0)
        assert np.array_equal(r64["score"].argmax(-1), want)                   # the float64 scores tie as well: first index
        assert (np.sort(r64["score"], -1)[:, -1] == np.sort(r64["score"], -1)[:, -2]).all()
        assert np.array_equal(r["v"].cpu().numpy(), want)
    finally:
        m._release()


@pytest.mark.parametrize("C", [2, 16, 17, 23, 32])
def test_log_sample_categorical(C):
    """shapemol_log_sample_categorical against oracle.gumbel_argmax on random logits and uniforms (N = 131), and torch's
    first-maximum rule on all-equal logits with all-equal uniforms (index 0)."""
    import shapemol_amd
    n = 131
    logits = (2.0 * synth.hash_normal((n, C), 301, C)).astype(np.float32)
    u = synth.hash_uniform((n, C), 302, C)
    want = O.gumbel_argmax(T(logits), T(u)).numpy()
    got = shapemol_amd.log_sample_categorical(T(logits, DEV), u=T(u, DEV)).cpu().numpy()
    score = -np.log(-np.log(u.astype(np.float64) + 1e-30) + 1e-30) + logits
    top = np.sort(score, -1)
    clear = top[:, -1] - top[:, -2] > 1e-4                # (no draw of this seed is closer; a float32 score is within ~1e-6)
    assert clear.all() and np.array_equal(want, score.argmax(-1))
    assert np.array_equal(got, want)
    for lv, uv in ((0.0, 0.5), (-3.25, 0.0), (7.0, 1.0 - 2.0 ** -24)):
        tie = shapemol_amd.log_sample_categorical(torch.full((n, C), lv, device=DEV), u=torch.full((n, C), uv, device=DEV))
        assert not tie.cpu().numpy().any(), (lv, uv)


# ------------------------------------------------------------------------------------------------------------------------
# chains
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("C", [10, 23])
def test_chain_vocab_golden(C, use_graph, mode):
    """20 reverse steps of the reference with 10 and 23 atom types on hash noise: the final and every step's atom types
    exact, the final and every step's positions within 1e-4.  At 23 the step ends with the separate coordinate
    update and the serial posterior kernel.  Both precision modes, eager launches and graph replay."""
    c = golden(f"chain_vocab_c{C}_b4_s20.npz")
    _, bb = _fixture_batch(c)
    S = int(c["S"])
    eps, u = hash_noise(len(bb["batch"]), S, int(c["seed"]), c=C)
    r = _chain(set_mode(hip_model(num_classes=C), mode), bb, S, eps, u, use_graph=use_graph)
    errs = {"pos": maxabs(r["pos"], c["pos"]), "pos_traj": maxabs(torch.stack(r["pos_traj"]), c["pos_traj"]),
            "v0_traj": maxabs(torch.stack(r["v0_traj"]), c["v0_traj"]), "vt_traj": maxabs(torch.stack(r["vt_traj"]), c["vt_traj"])}
    record("vocab_chain_golden", C=C, mode=mode, use_graph=use_graph, **errs)
    assert np.array_equal(r["v"].cpu().numpy(), c["v"])
    assert np.array_equal(torch.stack(r["v_traj"]).numpy(), c["v_traj"].astype(np.int64))
    assert max(errs["pos"], errs["pos_traj"]) < POS_TOL, errs       # (log v0 and the posterior: recorded; gated step by step in
                                                                    #  test_posterior_step_recomposed)


def test_ddpm_fold_option_is_inert_at_23_classes():
    """Above 16 classes the last coordinate update is never folded into the posterior kernel, so the option that controls the
    fold changes nothing: bit-identical chains.  Exact mode."""
    C = 23
    c = golden(f"chain_vocab_c{C}_b4_s20.npz")
    _, bb = _fixture_batch(c)
    S = int(c["S"])
    eps, u = hash_noise(len(bb["batch"]), S, int(c["seed"]), c=C)
    m = hip_model(num_classes=C)
    r1 = _chain(m, bb, S, eps, u)
    try:
        m.set_option("ddpm_fold", 0)
        r0 = _chain(m, bb, S, eps, u)
    finally:
        m.set_option("ddpm_fold", 1)
    assert torch.equal(r1["pos"], r0["pos"]) and torch.equal(r1["v"], r0["v"])
    for k in ("pos_traj", "v_traj", "v0_traj", "vt_traj", "pos_cond_traj", "v_cond_traj"):
        assert torch.equal(torch.stack(r1[k]), torch.stack(r0[k])), k


@pytest.mark.parametrize("opt", ["ddpm_fold", "vn_fold"])
def test_folds_on_and_off_agree_at_16_classes(opt, mode):
    """16 classes is the largest count at which the last layer's coordinate update runs inside the posterior kernel (every lane
    of a 16-lane group then holds a class): with the fold and with the separate launch the chain is the same to rounding, as
    test_folded_coordinate_update_equals_separate_launch requires at 15.  Both precision modes."""
    C = 16
    bb = synth.synthetic_batch(8, seed=9, num_classes=C)
    assert set(bb["init_v"].tolist()) == set(range(C))
    eps, u = hash_noise(len(bb["batch"]), 12, 9, c=C)
    m = set_mode(hip_model(num_classes=C), mode)
    r1 = _chain(m, bb, 12, eps, u)
    try:
        m.set_option(opt, 0)
        r0 = _chain(m, bb, 12, eps, u)
    finally:
        m.set_option(opt, 1)
    e = {"pos": maxabs(r1["pos"], r0["pos"]), "pos_cond_traj": maxabs(torch.stack(r1["pos_cond_traj"]), torch.stack(r0["pos_cond_traj"]))}
    record("vocab_fold_c16", opt=opt, mode=mode, **e)
    assert torch.equal(r1["v"], r0["v"]) and max(e.values()) < FOLD_TOL, e


@pytest.mark.parametrize("tag", ["none", "reference_threshold", "dynamic_threshold", "rescale"])
def test_cfg_step_recomposed_at_23_classes(tag):
    """Classifier-free guidance with 23 atom types (B = 8, 4 steps): every step recomposed on the host as
    test_gpu_cfg.test_cfg_step_recomposed_at_size does, the statistics over N * 23 logits.  Exact mode."""
    from test_gpu_cfg import STEP_TOL as tol, recomposed_step_errors
    assert tol == STEP_TOL
    worst, n = recomposed_step_errors(tag, 8, 4, 31, C=23)
    record("vocab_cfg_step_recomposed", tag=tag, C=23, n=n, **worst)
    assert worst["pos"] <= STEP_TOL and worst["v0"] <= STEP_TOL and worst["vt"] <= STEP_TOL, worst


# ------------------------------------------------------------------------------------------------------------------------
# training and validation
# ------------------------------------------------------------------------------------------------------------------------
def _loss_case(C, B=6, seed=61):
    import shapemol_amd
    cfg = model_cfg()
    bb = synth.synthetic_batch(B, seed=seed, num_classes=C)
    n = len(bb["batch"])
    bb["init_v"] = V.all_classes(n, C, 102, seed)
    t = np.array([0, 999, 130, 470, 820, 5], np.int64)[:B]
    noise, u = synth.hash_normal((n, 3), 502, seed), synth.hash_uniform((n, C), 503, seed)
    m = shapemol_amd.ScorePosNet3D(cfg, C)
    sdn = synth.synthetic_state_dict(cfg, seed=7, num_classes=C)
    sdn.update(synth.running_stats(m.dims.L, m.dims.heads))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=True)
    return m.to(DEV), cfg, sdn, bb, t, noise, u


@pytest.mark.parametrize("C", [10, 23])
def test_diffusion_loss_vs_oracle(C):
    """get_diffusion_loss as validate() calls it (eval mode, given time steps, no gradients), B = 6, against
    oracle.diffusion_loss: the perturbed types exact, the three losses within 2e-5 relative (the tolerance of
    test_diffusion_loss_golden against the reference's own loss).  Exact mode."""
    m, cfg, sdn, bb, t, noise, u = _loss_case(C)
    B = len(bb["counts"])
    try:
        m.eval()
        with torch.no_grad():
            r = m.get_diffusion_loss(T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1),
                                     time_step=T(t, DEV), eval_mode=True, noise=(T(noise, DEV), T(u, DEV)))
        m.check_status()
        ref = O.diffusion_loss(O.state_dict_from_numpy(sdn), O.Dims(cfg, C), T(bb["init_pos"]), T(bb["init_v"]), T(bb["batch"]), T(bb["shape"]),
                               T(t), T(noise), T(u), bn_eval=True, loss_v_weight=cfg["loss_v_weight"], loss_weight_type=cfg["loss_weight_type"])
        assert np.array_equal(r["ligand_v_perturbed"].cpu().numpy(), ref["ligand_v_perturbed"].numpy())
        errs = {k: maxabs(r[k], ref[k]) for k in ("pred_ligand_pos", "pred_ligand_v", "ligand_v_recon")}
        rel = {k: abs(float(r[k]) - float(ref[k])) / max(1.0, abs(float(ref[k]))) for k in ("loss_pos", "loss_v", "loss")}
        record("vocab_diffusion_loss", C=C, **errs, **{f"rel_{k}": v for k, v in rel.items()})
        assert max(errs.values()) < FWD_TOL, errs
        assert max(rel.values()) < 2e-5, rel
    finally:
        m._release()


def test_training_step_class_sized_gradients_at_23_classes():
    """One training step (autograd through the HIP operators) with 23 atom types: the gradients of the tensors whose shape depends
    on the class count -- the atom embedding and the head's second Linear -- against float64 autograd through
    oracle.score_with_grad and the oracle's loss, within 1e-4 of each tensor's gradient norm (the rule of
    test_training_step_gradients_golden: the scale is at least 1e-3 of the whole gradient's norm).  Exact mode."""
    C = 23
    m, cfg, sdn, bb, t, noise, u = _loss_case(C)
    B = len(bb["counts"])
    try:
        m.train()
        r = m.get_diffusion_loss(T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1),
                                 time_step=T(t, DEV), eval_mode=True, noise=(T(noise, DEV), T(u, DEV)))
        r["loss"].backward()
        names = [k for k, p in m.named_parameters() if p.requires_grad]
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in O.state_dict_from_numpy(sdn).items()}
        sd = {k: (v.requires_grad_(True) if k in names else v) for k, v in sd.items()}
        ref = O.diffusion_loss(sd, O.Dims(cfg, C), T(bb["init_pos"]).double(), T(bb["init_v"]), T(bb["batch"]), T(bb["shape"]).double(), T(t),
                               T(noise).double(), T(u), bn_eval=False, loss_v_weight=cfg["loss_v_weight"],
                               loss_weight_type=cfg["loss_weight_type"], with_grad=True)
        assert ref["loss"].dtype == torch.float64
        assert np.array_equal(r["ligand_v_perturbed"].cpu().numpy(), ref["ligand_v_perturbed"].numpy())
        assert abs(float(r["loss"]) - float(ref["loss"])) < 2e-5 * abs(float(ref["loss"]))
        ref["loss"].backward()
        total = np.sqrt(sum(float((sd[k].grad ** 2).sum()) for k in names if sd[k].grad is not None))
        grads = dict(m.named_parameters())
        worst = {}
        for key in ("ligand_atom_emb.weight", "ligand_atom_emb.bias", "v_inference.2.weight", "v_inference.2.bias"):
            want = sd[key].grad.numpy()
            got = grads[key].grad.detach().cpu().numpy().astype(np.float64)
            assert got.shape == want.shape
            norm = float(np.sqrt((want ** 2).sum()))
            scale = max(norm, 1e-3 * total)
            worst[key] = float(np.abs(got - want).max()) / scale
            assert abs(np.sqrt((got ** 2).sum()) - norm) <= 1e-4 * scale, key
        record("vocab_training_step_gradients", C=C, total_grad_norm=total, **worst)
        assert max(worst.values()) <= 1e-4, worst
    finally:
        m._release()


# ------------------------------------------------------------------------------------------------------------------------
# refusal
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 33])
def test_class_counts_outside_2_to_32_are_refused_at_creation(C):
    """shapemol_create fails for num_classes = 1 and 33 with a message naming the range, and leaves the out pointer alone (no
    context was made); the Python module raises from its first use."""
    import shapemol_amd
    from shapemol_amd import _lib
    lib = _lib.load()
    d = hip_model().dims
    conf = _lib.Config(d.H, d.heads, d.L, d.k, d.G, d.S, d.S_latent, d.temb, C, d.T)
    w = np.zeros(16, np.float32)
    ctx = C_.c_void_p(0x5A5A)
    rc = lib.shapemol_create(C_.byref(conf), w.ctypes.data_as(C_.c_void_p), w.size, 0, C_.byref(ctx))
    assert rc != 0 and ctx.value == 0x5A5A
    assert b"2..32" in lib.shapemol_last_error()
    m = shapemol_amd.ScorePosNet3D(model_cfg(), C).to(DEV)
    with pytest.raises(_lib.ShapeMolLibraryError, match=r"2\.\.32"):
        m(torch.zeros(3, 3, device=DEV), torch.zeros(3, dtype=torch.long, device=DEV), torch.zeros(3, dtype=torch.long, device=DEV),
          torch.zeros(1, 32, 3, device=DEV), torch.zeros(1, dtype=torch.long, device=DEV))
    assert m._ctx is None
