"""The launch forms that only a reverse step takes, at the shapes where they switch or fill up: graph_kernel (kNN graph + edge
weights, molecules up to 128 atoms, 32- or 64-lane candidate chunks, two atoms per wave at KP = 8), the coordinate update folded
into the next x2h kernel (a 256-row LDS table) and into the posterior kernel, and the streaming edge kernels' tails.  Every test
first reads the library's record of what it launched (debug_read "launch": tests/chain_forms.py names the fields) and asserts
that the form it means to cover ran; the shapes follow from the device's CU count and the host's formulas restated in
tests/chain_forms.py.  Integer results are exact; float results are gated by precision.bound of the float32 oracle's own error
against the float64 oracle at the same state (no chain divergence: every step is recomposed from the device chain's own state).
Run on the GPU box:  pytest tests/test_gpu_chain_forms.py -m gpu"""
import numpy as np
import pytest
import torch

import chain_forms as CF
import precision as P
import vocab as V
from util import O, T, hip_model, maxabs, oracle_model, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL = 2e-5      # one forward (the gate of tests/test_gpu_parity.py)
SEED = 5
MODES = {"exact": {"edge_bf16": 2, "node_f16": 0}, "f16x2": {"edge_bf16": 3, "node_f16": 1}}
OUTS = ("pred_ligand_pos", "pred_ligand_h", "pred_ligand_v")
OPTION_DEFAULTS = {"ddpm_fold": 1, "vn_fold": 1, "graph_fuse": 1, "x2h_chain": 1}
STEPS = 3


def set_mode(m, mode):
    for k in ("edge_bf16", "node_f16"):
        m.set_option(k, MODES[mode][k])
    return m


@pytest.fixture(autouse=True)
def _restore_options():
    """Every test leaves the cached models on the library defaults."""
    yield
    import util
    from shapemol_amd.molopt_score_model import DEFAULT_OPTIONS
    defaults = dict(DEFAULT_OPTIONS, **OPTION_DEFAULTS)
    for key, m in list(util._cache.items()):
        if key[0] != "h":
            continue
        opts = m.__dict__.get("_options", {})
        for k in ("feat_f16", "node_f16", "edge_bf16") + tuple(OPTION_DEFAULTS):
            if k in opts and opts[k] != defaults[k]:
                m.set_option(k, defaults[k])


def num_cu():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def launch(m):
    """The record of the most recent score evaluation: {field: value}."""
    rec = dict(zip(CF.LAUNCH, (int(x) for x in m.debug_read("launch", (8,), np.int64))))
    assert rec["num_cu"] == num_cu()
    return rec


def chain(m, bb, steps, **kw):
    b = len(bb["counts"])
    r = m.sample_diffusion(T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(b, -1),
                           num_steps=steps, center_pos_mode="none", noise=(T(bb["eps"][:steps], DEV), T(bb["u"][:steps], DEV)), **kw)
    m.check_status()
    return r


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


_memo = {}


def memo(key, fn):
    if key not in _memo:
        _memo[key] = fn()
    return _memo[key]


# ------------------------------------------------------------------------------------------------------------------------
# A. the graph stage in chain form
# ------------------------------------------------------------------------------------------------------------------------
def _graph_case(k, profile, extra=()):
    counts = CF.graph_counts(k, extra)
    bb = CF.batch(counts, SEED, profile, steps=1)
    sd, dm, _, _ = oracle_model(knn=k)
    return bb, memo(("graph", k, profile, tuple(extra)), lambda: CF.graph_reference(sd, dm, bb))


def _check_graph(m, bb, ref, label, **tags):
    nbr_ref, valid, ew32, ew64 = ref
    n, kp = nbr_ref.shape
    assert kp == int(m.debug_read("dims", (8,), np.int64)[2])
    nbr = m.debug_read("nbr", (n, kp), np.int32)
    ew = m.debug_read("ew", (n, kp), np.float32)
    wrong = int((nbr != nbr_ref).any(1).sum())
    eh, e32 = P.rel_err(ew[valid], ew64[valid]), P.rel_err(ew32[valid], ew64[valid])
    record(label, atoms=n, wrong_atoms=wrong, ew_eH=eh, ew_e32=e32, ew_over_bound=eh / P.bound(e32), **tags)
    print(label, tags, "atoms", n, "wrong neighbour lists", wrong, f"e_w eH {eh:.3e} e32 {e32:.3e} eH/bound {eh / P.bound(e32):.3f}")
    assert wrong == 0, np.nonzero((nbr != nbr_ref).any(1))[0][:8]
    assert eh <= P.bound(e32), (eh, e32)


@pytest.mark.parametrize("profile", CF.PROFILES)
@pytest.mark.parametrize("k", CF.GRAPH_KS)
def test_graph_stage_in_chain_form(k, profile):
    """One reverse step on molecules of 1, 2, k .. k + 2 atoms and both sides of every candidate-chunk edge up to the 128-atom cap
    (tests/chain_forms.graph_counts), random positions and an integer lattice with exact distance ties and coincident atoms:
    graph_kernel's neighbour lists equal O.knn_edges slot for slot (-1 in the unused ones), its edge weights are within the gate
    of the float64 edge-weight MLP.  Exact mode."""
    m = hip_model(knn=k)
    bb, ref = _graph_case(k, profile)
    counts = bb["counts"]
    assert len(bb["batch"]) % 2 == 1
    if CF.kp_of(k) == 8:
        pairs = CF.wave_pairs(counts, k)
        assert any(a < b for a, b in pairs) and any(a > b for a, b in pairs)
    chain(m, bb, 1, use_graph=False)
    rec = launch(m)
    print("launch", rec)
    assert rec["sampling"] == 1 and rec["graph_fused"] == 1, rec
    _check_graph(m, bb, ref, "chain_forms_graph", k=k, profile=profile, graph_fused=1)


@pytest.mark.parametrize("k", [8, 32])
def test_graph_stage_falls_back_above_the_cap(k):
    """The same batch plus a 129-atom molecule: the record shows the two separate kernels, the results are still equal."""
    m = hip_model(knn=k)
    bb, ref = _graph_case(k, "random", extra=(CF.GRAPH_CAP + 1,))
    chain(m, bb, 1, use_graph=False)
    rec = launch(m)
    print("launch", rec)
    assert rec["sampling"] == 1 and rec["graph_fused"] == 0, rec
    _check_graph(m, bb, ref, "chain_forms_graph", k=k, profile="random", graph_fused=0)


def test_graph_stage_reports_a_hint_below_the_largest_molecule():
    """A max_mol_atoms hint of 128 while a 129-atom molecule is present: the fused graph kernel runs (the record says so), clamps
    the molecule and raises the span flag -- the chain fails with the max_mol_atoms error instead of returning numbers."""
    from shapemol_amd import _lib
    from shapemol_amd.runtime import ChainRunner
    m = hip_model()
    bb, _ = _graph_case(8, "random", extra=(CF.GRAPH_CAP + 1,))
    r = ChainRunner(m, len(bb["batch"]), len(bb["counts"]), 1, keep_traj=False)
    try:
        r.load_batch(bb["init_pos"], bb["init_v"], bb["batch"], bb["shape"])
        m.set_option("max_mol_atoms", CF.GRAPH_CAP)
        r.run(1, use_graph=False)
        rec = launch(m)
        assert rec["graph_fused"] == 1 and rec["vn_fold"] == 0, rec       # (the fold, off at this size, is not what reports it)
        with pytest.raises(_lib.ShapeMolLibraryError, match="max_mol_atoms"):
            r.synchronize()
        r.load_batch(bb["init_pos"], bb["init_v"], bb["batch"], bb["shape"])      # the true hint: the plain kernels, no error
        r.run(1, use_graph=False)
        r.synchronize()
        assert launch(m)["graph_fused"] == 0
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------------
# B. the folded coordinate updates at the capacity of their table
# ------------------------------------------------------------------------------------------------------------------------
def _fold_case(name):
    mode, k, counts, on = CF.fold_cases(num_cu())[name]
    assert CF.fold_expected(mode, counts, k, num_cu()) == on
    return mode, k, CF.batch(counts, SEED, steps=STEPS), on


def _expect_forms(rec, mode, k, bb, fold, ddpm):
    n, kp = len(bb["batch"]), CF.kp_of(k)
    assert rec["sampling"] == 1 and rec["vn_fold"] == int(fold) and rec["ddpm_fold"] == int(ddpm), rec
    assert rec["graph_fused"] == int(CF.graph_fused_expected(bb["counts"])), rec
    if mode == "exact":
        assert (rec["stream_chunk"], rec["stream_grid"]) == (CF.stream_chunk(n, kp, num_cu()), CF.stream_grid(n, kp, num_cu())), rec
        assert rec["x2h_chain"] == 0
    else:
        assert rec["stream_chunk"] == 0 and rec["x2h_chain"] == 1, rec      # (the f16x2 table bound counts the fused launch's waves)


def _check_steps(m, mode, k, bb, r, label, **tags):
    """Every step of the chain r against the oracles at the chain's own state: the raw predictions (precision.gate), the posterior
    step from the device's own predictions (vocab.step_gate).  Returns the worst eH / bound."""
    sd, dm, _, _ = oracle_model(knn=k)
    b, worst, wrong, excluded = len(bb["counts"]), 0.0, 0, 0
    for s in range(STEPS):
        r32, r64, t = CF.recompose(sd, dm, bb, r, s)
        pos, v = CF.step_state(bb, r, s)
        pc, vc = _np(r["pos_cond_traj"][s]), _np(r["v_cond_traj"][s])
        g = CF.score_gate(pc, vc, r32, r64)
        with torch.no_grad():      # the plain forward at the same state, for the record: what the chain form is to be compared with
            f = m(T(pos, DEV), T(v, DEV), T(bb["batch"], DEV), T(bb["shape"], DEV), t.to(DEV))
        gf = CF.score_gate(_np(f["pred_ligand_pos"]), _np(f["pred_ligand_v"]), r32, r64)
        args = (pos, v, pc, vc, T(bb["batch"]), t, bb["eps"][s], bb["u"][s])
        got = {"x": _np(r["pos_traj"][s]), "v0": _np(r["v0_traj"][s]), "vt": _np(r["vt_traj"][s]), "v": _np(r["v_traj"][s])}
        pg, w, ex = V.step_gate(got, V.posterior_step32(sd, dm, *args), V.posterior_step64(sd, dm.C, *args))
        row = {f"{key.replace('pred_ligand_', '')}_{nm}": val for key, tup in g.items() for nm, val in zip(("eH", "e32", "over_bound"), tup)}
        row.update({f"fwd_{key.replace('pred_ligand_', '')}_over_bound": tup[2] for key, tup in gf.items()})
        row.update({f"post_{key}_over_bound": tup[2] for key, tup in pg.items()})
        record(label, mode=mode, k=k, atoms=len(bb["batch"]), step=s, wrong_types=w, excluded=ex, **tags, **row)
        print(label, tags, mode, "step", s, {k_: f"{v_:.3g}" for k_, v_ in row.items()}, "wrong", w, "excluded", ex)
        worst = max([worst] + [tup[2] for tup in g.values()] + [tup[2] for tup in pg.values()])
        wrong, excluded = wrong + w, excluded + ex
    assert wrong == 0
    assert excluded <= 0.01 * STEPS * len(bb["batch"])
    return worst


@pytest.mark.parametrize("name", sorted(CF.fold_cases()))
def test_folded_updates_at_capacity(name):
    """Three reverse steps on a batch with a workgroup whose molecules fill the fold's 256-row table exactly (`full`: the fold and
    the posterior kernel's fold are on) or exceed it by one row (`over`: both off), per launch path: the exact mode's streaming
    kernels with one and two tiles per workgroup at k = 8 and two at k = 12, the f16x2 kernels at k = 8.  Every step's predictions
    and posterior outputs within the gate.

    The f16x2 mode does not claim this gate on every weight profile (tests/test_gpu_precision.py keeps it as the negative control);
    with the natural weights used here its forward is expected inside it, and the recorded `fwd_*` columns show the plain forward
    at the same state beside the chain form.  Not yet run on an MI355X: no figures to report."""
    mode, k, bb, on = _fold_case(name)
    m = set_mode(hip_model(knn=k), mode)
    r = chain(m, bb, STEPS, use_graph=False)
    rec = launch(m)
    print("launch", rec)
    _expect_forms(rec, mode, k, bb, on, on)
    worst = _check_steps(m, mode, k, bb, r, "chain_forms_fold", case=name, vn_fold=int(on), ddpm_fold=int(on))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("mode", list(MODES))
def test_posterior_fold_off_beside_a_full_table(mode):
    """The other side of the posterior kernel's fold while the x2h fold stays on (its table exactly full): option ddpm_fold = 0."""
    name = "exact_k8_chunk1_full" if mode == "exact" else "f16x2_k8_full"
    _, k, bb, on = _fold_case(name)
    m = set_mode(hip_model(knn=k), mode)
    m.set_option("ddpm_fold", 0)
    r = chain(m, bb, STEPS, use_graph=False)
    rec = launch(m)
    print("launch", rec)
    _expect_forms(rec, mode, k, bb, True, False)
    worst = _check_steps(m, mode, k, bb, r, "chain_forms_fold", case=name, vn_fold=1, ddpm_fold=0)
    assert worst <= 1.0, worst


def test_full_table_graph_replay_equals_eager_launches():
    """The captured step of a full-table batch (two tiles per workgroup) is bit-identical to its eager launches, and reports the
    decisions taken at its capture."""
    mode, k, bb, on = _fold_case("exact_k8_chunk2_full")
    m = set_mode(hip_model(knn=k), mode)
    a = chain(m, bb, STEPS, use_graph=False)
    rec_a = launch(m)
    m(T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV), torch.zeros(len(bb["counts"]), dtype=torch.long, device=DEV))
    assert launch(m)["sampling"] == 0
    b = chain(m, bb, STEPS, use_graph=True)
    rec_b = launch(m)
    _expect_forms(rec_b, mode, k, bb, True, True)
    assert rec_a == rec_b
    assert torch.equal(a["pos"], b["pos"]) and torch.equal(a["v"], b["v"])
    for key in ("pos_traj", "v_traj", "v0_traj", "vt_traj", "pos_cond_traj", "v_cond_traj"):
        assert torch.equal(torch.stack([x.cpu() for x in a[key]]), torch.stack([x.cpu() for x in b[key]])), key
    b2 = chain(m, bb, STEPS, use_graph=True)          # a replay of the cached executable reports them too
    assert launch(m) == rec_b and torch.equal(b2["pos"], b["pos"])


# ------------------------------------------------------------------------------------------------------------------------
# C. the streaming edge kernels' tails (one forward)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", ["c1m", "c1e", "c1p", "c2m", "c2e", "c2p", "chunk3_short"])
@pytest.mark.parametrize("k", sorted(CF.STREAM_KS))
def test_stream_tails_forward(k, case, mode):
    """One forward with as many 16-slot tiles as one fewer than, exactly and one more than once and twice the CU count (k > 16:
    two tiles per atom, so two fewer / more), and with three tiles per workgroup and a short last workgroup, at KP = 8 (odd N: the
    last tile holds one atom), 16 and 32, against the CPU oracle.  The f16x2 mode runs its own edge kernels on the same sizes."""
    kp = CF.kp_of(k)
    n = CF.stream_sizes(kp, num_cu())[case]
    bb = CF.stream_batch(k, n)
    t = (np.arange(len(bb["counts"])) * 37 % 1000).astype(np.int64)
    t[0], t[-1] = 0, 999
    sd, dm, _, _ = oracle_model(knn=k)
    ref = memo(("fwd", k, n), lambda: {key: val.numpy() for key, val in
                                       O.score(sd, dm, T(bb["init_pos"]), T(bb["init_v"]), T(bb["batch"]), T(bb["shape"]), T(t)).items()})
    m = set_mode(hip_model(knn=k), mode)
    with torch.no_grad():
        out = m(T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV), T(t, DEV))
    m.check_status()
    rec = launch(m)
    assert rec["sampling"] == 0 and rec["graph_fused"] == 0 and rec["vn_fold"] == 0 and rec["ddpm_fold"] == 0, rec
    if mode == "exact":
        jobs, chunk = CF.stream_jobs(n, kp), CF.stream_chunk(n, kp, num_cu())
        assert (rec["stream_chunk"], rec["stream_grid"]) == (chunk, CF.ceil_div(jobs, chunk)), rec
        if case == "chunk3_short":
            assert chunk == (3 if kp <= 16 else 4) and jobs % chunk != 0
        else:
            assert jobs - num_cu() * int(case[1]) == {"m": -1, "e": 0, "p": 1}[case[2]] * (2 if kp > 16 else 1)
    errs = {key: maxabs(out[key], ref[key]) for key in OUTS}
    record("chain_forms_stream_tails", k=k, case=case, mode=mode, atoms=n, chunk=rec["stream_chunk"], grid=rec["stream_grid"], **errs)
    print("launch", rec, errs)
    assert max(errs.values()) < FWD_TOL, errs
