"""Mesh shape guidance with one mesh per group of molecules on the device: sample_diffusion(use_mesh_data=[...]),
ScorePosNet3D.mesh_shape_guidance_groups and sample_diffusion_ligand_multi with mesh conditions, against the reference's chains
of tests/golden/make_golden_mesh_multi.py and against the single-mesh path.
Run on the GPU box:  pytest tests/test_gpu_mesh_multi.py -m gpu"""
import numpy as np
import pytest
import torch

from mesh_multi_util import CHAINS, FN, atom_ranges, chain_batch, mesh_groups, meshes
from util import T, golden, hash_noise, hip_model, maxabs, model_cfg, record, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POS_TOL = 1e-4      # the project's chain gate: coordinates within 1e-4 abs, atom types exact
FN_TOL = 1e-6       # the function alone, as the single-mesh test: float64 arithmetic as numpy's, rounded once to float32
MODES = {"exact": {"edge_bf16": 2, "node_f16": 0}, "f16x2": {"edge_bf16": 3, "node_f16": 1}}


def fixture_inputs(c):
    B, S, seed = int(c["B"]), int(c["S"]), int(c["seed"])
    bb = synth.synthetic_batch(B, seed=seed)
    eps, u = hash_noise(len(bb["batch"]), S, seed)
    return bb, eps, u, B, S


def run(m, bb, eps, u, B, S, **kw):
    return m.sample_diffusion(T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1),
                              num_steps=S, center_pos_mode="none", noise=(T(eps, DEV), T(u, DEV)), **kw)


def eval_model():
    """A model in evaluation mode with non-trivial running statistics: molecules of a batch are then independent."""
    import shapemol_amd
    cfg = model_cfg()
    m = shapemol_amd.ScorePosNet3D(cfg, 15)
    sdn = synth.synthetic_state_dict(cfg, seed=7)
    sdn.update(synth.running_stats(m.dims.L, m.dims.heads, 23))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=True)
    return m.to(DEV).eval()


def sub_batch(bb, eps, u, draws, mol_lo, mol_hi, lo, hi):
    sub = dict(init_pos=bb["init_pos"][lo:hi], init_v=bb["init_v"][lo:hi], batch=bb["batch"][lo:hi] - mol_lo,
               shape=bb["shape"][mol_lo:mol_hi], counts=bb["counts"][mol_lo:mol_hi])
    return sub, eps[:, lo:hi], u[:, lo:hi], np.ascontiguousarray(draws[:, :, lo:hi])


def moved(a, b):
    return (np.asarray(a) != np.asarray(b)).any(1)


def test_grouped_function_golden():
    """Function parity: mesh_shape_guidance_groups on the fixtures' atoms and draws equals the reference dispatcher: the same
    moved set, every atom within 1e-6 (no atom exempted); in place; device Philox draws are deterministic per seed."""
    m = hip_model()
    f = golden(FN)
    cases = [(FN, f["pred"], f["out"], f["draws"], f["batch"], mesh_groups(f))]
    for name in CHAINS:
        c = golden(name)
        cases.append((name, c["fn_pred"], c["fn_out"], c["draws"][0], chain_batch(c)["batch"], mesh_groups(c)))
    for name, pred, ref, draws, batch, groups in cases:
        pos = T(pred.copy(), DEV)
        out = m.mesh_shape_guidance_groups(groups, pos, T(batch.astype(np.int64), DEV), draws=T(draws, DEV))
        assert out.data_ptr() == pos.data_ptr()
        got = out.cpu().numpy()
        err = maxabs(got, ref)
        print(f"grouped_mesh_function_golden {name}: moved {int(moved(ref, pred).sum())} of {len(pred)} max_err {err:.3e}")
        record("grouped_mesh_function_golden", fixture=name, moved=int(moved(ref, pred).sum()), max_err=err)
        assert np.array_equal(moved(got, pred), moved(ref, pred))
        assert err <= FN_TOL
    name, pred, ref, draws, batch, groups = cases[0]
    bt = T(batch.astype(np.int64), DEV)
    a = m.mesh_shape_guidance_groups(groups, T(pred.copy(), DEV), bt, seed=5).cpu().numpy()
    b = m.mesh_shape_guidance_groups(groups, T(pred.copy(), DEV), bt, seed=5).cpu().numpy()
    d = m.mesh_shape_guidance_groups(groups, T(pred.copy(), DEV), bt, seed=6).cpu().numpy()
    assert np.array_equal(a, b) and not np.array_equal(a, d)
    assert not moved(a, pred)[~(f["pulls"] > 0)].any()              # atoms that need no pull never move, whatever the draws


def test_grouped_function_with_odd_cloud_sizes():
    """Clouds whose sizes are odd or 2 mod 4 (199 / 511 / 298 points: the LDS tile behind a group's cloud then starts at 24 P_g
    bytes rounded up to 32) against tests/mesh_oracle.py applied per group on the function fixture's atoms and draws."""
    import mesh_oracle as M
    m = hip_model()
    f = golden(FN)
    sizes = (199, 511, 298)
    groups = [(g[0], g[1][:n], None, g[3]) for g, n in zip(mesh_groups(f), sizes)]
    _, off = atom_ranges(np.bincount(f["batch"]), f["group_mols"])
    ref = f["pred"].copy()
    for g, (mesh, cloud, _, _n) in enumerate(groups):
        lo, hi = off[g], off[g + 1]
        ref[lo:hi] = M.mesh_shape_guidance(mesh[0], mesh[1], cloud, f["pred"][lo:hi], f["draws"][:, lo:hi])
    got = m.mesh_shape_guidance_groups(groups, T(f["pred"].copy(), DEV), T(f["batch"].astype(np.int64), DEV), draws=T(f["draws"], DEV)).cpu().numpy()
    err = maxabs(got, ref)
    print(f"grouped_mesh_function_odd_clouds: moved {int(moved(ref, f['pred']).sum())} max_err {err:.3e}")
    record("grouped_mesh_function_odd_clouds", moved=int(moved(ref, f["pred"]).sum()), max_err=err)
    assert moved(ref, f["pred"]).sum() > 100 and np.array_equal(moved(got, f["pred"]), moved(ref, f["pred"]))
    assert err <= FN_TOL


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", CHAINS)
def test_grouped_chain_golden(name, mode):
    """Chain parity in both precision modes: the fixture chain with the mesh list and the recorded draws, with and without the
    captured graph: atom types exact at every step, final positions, pos_traj and pos_cond_traj (at the stored steps) within
    1e-4 for every atom."""
    m = hip_model()
    c = golden(name)
    bb, eps, u, B, S = fixture_inputs(c)
    try:
        for k, v in MODES[mode].items():
            m.set_option(k, v)
        for use_graph in (True, False):
            r = run(m, bb, eps, u, B, S, use_graph=use_graph, use_mesh_data=mesh_groups(c), grad_step=int(c["grad_step"]),
                    guide_draws=T(c["draws"], DEV))
            ts = c["traj_steps"]
            e_pos = maxabs(r["pos"], c["pos"])
            e_cond = maxabs(torch.stack(r["pos_cond_traj"])[ts], c["pos_cond_traj"])
            e_traj = maxabs(torch.stack(r["pos_traj"])[ts], c["pos_traj"])
            v_same = np.array_equal(r["v"].cpu().numpy(), c["v"]) and np.array_equal(torch.stack(r["v_traj"]).numpy(), c["v_traj"])
            print(f"grouped_mesh_chain_golden {name} {mode} use_graph={use_graph}: pos {e_pos:.3e} pos_cond_traj {e_cond:.3e} "
                  f"pos_traj {e_traj:.3e} types_exact {v_same}")
            record("grouped_mesh_chain_golden", fixture=name, mode=mode, use_graph=use_graph, pos_end=e_pos, pos_cond_traj=e_cond,
                   pos_traj=e_traj, types_exact=bool(v_same))
            assert v_same
            assert e_pos < POS_TOL and e_cond < POS_TOL and e_traj < POS_TOL
    finally:
        for k, v in MODES["exact"].items():
            m.set_option(k, v)


@pytest.mark.parametrize("use_graph", (True, False))
def test_one_group_is_the_single_mesh_chain(use_graph):
    """G = 1 identity: one group that spans the whole batch is bit-identical to the single-mesh call, with fed draws and with
    device Philox draws on the same seed (same key: the batch-global atom, same counter domain).  Both forms run the group
    kernels, so both are also compared, to the bit, with what the single-mesh kernels gave before they were removed
    (tests/golden/make_golden_guided_single_bits.py)."""
    m = hip_model()
    c = golden("chain_mesh_guided_b4_s20.npz")
    mf = golden("mesh_fixture.npz")
    bits = golden("guided_single_bits.npz")
    mesh, cloud = (mf["verts"], mf["faces"]), mf["cloud"]
    bb, eps, u, B, S = fixture_inputs(c)
    for tag, extra in (("fed", dict(guide_draws=T(c["draws"], DEV))), ("philox", dict(seed=int(bits["seed"])))):
        kw = dict(use_graph=use_graph, grad_step=int(c["grad_step"]), **extra)
        a = run(m, bb, eps, u, B, S, use_mesh_data=(mesh, cloud, None), **kw)
        b = run(m, bb, eps, u, B, S, use_mesh_data=[(mesh, cloud, None, B)], **kw)
        assert torch.equal(a["pos"], b["pos"]) and torch.equal(a["v"], b["v"])
        for k in ("pos_traj", "v_traj", "v0_traj", "vt_traj", "pos_cond_traj", "v_cond_traj"):
            assert torch.equal(torch.stack(a[k]), torch.stack(b[k])), k
        assert torch.equal(a["pos"].cpu(), T(bits[f"mesh_{tag}_pos"])), tag
        assert torch.equal(a["v"].cpu(), T(bits[f"mesh_{tag}_v"]).long()), tag
        assert torch.equal(torch.stack(a["pos_cond_traj"]).cpu(), T(bits[f"mesh_{tag}_pos_cond_traj"])), tag
        if "guide_draws" in extra:
            assert maxabs(a["pos"], c["pos"]) < POS_TOL
    assert maxabs(a["pos"], c["pos"]) > 1e-3          # (the Philox chain is a different chain than the fixture's)


def test_mixed_batch_is_independent_in_eval_mode():
    """Independence: after model.eval() the mixed B = 6 chain equals, molecule by molecule, each group's own single-mesh chain on
    the same per-atom noise and draws (types exact, positions within the chain gate); the group without a mesh equals the
    unguided chain of the batch, the guided groups differ from it."""
    m = eval_model()
    for name in CHAINS:
        c = golden(name)
        bb, eps, u, B, S = fixture_inputs(c)
        kw = dict(grad_step=int(c["grad_step"]))
        groups = mesh_groups(c)
        mixed = run(m, bb, eps, u, B, S, use_mesh_data=groups, guide_draws=T(c["draws"], DEV), **kw)
        plain = run(m, bb, eps, u, B, S)
        mol_off, atom_off = atom_ranges(bb["counts"], c["group_mols"])
        worst = 0.0
        for g, (mesh, cloud, _, n_mols) in enumerate(groups):
            lo, hi = int(atom_off[g]), int(atom_off[g + 1])
            if mesh is None:
                alone = {k: (plain[k][lo:hi] if k in ("pos", "v") else [x[lo:hi] for x in plain[k]]) for k in ("pos", "v", "v_traj", "pos_cond_traj")}
            else:
                sub, e_, u_, d_ = sub_batch(bb, eps, u, c["draws"], int(mol_off[g]), int(mol_off[g + 1]), lo, hi)
                alone = run(m, sub, e_, u_, n_mols, S, use_mesh_data=(mesh, cloud, None), guide_draws=T(d_, DEV), **kw)
                assert maxabs(mixed["pos"][lo:hi], plain["pos"][lo:hi]) > 1e-3, g          # guidance reached the group
            assert torch.equal(alone["v"], mixed["v"][lo:hi]), g
            assert torch.equal(torch.stack(alone["v_traj"]), torch.stack(mixed["v_traj"])[:, lo:hi]), g
            worst = max(worst, maxabs(alone["pos"], mixed["pos"][lo:hi]),
                        maxabs(torch.stack(alone["pos_cond_traj"]), torch.stack(mixed["pos_cond_traj"])[:, lo:hi]))
        print(f"mixed_mesh_batch_independence {name}: max |dpos| {worst:.3e}")
        record("mixed_mesh_batch_independence", fixture=name, max_dpos=worst)
        assert worst < POS_TOL
    # a list of groups without any mesh is the unguided chain
    none = run(m, bb, eps, u, B, S, use_mesh_data=[(None, None, None, 4), (None, None, None, 2)], grad_step=990)
    assert torch.equal(none["pos"], plain["pos"]) and torch.equal(none["v"], plain["v"])


def test_group_without_atoms_inside_raises_mesh_guidance_error():
    """Error path: a group whose mesh encloses none of its atoms raises MeshGuidanceError (a ValueError), from the function (the
    other groups guided as before, the failing group untouched) and from the chain; the library names a malformed group; the
    context then runs an unguided chain correctly."""
    from shapemol_amd import _lib
    m = hip_model()
    c = golden(CHAINS[0])
    bb, eps, u, B, S = fixture_inputs(c)
    base = run(m, bb, eps, u, B, S)
    groups = mesh_groups(c)
    far = list(groups)
    far[1] = ((groups[1][0][0] + 100.0, groups[1][0][1]), groups[1][1] + 100.0, None, groups[1][3])
    _, atom_off = atom_ranges(bb["counts"], c["group_mols"])
    lo, hi = int(atom_off[1]), int(atom_off[2])
    pos = T(c["fn_pred"].copy(), DEV)
    with pytest.raises(_lib.MeshGuidanceError, match=r"group 1 in 1 step\(s\)") as ei:
        m.mesh_shape_guidance_groups(far, pos, T(bb["batch"], DEV), draws=T(c["draws"][0], DEV))
    assert ei.value.group_steps.tolist() == [0, 1, 0]
    got = pos.cpu().numpy()
    assert np.array_equal(got[lo:hi], c["fn_pred"][lo:hi])
    assert maxabs(got[:lo], c["fn_out"][:lo]) <= FN_TOL and maxabs(got[hi:], c["fn_out"][hi:]) <= FN_TOL
    with pytest.raises(ValueError, match=r"group 1 in 9 step\(s\)") as ei:          # the chain: every guided step, that group only
        run(m, bb, eps, u, B, S, use_mesh_data=far, grad_step=int(c["grad_step"]), guide_draws=T(c["draws"], DEV))
    assert isinstance(ei.value, _lib.MeshGuidanceError) and ei.value.group_steps.tolist() == [0, 9, 0]
    with pytest.raises(ValueError, match="the groups hold 4 molecules, batch_ligand names 6"):       # groups that do not cover the batch
        m.mesh_shape_guidance_groups([groups[0], groups[1]], T(c["fn_pred"].copy(), DEV), T(bb["batch"], DEV))
    ok = m.mesh_shape_guidance_groups(groups, T(c["fn_pred"].copy(), DEV), T(bb["batch"], DEV), draws=T(c["draws"][0], DEV))
    assert maxabs(ok, c["fn_out"]) <= FN_TOL                       # the call returns normally otherwise
    # host validation names the group
    bad = list(groups)
    bad[2] = (groups[2][0], groups[2][1][:2], None, 2)
    with pytest.raises(_lib.ShapeMolLibraryError, match=r"group 2: the cloud needs 3 \.\. 2048 points"):
        run(m, bb, eps, u, B, S, use_mesh_data=bad, grad_step=990)
    f_bad = groups[1][0][1].copy()
    f_bad[7, 1] = f_bad[7, 0]
    bad[2], bad[1] = groups[2], ((groups[1][0][0], f_bad), groups[1][1], None, 3)
    with pytest.raises(_lib.ShapeMolLibraryError, match=r"group 1: face 7 repeats a vertex"):
        run(m, bb, eps, u, B, S, use_mesh_data=bad, grad_step=990)
    from shapemol_amd.guidance import _clear_guidance, _install_guidance, _mesh_guidance_groups
    lib, ctx = _lib.load(), m._context(torch.device(DEV))
    _install_guidance(lib, ctx, "mesh_groups", _mesh_guidance_groups([(groups[0][0], groups[0][1], None, 5)], 5), 990, None)
    try:
        with pytest.raises(_lib.ShapeMolLibraryError, match="n_mols = 6 but the mesh guidance groups cover 5 molecules"):
            run(m, bb, eps, u, B, S)
    finally:
        _clear_guidance(lib, ctx, "mesh_groups")
    assert torch.equal(run(m, bb, eps, u, B, S)["pos"], base["pos"])


def test_graph_capture_per_mesh_set():
    """Graph reuse, as DESIGN.md section 13 states it: installing a set of meshes drops the captured step, exactly as installing
    a single mesh does, so a chain with a new set of meshes and the same (N, B) captures as often as a single-mesh chain does --
    the one-step and the unrolled executable, once per chain -- and nothing is captured beyond that."""
    m = hip_model()
    c = golden(CHAINS[0])
    bb, eps, u, B, S = fixture_inputs(c)
    groups = mesh_groups(c)
    kw = dict(grad_step=int(c["grad_step"]), guide_draws=T(c["draws"], DEV))
    caps = lambda: int(m.debug_read("captures", (1,), np.int64)[0])      # noqa: E731
    run(m, bb, eps, u, B, S, use_mesh_data=groups, **kw)
    c0 = caps()
    run(m, bb, eps, u, B, S, use_mesh_data=[groups[0][:3] + (4,), groups[2][:3] + (2,)], **kw)      # another set, same (N, B)
    c1 = caps()
    run(m, bb, eps, u, B, S, use_mesh_data=(groups[1][0], groups[1][1], None), **kw)               # the single-mesh path
    c2 = caps()
    print(f"graph_capture_per_mesh_set: grouped {c1 - c0} single {c2 - c1}")
    assert c1 - c0 == c2 - c1 == 2


# ---- the driver ---------------------------------------------------------------------------------------------------
N_COND, N_SAMPLES, BATCH, STEPS, GRAD_STEP = 3, 4, 7, 6, 996


def test_driver_matches_the_direct_list_call():
    """sample_diffusion_ligand_multi with mesh conditions (condition 1 unguided, straddling the two batches) returns
    per-condition 9-tuples whose molecules equal the direct sample_diffusion list call of every batch on the same seeds."""
    from shapemol_amd.sampling import guidance_groups, plan_batches, plan_guidance, sample_diffusion_ligand_multi
    m = hip_model()
    ms = meshes()
    shapes = synth.hash_normal((N_COND, 32, 3), 103, 77)
    conds = [(shapes[0], None, ((ms[0][0], ms[0][1]), ms[0][2], None)), (shapes[1], None), (shapes[2], None, ((ms[2][0], ms[2][1]), ms[2][2], None))]
    counts = [[14, 17, 15, 16], [18, 13, 16, 15], [15, 15, 19, 14]]
    funcs = lambda: [lambda n, it=iter(cs): [next(it) for _ in range(n)] for cs in counts]      # noqa: E731
    torch.manual_seed(41)
    multi = sample_diffusion_ligand_multi(m, conds, N_SAMPLES, batch_size=BATCH, device=DEV, num_steps=STEPS, sample_func=funcs(),
                                          sample_num_atoms="size", seed=3, grad_step=GRAD_STEP)
    assert len(multi) == N_COND and all(len(o) == 9 for o in multi)
    assert [len(o[6]) for o in multi] == [1, 2, 1]
    # the same job by hand: the driver's draw order (initial coordinates, then the initial types) from the same generator state
    from shapemol_amd import sampling
    kind, data = plan_guidance(conds)
    torch.manual_seed(41)
    it = [iter(cs) for cs in counts]
    direct = [[] for _ in range(N_COND)]
    for i, segs in enumerate(plan_batches(N_COND, N_SAMPLES, BATCH)):
        n_at = [next(it[c]) for c, _f, n in segs for _ in range(n)]
        batch = torch.repeat_interleave(torch.arange(len(n_at)), torch.tensor(n_at)).to(DEV)
        pos0 = torch.randn(sum(n_at), 3).to(DEV)
        v0 = sampling._initial_types(m, sum(n_at), torch.device(DEV), False)
        key, groups = guidance_groups(kind, data, segs)
        assert key == "use_mesh_data"
        r = m.sample_diffusion(pos0, v0, batch, torch.cat([T(shapes[c]).float().reshape(1, -1).repeat(n, 1) for c, _f, n in segs]).to(DEV),
                               num_steps=STEPS, center_pos_mode="none", grad_step=GRAD_STEP, seed=3 + i, use_mesh_data=groups)
        off = np.concatenate([[0], np.cumsum(n_at)])
        k = 0
        for c, _f, n in segs:
            for _ in range(n):
                direct[c].append((r["pos"][off[k]:off[k + 1]].cpu().numpy(), r["v"][off[k]:off[k + 1]].cpu().numpy()))
                k += 1
    for c in range(N_COND):
        assert len(multi[c][0]) == len(direct[c]) == N_SAMPLES
        for k in range(N_SAMPLES):
            assert multi[c][0][k].shape == (counts[c][k], 3) and multi[c][2][k].shape == (STEPS, counts[c][k], 3)
            assert np.array_equal(multi[c][1][k], direct[c][k][1]), (c, k)
            assert np.array_equal(multi[c][0][k].astype(np.float32), direct[c][k][0]), (c, k)
    # guidance reached the mesh conditions only (eval-free check on the guided prediction of the first step would need the
    # unguided twin; here: the unguided twin of the job differs in conditions 0 and 2)
    torch.manual_seed(41)
    plain = sample_diffusion_ligand_multi(m, [(s, None) for s, *_ in conds], N_SAMPLES, batch_size=BATCH, device=DEV, num_steps=STEPS,
                                          sample_func=funcs(), sample_num_atoms="size", seed=3, grad_step=GRAD_STEP)
    diff = [max(float(np.abs(a - b).max()) for a, b in zip(multi[c][0], plain[c][0])) for c in range(N_COND)]
    print(f"mesh driver guided vs unguided twin: {diff}")
    assert diff[0] > 1e-3 and diff[2] > 1e-3
    with pytest.raises(ValueError, match="mix meshes and point clouds"):
        sample_diffusion_ligand_multi(m, [conds[0], (shapes[1], (ms[1][2], None, 0.2))], N_SAMPLES, device=DEV)
