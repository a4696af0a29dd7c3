"""Point-cloud shape guidance with one cloud per group of molecules on the device: sample_diffusion(use_pointcloud_data=[...]),
shapemol_set_guidance_groups and sample_diffusion_ligand_multi against the reference's chains of
tests/golden/make_golden_guided_multi.py and against today's single-cloud path.
Run on the GPU box:  pytest tests/test_gpu_guided_multi.py -m gpu"""
import numpy as np
import pytest
import torch

from util import T, golden, hash_noise, hip_model, maxabs, model_cfg, record, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POS_TOL = 1e-4      # the project's chain gate: coordinates within 1e-4 abs, atom types exact
FIXTURES = ("chain_guided_multi_b6_s20.npz", "chain_guided_multi_b6_s20_gap.npz")


def fixture_inputs(c):
    B, S, seed = int(c["B"]), int(c["S"]), int(c["seed"])
    bb = synth.synthetic_batch(B, seed=seed)
    eps, u = hash_noise(len(bb["batch"]), S, seed)
    return bb, eps, u, B, S


def fixture_groups(c):
    """The list form of use_pointcloud_data of a fixture: [(cloud or None, None, radius, n_mols)]."""
    return [(c["clouds"][c["cloud_off"][g]:c["cloud_off"][g + 1]] if c["has_cloud"][g] else None, None, float(c["radii"][g]),
             int(c["group_mols"][g])) for g in range(len(c["group_mols"]))]


def atom_ranges(bb, group_mols):
    mol_off = np.concatenate([[0], np.cumsum(group_mols)])
    return mol_off, np.concatenate([[0], np.cumsum(bb["counts"])])[mol_off]


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
    """Molecules mol_lo .. mol_hi - 1 (atoms lo .. hi - 1) of a batch as a batch of their own, with their noise and draws."""
    sub = dict(init_pos=bb["init_pos"][lo:hi], init_v=bb["init_v"][lo:hi], batch=bb["batch"][lo:hi] - mol_lo,
               shape=bb["shape"][mol_lo:mol_hi], counts=bb["counts"][mol_lo:mol_hi])
    return sub, eps[:, lo:hi], u[:, lo:hi], None if draws is None else np.ascontiguousarray(draws[:, :, lo:hi])


@pytest.mark.parametrize("name", FIXTURES)
def test_grouped_chain_golden(name):
    """1. Reference parity: the fixture chain with the grouped list and the recorded draws, with and without the captured graph.
    Measured on an MI355X: final positions 3.6e-7 / 2.4e-7 (all groups guided / middle group without a
    cloud), pos_cond_traj 8.3e-7 / 9.5e-7, pos_traj 3.6e-7 / 2.4e-7, the same with and without the graph; types exact."""
    m = hip_model()
    c = golden(name)
    bb, eps, u, B, S = fixture_inputs(c)
    for use_graph in (True, False):
        r = run(m, bb, eps, u, B, S, use_graph=use_graph, use_pointcloud_data=fixture_groups(c), grad_step=int(c["grad_step"]),
                guide_draws=T(c["draws"], DEV))
        ts = c["traj_steps"]
        e_pos = maxabs(r["pos"], c["pos"])
        e_cond = maxabs(torch.stack(r["pos_cond_traj"])[ts], c["pos_cond_traj"])
        e_traj = maxabs(torch.stack(r["pos_traj"])[ts], c["pos_traj"])
        print(f"grouped_chain_golden {name} use_graph={use_graph}: pos {e_pos:.3e} pos_cond_traj {e_cond:.3e} pos_traj {e_traj:.3e}")
        record("grouped_chain_golden", fixture=name, use_graph=use_graph, pos_end=e_pos, pos_cond_traj=e_cond, pos_traj=e_traj)
        assert np.array_equal(r["v"].cpu().numpy(), c["v"])
        assert np.array_equal(torch.stack(r["v_traj"]).numpy(), c["v_traj"])
        assert e_pos < POS_TOL and e_cond < POS_TOL and e_traj < POS_TOL


@pytest.mark.parametrize("name", FIXTURES)
def test_grouped_function_golden(name):
    """2. Function level: one guided step on the recorded first-step prediction equals the reference's output bit for bit."""
    m = hip_model()
    c = golden(name)
    bb = synth.synthetic_batch(int(c["B"]), seed=int(c["seed"]))
    pos = T(c["fn_pred"].copy(), DEV)
    out = m.pointcloud_shape_guidance_groups(fixture_groups(c), pos, T(bb["batch"], DEV), draws=T(c["draws"][0], DEV))
    assert out.data_ptr() == pos.data_ptr()
    got = out.cpu().numpy()
    moved_ref = (c["fn_out"] != c["fn_pred"]).any(1)
    assert np.array_equal((got != c["fn_pred"]).any(1), moved_ref) and moved_ref.sum() > 50
    err = float(np.abs(got.astype(np.float64) - c["fn_out"]).max())
    print(f"grouped_function_golden {name}: moved {int(moved_ref.sum())} max_err {err:.3e}")
    record("grouped_function_golden", fixture=name, moved=int(moved_ref.sum()), max_err=err)
    assert err == 0.0 and np.array_equal(got, c["fn_out"])
    # device Philox: deterministic per seed, keyed by the batch-global atom, and the same atoms move
    a = m.pointcloud_shape_guidance_groups(fixture_groups(c), T(c["fn_pred"].copy(), DEV), T(bb["batch"], DEV), seed=5).cpu().numpy()
    b = m.pointcloud_shape_guidance_groups(fixture_groups(c), T(c["fn_pred"].copy(), DEV), T(bb["batch"], DEV), seed=5).cpu().numpy()
    d = m.pointcloud_shape_guidance_groups(fixture_groups(c), T(c["fn_pred"].copy(), DEV), T(bb["batch"], DEV), seed=6).cpu().numpy()
    assert np.array_equal(a, b) and not np.array_equal(a, d) and np.array_equal((a != c["fn_pred"]).any(1), moved_ref)


@pytest.mark.parametrize("use_graph", (True, False))
def test_one_group_is_the_single_cloud_chain(use_graph):
    """3. Degenerate grouping: one group that spans the whole batch is bit-identical to the tuple form, with fed draws and with
    device Philox draws (same key: the batch-global atom).  Both forms run the group kernel, so both are also compared, to the
    bit, with what the single-cloud kernel gave before it was removed (tests/golden/make_golden_guided_single_bits.py)."""
    m = hip_model()
    c = golden("chain_guided_b4_s20.npz")
    bits = golden("guided_single_bits.npz")
    bb, eps, u, B, S = fixture_inputs(c)
    cloud, radius = c["cloud"], float(c["radius"])
    for tag, extra in (("fed", dict(guide_draws=T(c["draws"], DEV))), ("philox", dict(seed=int(bits["seed"])))):
        kw = dict(use_graph=use_graph, grad_step=int(c["grad_step"]), **extra)
        a = run(m, bb, eps, u, B, S, use_pointcloud_data=(cloud, None, radius), **kw)
        b = run(m, bb, eps, u, B, S, use_pointcloud_data=[(cloud, None, radius, B)], **kw)
        assert torch.equal(a["pos"], b["pos"]) and torch.equal(a["v"], b["v"])
        for k in ("pos_traj", "v_traj", "v0_traj", "vt_traj", "pos_cond_traj", "v_cond_traj"):
            assert torch.equal(torch.stack(a[k]), torch.stack(b[k])), k
        assert torch.equal(a["pos"].cpu(), T(bits[f"cloud_{tag}_pos"])), tag
        assert torch.equal(a["v"].cpu(), T(bits[f"cloud_{tag}_v"]).long()), tag
        assert torch.equal(torch.stack(a["pos_cond_traj"]).cpu(), T(bits[f"cloud_{tag}_pos_cond_traj"])), tag
    assert maxabs(a["pos"], c["pos"]) > 1e-3          # (the Philox chain is a different chain than the fixture's)


@pytest.mark.parametrize("use_graph", (True, False))
def test_mixed_batch_is_independent_in_eval_mode(use_graph):
    """4. After model.eval() the mixed B = 6 chain equals, molecule by molecule, the three single-condition chains run through
    the tuple path on the same per-atom noise and draws.  The issue's gate is types exact and positions within 1e-4; the difference
    measured on an MI355X is exactly 0, so the test demands equality."""
    m = eval_model()
    c = golden(FIXTURES[0])
    bb, eps, u, B, S = fixture_inputs(c)
    kw = dict(use_graph=use_graph, grad_step=int(c["grad_step"]))
    mixed = run(m, bb, eps, u, B, S, use_pointcloud_data=fixture_groups(c), guide_draws=T(c["draws"], DEV), **kw)
    mol_off, atom_off = atom_ranges(bb, c["group_mols"])
    worst = 0.0
    for g, (cloud, _, radius, n_mols) in enumerate(fixture_groups(c)):
        lo, hi = int(atom_off[g]), int(atom_off[g + 1])
        sub, e_, u_, d_ = sub_batch(bb, eps, u, c["draws"], int(mol_off[g]), int(mol_off[g + 1]), lo, hi)
        alone = run(m, sub, e_, u_, n_mols, S, use_pointcloud_data=(cloud, None, radius), guide_draws=T(d_, DEV), **kw)
        assert torch.equal(alone["v"], mixed["v"][lo:hi]), g
        assert torch.equal(torch.stack(alone["v_traj"]), torch.stack(mixed["v_traj"])[:, lo:hi]), g
        worst = max(worst, maxabs(alone["pos"], mixed["pos"][lo:hi]),
                    maxabs(torch.stack(alone["pos_cond_traj"]), torch.stack(mixed["pos_cond_traj"])[:, lo:hi]))
    print(f"mixed_batch_independence use_graph={use_graph}: max |dpos| {worst:.3e}")
    record("mixed_batch_independence", use_graph=use_graph, max_dpos=worst)
    assert worst == 0.0


def test_negative_control_one_cloud_for_all():
    """5. The same chain with group 0's cloud applied to every molecule (the only option before groups) misses the fixture by more
    than the gate on an atom of another group: the parity test cannot pass on a kernel that ignores the grouping."""
    m = hip_model()
    c = golden(FIXTURES[0])
    bb, eps, u, B, S = fixture_inputs(c)
    g0 = fixture_groups(c)[0]
    r = run(m, bb, eps, u, B, S, use_pointcloud_data=(g0[0], None, g0[2]), grad_step=int(c["grad_step"]), guide_draws=T(c["draws"], DEV))
    _, atom_off = atom_ranges(bb, c["group_mols"])
    err = np.abs(r["pos"].cpu().numpy().astype(np.float64) - c["pos"]).max(1)
    print(f"negative_control: max |dpos| group 0 {err[:atom_off[1]].max():.3e}, other groups {err[atom_off[1]:].max():.3e}")
    assert err[atom_off[1]:].max() > POS_TOL


def test_cloudless_group_equals_the_unguided_run():
    """6a. In eval mode the molecules of a group without a cloud equal the unguided run of those molecules (types exact, positions
    within the chain gate); the guided groups around it differ from their unguided run."""
    m = eval_model()
    c = golden(FIXTURES[1])
    bb, eps, u, B, S = fixture_inputs(c)
    mixed = run(m, bb, eps, u, B, S, use_pointcloud_data=fixture_groups(c), grad_step=int(c["grad_step"]), guide_draws=T(c["draws"], DEV))
    plain = run(m, bb, eps, u, B, S)
    _, atom_off = atom_ranges(bb, c["group_mols"])
    lo, hi = int(atom_off[1]), int(atom_off[2])
    # (not bit for bit: a chain with guidance applies the last layer's coordinate update in a kernel of its own, an unguided chain
    # inside the posterior-step kernel -- the same arithmetic in another order)
    assert torch.equal(mixed["v"][lo:hi], plain["v"][lo:hi])
    assert torch.equal(torch.stack(mixed["v_traj"])[:, lo:hi], torch.stack(plain["v_traj"])[:, lo:hi])
    err = max(maxabs(mixed["pos"][lo:hi], plain["pos"][lo:hi]),
              maxabs(torch.stack(mixed["pos_cond_traj"])[:, lo:hi], torch.stack(plain["pos_cond_traj"])[:, lo:hi]))
    print(f"cloudless_group_vs_unguided: max |dpos| {err:.3e}")
    record("cloudless_group_vs_unguided", max_dpos=err)
    assert err < POS_TOL
    assert maxabs(mixed["pos"][:lo], plain["pos"][:lo]) > 1e-3 and maxabs(mixed["pos"][hi:], plain["pos"][hi:]) > 1e-3
    # a list of cloud-less groups only is the unguided chain
    none = run(m, bb, eps, u, B, S, use_pointcloud_data=[(None, None, None, 4), (None, None, None, 2)], grad_step=int(c["grad_step"]))
    assert torch.equal(none["pos"], plain["pos"]) and torch.equal(none["v"], plain["v"])


def test_errors_name_the_group_and_leave_nothing_installed():
    """6b. Bad offsets, a 2-point cloud and an n_mols mismatch raise with the library's message; the same context then runs an
    unguided chain correctly (neither the clouds nor the caller's draws pointer stay installed)."""
    import ctypes as C
    from shapemol_amd import _lib
    m = hip_model()
    c = golden(FIXTURES[0])
    bb, eps, u, B, S = fixture_inputs(c)
    base = run(m, bb, eps, u, B, S)
    groups = fixture_groups(c)
    draws = T(c["draws"], DEV)
    with pytest.raises(_lib.ShapeMolLibraryError, match=r"group 1: the cloud needs 3 \.\. 2048 points"):
        run(m, bb, eps, u, B, S, use_pointcloud_data=[groups[0], (groups[1][0][:2], None, 0.3, 3), groups[2]], guide_draws=draws)
    with pytest.raises(_lib.ShapeMolLibraryError, match=r"group 2: the cloud needs 3 \.\. 2048 points"):
        run(m, bb, eps, u, B, S, use_pointcloud_data=[groups[0], groups[1], (np.zeros((2049, 3)), None, 0.2, 2)], guide_draws=draws)
    with pytest.raises(_lib.ShapeMolLibraryError, match=r"group 0: the radius must be > 0"):
        run(m, bb, eps, u, B, S, use_pointcloud_data=[(groups[0][0], None, 0.0, 1), groups[1], groups[2]], guide_draws=draws)
    assert torch.equal(run(m, bb, eps, u, B, S)["pos"], base["pos"])
    # the C ABI directly: offsets that decrease or do not start at 0, and a chain whose n_mols the groups do not cover
    lib, ctx = _lib.load(), m._context(torch.device(DEV))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)        # noqa: E731
    cloud = np.ascontiguousarray(groups[0][0])
    i64 = lambda *x: np.array(x, dtype=np.int64)        # noqa: E731
    rad = np.array([0.2, 0.2])
    n = len(cloud)
    with pytest.raises(_lib.ShapeMolLibraryError, match="group 1: the molecule offsets decrease"):
        _lib.check(lib.shapemol_set_guidance_groups(ctx, 2, vp(i64(0, 4, 3)), vp(cloud), vp(i64(0, n, n)), vp(rad), 990, None), "set")
    with pytest.raises(_lib.ShapeMolLibraryError, match="group 1: the cloud offsets decrease"):
        _lib.check(lib.shapemol_set_guidance_groups(ctx, 2, vp(i64(0, 4, 6)), vp(cloud), vp(i64(0, n, n - 1)), vp(rad), 990, None), "set")
    with pytest.raises(_lib.ShapeMolLibraryError, match="group 0: the molecule and cloud offsets must start at 0"):
        _lib.check(lib.shapemol_set_guidance_groups(ctx, 2, vp(i64(1, 4, 6)), vp(cloud), vp(i64(0, n, n)), vp(rad), 990, None), "set")
    assert torch.equal(run(m, bb, eps, u, B, S)["pos"], base["pos"])          # a rejected call installs nothing
    _lib.check(lib.shapemol_set_guidance_groups(ctx, 2, vp(i64(0, 3, 5)), vp(cloud), vp(i64(0, n, n)), vp(rad), 990, None), "set")
    try:
        with pytest.raises(_lib.ShapeMolLibraryError, match="n_mols = 6 but the guidance groups cover 5 molecules"):
            run(m, bb, eps, u, B, S)
    finally:
        _lib.check(lib.shapemol_set_guidance_groups(ctx, 0, None, None, None, None, 0, None), "unset")
    assert torch.equal(run(m, bb, eps, u, B, S)["pos"], base["pos"])
    # a failing grouped chain (too many steps) drops its groups too
    with pytest.raises(Exception):
        m.sample_diffusion(T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1),
                           num_steps=2000, center_pos_mode="none", use_pointcloud_data=groups, grad_step=990)
    assert torch.equal(run(m, bb, eps, u, B, S)["pos"], base["pos"])
    # groups and a single cloud replace each other: a tuple chain after a grouped one is the tuple chain
    g4 = golden("chain_guided_b4_s20.npz")
    b4, e4, u4, B4, S4 = fixture_inputs(g4)
    run(m, bb, eps, u, B, S, use_pointcloud_data=groups, grad_step=990, guide_draws=draws)
    r4 = run(m, b4, e4, u4, B4, S4, use_pointcloud_data=(g4["cloud"], None, float(g4["radius"])), grad_step=int(g4["grad_step"]),
             guide_draws=T(g4["draws"], DEV))
    assert np.array_equal(r4["v"].cpu().numpy(), g4["v"]) and maxabs(r4["pos"], g4["pos"]) < POS_TOL


# ---- the driver ---------------------------------------------------------------------------------------------------
N_COND, N_SAMPLES, BATCH, STEPS, GRAD_STEP, CLASSES = 3, 5, 8, 6, 996, 15


class MoleculeTape:
    """Per-molecule random numbers of a job, defined up front from hashes: molecule (condition, sample) has its atom count, its
    initial coordinates and type uniforms, its noise of every step and its guidance draws.  `feed(batches)` yields, for a run whose
    batches hold the given molecules, the values torch.randn / torch.rand must return in the driver's draw order."""

    def __init__(self):
        rs = np.random.RandomState(5)
        self.counts = rs.randint(12, 28, size=(N_COND, N_SAMPLES))
        self.mol = {}
        for c in range(N_COND):
            for k in range(N_SAMPLES):
                n, seed = int(self.counts[c, k]), 1000 * c + k
                eps, u = hash_noise(n, STEPS, seed)
                self.mol[c, k] = dict(pos=synth.hash_normal((n, 3), 701, seed), u0=synth.hash_uniform((n, CLASSES), 702, seed),
                                      eps=eps, u=u, draws=synth.hash_uniform((STEPS, 5, n), 703, seed).astype(np.float64))

    def cat(self, mols, key, axis=0):
        return np.concatenate([self.mol[m][key] for m in mols], axis=axis)

    def install(self, monkeypatch, model, batches):
        """Patch torch.randn / torch.rand to replay the tape for `batches` (lists of (condition, sample)), and wrap
        model.sample_diffusion to hand every chain its molecules' guidance draws."""
        normal, uniform = [], []
        for mols in batches:
            normal.append(self.cat(mols, "pos"))
            uniform.append(self.cat(mols, "u0"))
            eps, u = self.cat(mols, "eps", 1), self.cat(mols, "u", 1)
            normal += list(eps)
            uniform += list(u)
        chains = iter(batches)

        def pop(queue, shape):
            a = queue.pop(0)
            assert tuple(a.shape) == tuple(shape), (a.shape, shape)
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        monkeypatch.setattr(torch, "randn", lambda *shape: pop(normal, shape))
        monkeypatch.setattr(torch, "rand", lambda *shape: pop(uniform, shape))
        real = type(model).sample_diffusion

        def fed(*a, **kw):
            mols = next(chains)
            if kw.get("use_pointcloud_data") is not None:
                kw["guide_draws"] = T(self.cat(mols, "draws", 2), DEV)
            return real(model, *a, **kw)
        monkeypatch.setattr(model, "sample_diffusion", fed, raising=False)
        return normal, uniform


def _conditions():
    f = golden(FIXTURES[0])
    groups = fixture_groups(f)
    shapes = synth.hash_normal((N_COND, 32, 3), 103, 77)
    # condition 1 is unguided: guided and unguided conditions share the batches
    return [(shapes[0], (groups[0][0], None, groups[0][2])), (shapes[1], None), (shapes[2], (groups[2][0], None, groups[2][2]))]


def _count_funcs(tape):
    """sample_func of every condition: hands out the tape's atom counts of that condition in order, however the calls are cut."""
    its = [iter(tape.counts[c].tolist()) for c in range(N_COND)]
    return [lambda n, it=it: [next(it) for _ in range(n)] for it in its]


def test_driver_matches_per_condition_runs(monkeypatch):
    """7. sample_diffusion_ligand_multi, 3 conditions x 5 samples at batch_size 8 (condition 1 straddles the two batches),
    host_rng, model.eval(): each condition's molecules equal what sample_diffusion_ligand gives for that condition alone on
    the same per-molecule random numbers."""
    from shapemol_amd.sampling import plan_batches, sample_diffusion_ligand, sample_diffusion_ligand_multi
    m = eval_model()
    tape = MoleculeTape()
    conds = _conditions()
    batches = [[(c, f + k) for c, f, n in segs for k in range(n)] for segs in plan_batches(N_COND, N_SAMPLES, BATCH)]
    assert [len(b) for b in batches] == [8, 7]
    with monkeypatch.context() as mp:
        left = tape.install(mp, m, batches)
        multi = sample_diffusion_ligand_multi(m, conds, N_SAMPLES, batch_size=BATCH, num_steps=STEPS, sample_func=_count_funcs(tape),
                                              sample_num_atoms="size", host_rng=True, grad_step=GRAD_STEP)
        assert left == ([], [])
    assert len(multi) == N_COND
    worst = 0.0
    for c in range(N_COND):
        with monkeypatch.context() as mp:
            left = tape.install(mp, m, [[(c, k) for k in range(N_SAMPLES)]])
            alone = sample_diffusion_ligand(m, conds[c][0], N_SAMPLES, batch_size=N_SAMPLES, num_steps=STEPS,
                                            sample_func=_count_funcs(tape)[c], sample_num_atoms="size", host_rng=True,
                                            use_pointcloud_data=conds[c][1], grad_step=GRAD_STEP)
            assert left == ([], [])
        assert len(multi[c]) == 9 and len(multi[c][6]) == (2 if c == 1 else 1)
        for slot in (0, 1, 2, 3, 4, 5, 7, 8):
            assert len(multi[c][slot]) == len(alone[slot]) == N_SAMPLES
            for k in range(N_SAMPLES):
                a, b = multi[c][slot][k], alone[slot][k]
                assert a.shape == b.shape and a.dtype == b.dtype, (c, slot, k)
                if slot in (1, 3):
                    assert np.array_equal(a, b), (c, slot, k)                      # atom types exact
                elif slot in (0, 2, 7):
                    worst = max(worst, float(np.abs(a - b).max()))
    print(f"driver_matches_per_condition_runs: max |dpos| {worst:.3e}")
    record("driver_matches_per_condition_runs", max_dpos=worst)
    assert worst < POS_TOL
    # guidance reached the guided conditions only: the unguided twin of the job differs there and not in condition 1
    with monkeypatch.context() as mp:
        tape.install(mp, m, batches)
        plain = sample_diffusion_ligand_multi(m, [(s, None) for s, _ in conds], N_SAMPLES, batch_size=BATCH, num_steps=STEPS,
                                              sample_func=_count_funcs(tape), sample_num_atoms="size", host_rng=True, grad_step=GRAD_STEP)
    diff = [max(float(np.abs(a - b).max()) for a, b in zip(multi[c][0], plain[c][0])) for c in range(N_COND)]
    print(f"driver guided vs unguided twin: {diff}")
    assert diff[0] > 1e-3 and diff[2] > 1e-3 and diff[1] < POS_TOL


def test_driver_train_mode_shapes():
    """7 (train mode): the batch-norm statistics span the mixed batch, so only shapes, dtypes, counts and finiteness are checked."""
    from shapemol_amd.sampling import sample_diffusion_ligand_multi
    m = hip_model()
    assert m.training
    tape = MoleculeTape()
    out = sample_diffusion_ligand_multi(m, _conditions(), N_SAMPLES, batch_size=BATCH, num_steps=STEPS, sample_func=_count_funcs(tape),
                                        sample_num_atoms="size", seed=3, grad_step=GRAD_STEP)
    assert len(out) == N_COND
    for c, o in enumerate(out):
        pos, v, pos_traj, v_traj, v0_traj, vt_traj, times, pos_cond, v_cond = o
        assert len(times) == (2 if c == 1 else 1) and all(t > 0 for t in times)
        for k in range(N_SAMPLES):
            n = int(tape.counts[c, k])
            assert pos[k].shape == (n, 3) and pos[k].dtype == np.float64 and np.isfinite(pos[k]).all()
            assert v[k].shape == (n,) and v[k].dtype == np.int64 and v[k].min() >= 0 and v[k].max() < CLASSES
            assert pos_traj[k].shape == (STEPS, n, 3) and pos_traj[k].dtype == np.float64 and np.isfinite(pos_traj[k]).all()
            assert pos_cond[k].shape == (STEPS, n, 3) and pos_cond[k].dtype == np.float64 and np.isfinite(pos_cond[k]).all()
            assert v_traj[k].shape == (STEPS, n) and v0_traj[k].shape == vt_traj[k].shape == v_cond[k].shape == (STEPS, n, CLASSES)
            assert np.isfinite(v0_traj[k]).all() and np.isfinite(vt_traj[k]).all() and np.isfinite(v_cond[k]).all()
