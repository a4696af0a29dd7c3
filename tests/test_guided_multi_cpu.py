"""Point-cloud guidance with one cloud per group of molecules, the parts that need no GPU: the fixtures of
tests/golden/make_golden_guided_multi.py (self-consistency against the oracle's single-cloud function applied per group, and the
conditions the generator promises), the argument checks of sample_diffusion, and the driver's packing."""
import numpy as np
import pytest
import torch

from util import O, golden, model_cfg, synth

FIXTURES = ("chain_guided_multi_b6_s20.npz", "chain_guided_multi_b6_s20_gap.npz")


def group_ranges(c):
    """[(atom_lo, atom_hi, cloud or None, radius)] of a fixture."""
    counts = synth.synthetic_batch(int(c["B"]), seed=int(c["seed"]))["counts"]
    mol_off = np.concatenate([[0], np.cumsum(c["group_mols"])])
    atom_off = np.concatenate([[0], np.cumsum(counts)])[mol_off]
    out = []
    for g in range(len(c["group_mols"])):
        cloud = c["clouds"][c["cloud_off"][g]:c["cloud_off"][g + 1]] if c["has_cloud"][g] else None
        out.append((int(atom_off[g]), int(atom_off[g + 1]), cloud, float(c["radii"][g])))
    return out


def pulls_per_atom(cloud, radius, pred, draws):
    """How many pulls each atom takes (0 = not moved), by the oracle's function run with 0 .. 5 iterations' worth of draws."""
    d2 = ((pred[:, None, :].astype(np.float64) - cloud[None]) ** 2).sum(-1)
    far = np.sqrt(np.sort(d2, 1)[:, :3]).mean(1) > radius
    n = np.zeros(len(pred), dtype=np.int64)
    pts = pred.astype(np.float64)
    for j in range(5):
        if not far.any():
            break
        d2 = ((pts[:, None, :] - cloud[None]) ** 2).sum(-1)
        idx = np.argsort(d2, axis=1, kind="stable")[:, :3]
        nearest = cloud[idx].mean(1)
        scalar = (draws[j] * 0.6 + 0.2)[:, None]
        pts = np.where(far[:, None], pts - scalar * (pts - nearest), pts)
        n += far
        d2 = ((pts[:, None, :] - cloud[None]) ** 2).sum(-1)
        far = far & ~(np.sqrt(np.sort(d2, 1)[:, :3]).mean(1) < radius)
    return n


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_is_self_consistent(name):
    """The oracle's single-cloud function, unchanged, applied per group to the recorded first-step prediction with the recorded
    draws reproduces the reference's recorded output exactly; a group without a cloud is untouched."""
    c = golden(name)
    assert c["fn_pred"].dtype == np.float32 and c["draws"].shape == (int(c["S"]), 5, len(c["fn_pred"]))
    out = c["fn_pred"].copy()
    for lo, hi, cloud, radius in group_ranges(c):
        if cloud is not None:
            out[lo:hi] = O.pointcloud_shape_guidance(cloud, radius, c["fn_pred"][lo:hi], c["draws"][0][:, lo:hi])
    assert np.array_equal(out, c["fn_out"])
    for lo, hi, cloud, _ in group_ranges(c):
        if cloud is None:
            assert np.array_equal(c["fn_out"][lo:hi], c["fn_pred"][lo:hi])


def test_fixture_layout():
    c, g = golden(FIXTURES[0]), golden(FIXTURES[1])
    assert int(c["B"]) == 6 and c["group_mols"].tolist() == [1, 3, 2] and int(c["S"]) == 20 and int(c["grad_step"]) == 990
    assert c["has_cloud"].tolist() == [True, True, True] and g["has_cloud"].tolist() == [True, False, True]
    sizes = np.diff(c["cloud_off"])
    assert len(set(sizes.tolist())) == 3 and sizes.min() >= 3 and sizes.max() <= 2048
    assert len(set(c["radii"].tolist())) == 2
    centres = [c["clouds"][c["cloud_off"][k]:c["cloud_off"][k + 1]].mean(0) for k in range(3)]
    assert min(np.abs(centres[a] - centres[b]).max() for a in range(3) for b in range(a)) > 0.2


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_guidance_bites_in_every_group(name):
    """In every guided step every group that has a cloud moves at least one atom, and at least one atom somewhere needs two or
    more pulls.  Checked on the stored steps whose prediction is in the file (pos_cond_traj holds the GUIDED prediction, as in
    the reference, whose guidance writes into the tensor the trajectory keeps; so the first step is checked from fn_pred, and
    every guided step through the draws the recorder scattered: an atom's draw differs from the 0.5 filler iff it was pulled)."""
    c = golden(name)
    guided_steps = int(c["guided_steps"])
    assert guided_steps == 999 - int(c["grad_step"]) == 9
    filler = c["draws"] != 0.5                                     # (S, 5, N): drawn entries
    assert not filler[guided_steps:].any()
    multi = False
    for lo, hi, cloud, radius in group_ranges(c):
        drawn = filler[:guided_steps, :, lo:hi]
        if cloud is None:
            assert not drawn.any()
            continue
        assert (drawn[:, 0].sum(1) > 0).all()                      # a moved atom in every guided step
        multi |= bool(drawn[:, 1].any())
        n = pulls_per_atom(cloud, radius, c["fn_pred"][lo:hi], c["draws"][0][:, lo:hi])       # the first step, from the prediction
        assert np.array_equal(n, drawn[0].sum(0)) and (n > 0).any()
        assert np.array_equal(n > 0, (c["fn_out"][lo:hi] != c["fn_pred"][lo:hi]).any(1))
    assert multi


class _NoLibrary(RuntimeError):
    pass


def _cpu_model(monkeypatch):
    import shapemol_amd
    from shapemol_amd import _lib

    def no_load():
        raise _NoLibrary("the library must not be loaded by an argument check")
    monkeypatch.setattr(_lib, "load", no_load)
    return shapemol_amd.ScorePosNet3D(model_cfg(), 15)


def test_argument_checks_raise_before_the_library_is_loaded(monkeypatch):
    m = _cpu_model(monkeypatch)
    bb = synth.synthetic_batch(6, seed=31)
    args = (torch.from_numpy(bb["init_pos"]), torch.from_numpy(bb["init_v"]), torch.from_numpy(bb["batch"]),
            torch.from_numpy(bb["shape"]).view(6, -1))
    cloud = np.zeros((8, 3))
    with pytest.raises(ValueError, match="5 molecules, the batch has 6"):
        m.sample_diffusion(*args, num_steps=2, use_pointcloud_data=[(cloud, None, 0.2, 2), (None, None, None, 3)])
    with pytest.raises(ValueError, match="7 molecules, the batch has 6"):
        m.sample_diffusion(*args, num_steps=2, use_pointcloud_data=[(cloud, None, 0.2, 7)])
    with pytest.raises(ValueError, match=r"use_pointcloud_data\[1\] must be"):
        m.sample_diffusion(*args, num_steps=2, use_pointcloud_data=[(cloud, None, 0.2, 3), (cloud, None, 0.2)])
    with pytest.raises(ValueError, match="empty"):
        m.sample_diffusion(*args, num_steps=2, use_pointcloud_data=[])
    with pytest.raises(NotImplementedError, match="mesh guidance takes one mesh per chain"):
        m.sample_diffusion(*args, num_steps=2, use_pointcloud_data=[(cloud, None, 0.2, 6)], use_mesh_data=(object(), cloud, None))
    # a well-formed list passes the checks and gets as far as the device check (no CPU path)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.sample_diffusion(*args, num_steps=2, use_pointcloud_data=[(cloud, None, 0.2, 4), (None, None, None, 2)])


def test_group_arrays():
    from shapemol_amd.guidance import _guidance_groups
    a, b = np.arange(12.0).reshape(4, 3), np.arange(9.0).reshape(3, 3) + 100
    mol_off, clouds, cloud_off, radii = _guidance_groups([(a, None, 0.2, 2), (None, None, None, 1), (b, "tree", 0.3, 4)], 7)
    assert mol_off.tolist() == [0, 2, 3, 7] and mol_off.dtype == np.int64
    assert cloud_off.tolist() == [0, 4, 4, 7] and cloud_off.dtype == np.int64
    assert clouds.dtype == np.float64 and clouds.flags["C_CONTIGUOUS"] and np.array_equal(clouds, np.concatenate([a, b]))
    assert radii[0] == 0.2 and radii[2] == 0.3 and radii[1] > 0


@pytest.mark.parametrize("n_cond,num_samples,batch_size", [(3, 5, 8), (3, 5, 4), (16, 50, 256), (16, 50, 800), (2, 7, 1), (4, 3, 100),
                                                            (5, 6, 6), (7, 11, 13)])
def test_plan_batches_is_a_bijection(n_cond, num_samples, batch_size):
    """Condition-major packing and per-condition unpacking: every (condition, sample) appears exactly once, in order, batches are
    full except the last, and segments of a batch are contiguous runs of conditions."""
    from shapemol_amd.sampling import plan_batches
    plan = plan_batches(n_cond, num_samples, batch_size)
    total = n_cond * num_samples
    assert len(plan) == -(-total // batch_size)
    flat = []
    for i, segs in enumerate(plan):
        size = sum(n for _c, _f, n in segs)
        assert size == (batch_size if i < len(plan) - 1 else total - batch_size * (len(plan) - 1))
        assert all(n > 0 and 0 <= f and f + n <= num_samples for _c, f, n in segs)
        assert [c for c, _f, _n in segs] == list(range(segs[0][0], segs[-1][0] + 1))
        flat += [(c, f + k) for c, f, n in segs for k in range(n)]
    assert flat == [(c, k) for c in range(n_cond) for k in range(num_samples)]
    # unpacking: what the driver does with a batch's per-molecule list
    per_cond = [[] for _ in range(n_cond)]
    m = 0
    for segs in plan:
        mols = list(range(m, m + sum(n for _c, _f, n in segs)))
        off = 0
        for c, _f, n in segs:
            per_cond[c] += mols[off:off + n]
            off += n
        m += len(mols)
    assert per_cond == [list(range(c * num_samples, (c + 1) * num_samples)) for c in range(n_cond)]
    if (n_cond, num_samples, batch_size) == (3, 5, 8):
        assert plan == [[(0, 0, 5), (1, 0, 3)], [(1, 3, 2), (2, 0, 5)]]          # condition 1 straddles the two batches


def test_plan_batches_rejects_empty_jobs():
    from shapemol_amd.sampling import plan_batches
    for bad in ((0, 5, 8), (3, 0, 8), (3, 5, 0)):
        with pytest.raises(ValueError):
            plan_batches(*bad)


def test_header_declares_the_entry_point():
    import os
    import re
    from util import ROOT
    from shapemol_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "shapemol_hip.h")).read()
    assert re.search(r"\bint shapemol_set_guidance_groups\(shapemol_ctx \*ctx, int32_t n_groups, const int64_t \*h_mol_off,", hdr)
    assert "shapemol_set_guidance_groups" in _lib.EXPORTS and "shapemol_guide_points_groups" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 5
