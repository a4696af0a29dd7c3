"""Device memory of a sampling context across regrowth (csrc/sm_devmem.h): a context whose workspace, guidance tables and
blocks have grown computes, bit for bit, what a fresh context computes that runs only that one call; the two sets of prepared
shape data of classifier-free guidance are not left exchanged.  Reduced model (hidden_dim 32, 4 heads, 2 layers).
Run on the GPU box:  pytest tests/test_gpu_workspace.py -m gpu"""
import numpy as np
import pytest
import torch

from util import T, hash_noise, model_cfg, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REDUCED = dict(hidden_dim=32, n_heads=4, num_layers=2)
STEPS = 4
# atoms per molecule: (B = 2, N = 9), (B = 2, N = 40): capN alone grows, (B = 5, N = 40): capB alone grows, the first again:
# nothing grows and the buffers are larger than the batch.  The smallest shapes that cross each capacity separately and
# span more than one 16-atom column tile
SEQUENCE = ((4, 5), (19, 21), (7, 9, 8, 6, 10), (4, 5))
TRAJ = ("pos_traj", "v_traj", "v0_traj", "vt_traj", "pos_cond_traj", "v_cond_traj", "pos_uncond_traj", "v_uncond_traj")


def fresh(**overrides):
    """A new model, so a new library context, with the suite's synthetic weights."""
    import shapemol_amd
    cfg = model_cfg(**REDUCED, **overrides)
    m = shapemol_amd.ScorePosNet3D(cfg, 15)
    sdn = synth.synthetic_state_dict(cfg, seed=7)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=True)
    return m.to(DEV)


def batch_of(counts, seed=11):
    """(init_pos, init_v, batch, shape) on the device for molecules of the given atom counts, and the chain's fed noise."""
    counts = np.asarray(counts, np.int64)
    n, B = int(counts.sum()), len(counts)
    args = (T(synth.hash_normal((n, 3), tag=101, seed=seed), DEV), T((synth.hash_u24(n, tag=102, seed=seed) % 15).astype(np.int64), DEV),
            T(np.repeat(np.arange(B, dtype=np.int64), counts), DEV), T(synth.hash_normal((B, 32, 3), tag=103, seed=seed), DEV).view(B, -1))
    eps, u = hash_noise(n, STEPS, seed)
    return args, dict(num_steps=STEPS, center_pos_mode="none", noise=(T(eps, DEV), T(u, DEV)))


def forward(m, counts):
    pos, v, batch, shape = batch_of(counts)[0]
    t = torch.full((len(counts),), 700, dtype=torch.int64, device=DEV)
    return m(pos, v, batch, shape, time_step=t)


def chain(m, counts, **kw):
    args, base = batch_of(counts)
    return m.sample_diffusion(*args, **base, **kw)


def assert_same(got, want):
    """Every tensor (and list of tensors) of two result dicts, bit for bit."""
    assert sorted(got) == sorted(want)
    n = 0
    for k in want:
        a, b = got[k], want[k]
        if isinstance(b, (list, tuple)):
            assert len(a) == len(b), k
            if len(b) and torch.is_tensor(b[0]):
                assert all(torch.equal(x, y) for x, y in zip(a, b)), k
                n += len(b)
        elif torch.is_tensor(b):
            assert torch.equal(a, b), k
            n += 1
    assert n >= 2


def captures(m):
    return int(m.debug_read("captures", (1,), np.int64)[0])


def test_regrowth_keeps_bits_forward():
    m = fresh()
    for counts in SEQUENCE:
        assert_same(forward(m, counts), forward(fresh(), counts))


def test_regrowth_keeps_bits_captured_chain():
    """debug_read("captures") after each chain: what the commit before the one allocator reported for this sequence (every growth
    of the workspace drops both captured executables, and so does the change of batch geometry at the end)."""
    m = fresh()
    seen = []
    for counts in SEQUENCE:
        assert_same(chain(m, counts, use_graph=True), chain(fresh(), counts, use_graph=True))
        seen.append(captures(m))
    assert seen == [2, 4, 6, 8], seen


def test_shape_sets_are_not_left_exchanged():
    """A classifier-free-guidance chain (it fills and reads both sets), then an unguided chain and a forward on the same
    context: both equal a fresh context's, and so does the layer-0 shape term of set 0 that the forward left behind."""
    counts = SEQUENCE[0]
    H = REDUCED["hidden_dim"]
    m = fresh(cond_mask_prob=0.1)
    g = chain(m, counts, guide_stren=1.5, threshold_type=None, bounds=None)
    assert len(g["pos_uncond_traj"]) == STEPS
    plain = chain(m, counts)
    assert_same(plain, chain(fresh(cond_mask_prob=0.1), counts))
    assert not torch.equal(plain["pos"], g["pos"])
    f = fresh(cond_mask_prob=0.1)
    assert_same(forward(m, counts), forward(f, counts))
    add0 = m.debug_read("add0", (len(counts), 4 * H), np.float32)
    assert np.array_equal(add0, f.debug_read("add0", (len(counts), 4 * H), np.float32)) and np.abs(add0).max() > 0


def box_mesh(h):
    """An axis-aligned cube of half-width h around the origin, outward-facing triangles; vertex 4 dx + 2 dy + dz."""
    verts = np.array([[(2 * dx - 1) * h, (2 * dy - 1) * h, (2 * dz - 1) * h] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)], np.float64)
    quads = ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3))
    faces = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    return verts, faces


def cloud_of(g, n):
    return synth.hash_normal((n, 3), 501 + g, 3).astype(np.float64) * 2.0


def cloud_groups(mols):
    return dict(use_pointcloud_data=[(cloud_of(g, 64 + 37 * g), None, 0.2, n) for g, n in enumerate(mols)], grad_step=990, seed=5)


def mesh_groups(mols):
    # the cloud of a mesh: the cube's corners pulled in a little, so most atoms inside the cube are far from it
    return dict(use_mesh_data=[(box_mesh(2.0 + 0.5 * g), box_mesh(1.9 + 0.5 * g)[0], None, n) for g, n in enumerate(mols)],
                grad_step=990, seed=5)


def cfg_groups(mols):
    return dict(guide_stren=[((1.5, 0.0, 0.7)[g], n) for g, n in enumerate(mols)], threshold_type="dynamic_threshold",
                threshold_args={"p": 0.9}, bounds=None)


@pytest.mark.parametrize("kind", ("cloud", "mesh", "cfg"))
def test_guidance_blocks_regrow(kind):
    """B = 2 in two groups, then B = 4 in three on the same context: the per-workgroup table (cloud and mesh groups), the mesh
    lists and counters, and the block of the classifier-free-guidance groups (n_groups > cap) grow between the chains."""
    groups = {"cloud": cloud_groups, "mesh": mesh_groups, "cfg": cfg_groups}[kind]
    model = dict(cond_mask_prob=0.1) if kind == "cfg" else {}
    m = fresh(**model)
    for counts, mols in (((9, 11), (1, 1)), ((9, 11, 17, 10), (1, 1, 2))):
        got = chain(m, counts, **groups(mols))
        assert_same(got, chain(fresh(**model), counts, **groups(mols)))
        plain = chain(fresh(**model), counts)
        assert not torch.equal(got["pos"], plain["pos"])            # (the guidance did guide)
