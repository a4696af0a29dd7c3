"""The shape-data builder on the device (shapemol_amd/shape_data.py, csrc/sm_shape_data.h) against its float64 oracle
(tests/shape_data_oracle.py).  Run on the GPU box:  pytest tests/test_gpu_shape_data.py -m gpu

Fed draws: the face of every cloud point, the containment flag of EVERY candidate, the selected candidates and the counts are
exact; cloud, centres, bounds, points and values lie within 1 float32 ulp of the float64 oracle rounded to float32 (the
computation is float64 rounded once: only a double-rounding tie can differ).  Independently of the ray parity, the flags agree
with the winding number wherever |winding - 0.5| > 0.4 (at most 2 % of the candidates may lie within that margin).
T in {2, 5, 341}: 3T = 1023 takes four passes of the select workgroup's 256-wide scan."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mesh_oracle as M  # noqa: E402
import shape_data_oracle as S  # noqa: E402
from util import record  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ulp_ok(got, want):
    """|got - want| <= 1 ulp of float32 at `want`, element by element."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.maximum(np.abs(want), np.float32(np.finfo(np.float32).tiny))).astype(np.float64)
    return bool((err <= ulp).all()), float((err / ulp).max()) if err.size else 0.0


def _build(meshes, P, T, loss, **kw):
    from shapemol_amd.shape_data import build_batch
    out = build_batch(meshes, P, T, loss, device=DEV, debug=True, **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


@pytest.mark.parametrize("name", sorted(S.FED_CASES))
def test_fed_draws_against_the_oracle(name):
    meshes, P, T, loss, cd, qd, res = S.fed_case(name)
    got = _build(meshes, P, T, loss, cloud_draws=cd, query_draws=qd)
    worst = 0.0
    for b, ((v, f), r) in enumerate(zip(meshes, res)):
        assert np.array_equal(got["face_idx"][b], r["face_idx"])
        assert np.array_equal(got["flags"][b].astype(bool), r["flags"])             # every candidate == contains_parity
        assert np.array_equal(got["sel"][b], r["sel"])
        assert tuple(got["counts"][b]) == tuple(r["counts"])
        for key in ("cloud", "centres", "bounds", "points", "values"):
            ok, w = _ulp_ok(got[key][b], r[key])
            worst = max(worst, w)
            assert ok, (key, b, w)
        n_in = r["n_in"]
        if loss == "occupancy":
            assert (got["values"][b][:n_in] == 1.0).all() and (got["values"][b][n_in:] == 0.0).all()
        else:
            assert (got["values"][b][:n_in] >= 0).all() and (got["values"][b][n_in:] <= 0).all()     # the sign follows the row block
        if T >= 100:
            skipped, agree = S.winding_check(v, f, r["cand"], got["flags"][b])
            assert agree and skipped <= S.WINDING_SKIP_CAP
    record("shape_data_fed_" + name, worst_ulp=worst)
    if name == "tetra":
        assert res[0]["n_in"] < T // 2
    if name.startswith("tile"):
        assert len(meshes[0][1]) == int(name[4:7])              # just below, at, just above kMeshFaceTile = 512
    if name == "batch3":
        assert len({len(f) for _, f in meshes}) == 3
    if name == "batch3_twice":
        for key in ("cloud", "points", "values", "centres", "bounds", "sel", "flags"):
            assert np.array_equal(got[key][0], got[key][2]), key


@pytest.mark.parametrize("P", [1, 16, 17, 512])
def test_cloud_sizes(P):
    """P in {1, 16, 17, 512} on a batch of two meshes, clouds only (as get_pointAE_shape_emb builds them) and with T = 2."""
    meshes = [S.tile_mesh(512), S.tetrahedron()]
    cd, qd = S.draws((2, P, 3), 40 + P), S.draws((2, 6, 3), 41 + P)
    res = [S.build(v, f, cd[b], qd[b], 2) for b, (v, f) in enumerate(meshes)]
    alone = _build(meshes, P, 0, "signed_distance", cloud_draws=cd)
    full = _build(meshes, P, 2, "signed_distance", cloud_draws=cd, query_draws=qd)
    assert "points" not in alone
    for b, r in enumerate(res):
        assert np.array_equal(alone["face_idx"][b], r["face_idx"]) and np.array_equal(full["sel"][b], r["sel"])
        for key in ("cloud", "centres", "bounds"):
            assert _ulp_ok(alone[key][b], r[key])[0], key
            assert np.array_equal(alone[key][b], full[key][b]), key
        for key in ("points", "values"):
            assert _ulp_ok(full[key][b], r[key])[0], key


def test_too_few_outside_candidates_raise_and_the_context_survives():
    """A 40 A cube holds (40 / 42)^3 = 0.86 of its candidates: the outside rows (at least T / 2) cannot be filled."""
    from shapemol_amd.shape_data import ShapeData
    (tet, cube), P, T, cd, qd = S.short_case()
    r = S.build(*cube, cd[1], qd[1], T)
    assert r["short"] and r["counts"][1] < T - r["n_in"]                 # the oracle: the outside count is short
    cfg = dict(shape_type="point_cloud", point_cloud_samples=P, num_samples=T, loss_type="signed_distance")
    with pytest.raises(ValueError, match=r"shape 1 \(") as e:
        ShapeData([{"mesh": tet}, {"mesh": cube}], cfg, device=DEV, cloud_draws=cd, query_draws=qd)
    assert "shape 0" not in str(e.value) and tuple(e.value.counts[1]) == tuple(r["counts"])
    # the next call on the same context
    ok = ShapeData([{"mesh": tet}], cfg, device=DEV, cloud_draws=cd[:1], query_draws=qd[:1])
    want = S.build(*tet, cd[0], qd[0], T)
    assert _ulp_ok(ok.points[0].cpu().numpy(), want["points"])[0] and _ulp_ok(ok.values[0].cpu().numpy(), want["values"])[0]
    assert tuple(ok.counts[0]) == tuple(want["counts"])


def test_philox_mode():
    """Device-drawn uniforms: deterministic per seed; two copies of a mesh in one batch get different rows; and, recomputed from
    the outputs plus the centres, the rows obey the builder's rules under the oracle.

    The bound on |values|: the oracle sees the un-centred cloud and points as (centred float32 + centre) in float64, while the
    device measured the float64 candidate against the float32 cloud before centring.  Centring rounded every coordinate once
    (<= ulp / 2 of the centred coordinate each), so a cloud point and a query point are each displaced by <= sqrt(3) ulp / 2,
    the distance -- 1-Lipschitz in both -- by <= sqrt(3) ulp, and its own rounding to float32 adds <= ulp / 2: 2.3 ulp, taken at
    the largest magnitude among the centred coordinates, the centre and the values."""
    v, f = S.u_mesh()
    P, T = 512, 341
    a = _build([(v, f), (v, f)], P, T, "signed_distance", seed=11)
    b = _build([(v, f), (v, f)], P, T, "signed_distance", seed=11)
    c = _build([(v, f), (v, f)], P, T, "signed_distance", seed=12)
    for key in ("cloud", "points", "values", "centres", "bounds", "sel", "flags", "face_idx"):
        assert np.array_equal(a[key], b[key]), key
    assert not np.array_equal(a["cloud"], c["cloud"]) and not np.array_equal(a["points"], c["points"])
    assert not np.array_equal(a["cloud"][0], a["cloud"][1]) and not np.array_equal(a["points"][0], a["points"][1])
    tables = M.MeshTables(v, f)
    lo, hi = v.min(0), v.max(0)
    for s in range(2):
        off = a["centres"][s].astype(np.float64)
        cloud = a["cloud"][s].astype(np.float64) + off
        pts = a["points"][s].astype(np.float64) + off
        tot_in = int(a["counts"][s][0])
        n_in = min(T // 2, tot_in)
        assert a["counts"][s].sum() == 3 * T and int(a["flags"][s].sum()) == tot_in
        big = max(np.abs(a["cloud"][s]).max(), np.abs(a["points"][s]).max(), np.abs(off).max(), np.abs(a["values"][s]).max())
        ulp = float(np.spacing(np.float32(big)))
        assert (pts >= lo - 1 - ulp).all() and (pts <= hi + 1 + ulp).all()            # candidates of the grown bounding box
        w = M.winding_number(v, f, pts)
        clear = np.abs(w - 0.5) > S.WINDING_MARGIN
        assert (~clear).mean() <= S.WINDING_SKIP_CAP
        rows_in = np.arange(T) < n_in
        assert np.array_equal((w > 0.5)[clear], rows_in[clear])                       # the first n_in rows inside, the rest outside
        assert (a["values"][s][:n_in] >= 0).all() and (a["values"][s][n_in:] <= 0).all()
        d = M.nearest_dist(cloud, pts)
        err = float(np.abs(np.abs(a["values"][s].astype(np.float64)) - d).max())
        record("shape_data_philox", shape=s, dist_err=err, bound=2.3 * ulp)
        assert err <= 2.3 * ulp
        # the cloud lies on the mesh: every point on the face the kernel reports, to float32 rounding
        k = a["face_idx"][s]
        A, B, C = v[f[k, 0]], v[f[k, 1]], v[f[k, 2]]
        n = np.cross(B - A, C - A)
        plane = np.abs(np.einsum("ij,ij->i", cloud - A, n)) / np.linalg.norm(n, axis=1)
        assert plane.max() <= 2 * np.sqrt(3) * ulp
        assert not M.contains_parity(tables, pts[n_in:][clear[n_in:]]).any()


def test_area_weighting():
    """A closed mesh of 4 faces of which face 0 holds half the area: of 2 x 2048 device-drawn points, the share on face 0 lies
    within 0.5 +- 5 sqrt(0.25 / 4096)."""
    mesh = S.pillbox()
    k = np.concatenate([_build([mesh], 2048, 0, "signed_distance", seed=s)["face_idx"][0] for s in (3, 4)])
    share = float((k == 0).mean())
    record("shape_data_area_share", share=share)
    assert len(k) == 4096 and abs(share - 0.5) <= 5 * np.sqrt(0.25 / 4096)
    assert set(np.unique(k)) == {0, 1, 2, 3}


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _ae(loss_type="signed_distance"):
    import shapemol_amd
    torch.manual_seed(3)
    cfg = dict(encoder="VN_DGCNN", hidden_dim=128, latent_dim=32, layer_num=4, num_k=20, point_dim=3, loss_type=loss_type)
    return shapemol_amd.PointCloud_AE(cfg).to(DEV)


def test_batches_train_the_decoder():
    import shapemol_amd
    mesh = S.u_mesh()
    cfg = type("Cfg", (), dict(shape_type="point_cloud", point_cloud_samples=512, num_samples=64, loss_type="signed_distance"))
    data = shapemol_amd.collate_fn([{"mesh": mesh}, {"mesh": (torch.from_numpy(mesh[0]), torch.from_numpy(mesh[1]))}], cfg, device=DEV, seed=5)
    assert data.point_cloud.shape == (2, 512, 3) and data.points.shape == (2, 64, 3) and data.values.shape == (2, 64)
    assert data.point_cloud.dtype == data.points.dtype == data.values.dtype == torch.float32 and data.point_cloud.is_cuda
    assert len(data.mesh) == 2 and data.centres.shape == (2, 3) and data.bounds.shape == (2, 3, 2) and data.counts.shape == (2, 2)
    data.to(DEV)
    model = _ae()
    loss = model.get_generator_train_loss(data.point_cloud, data.points, data.values)
    loss.backward()
    assert torch.isfinite(loss)
    grads = [p.grad for p in model.generator.parameters()]
    assert grads and all(g is not None and torch.isfinite(g).all() for g in grads)
    # get_val_loss: its third scalar is the accuracy among the samples of value 1, of which a signed-distance batch has none
    # (0 / 0 by the reference's formula); the same batch -- same seed, so the same clouds and points -- with occupancy targets
    # has them, and all three scalars are finite
    val = model.get_val_loss(data.point_cloud, data.points, data.values)
    assert len(val) == 3 and torch.isfinite(val[0]) and torch.isfinite(val[1])
    cfg.loss_type = "occupancy"
    occ = shapemol_amd.collate_fn([{"mesh": mesh}, {"mesh": mesh}], cfg, device=DEV, seed=5)
    assert torch.equal(occ.point_cloud, data.point_cloud) and torch.equal(occ.points, data.points)
    assert torch.equal(occ.values, (data.values > 0).float()) and 0 < int(occ.values.sum()) <= 2 * 32
    val = _ae("occupancy").get_val_loss(occ.point_cloud, occ.points, occ.values)
    assert len(val) == 3 and all(torch.isfinite(x) for x in val)
    cpu = data.to("cpu")
    assert cpu.points.device.type == "cpu" and cpu.values.device.type == "cpu"


def test_shape_emb_from_meshes():
    import shapemol_amd
    from util import hip_model, synth
    meshes = [S.u_mesh(), S.tile_mesh(512), S.u_mesh()]
    model = _ae()
    zs, bounds, clouds, centres = shapemol_amd.get_pointAE_shape_emb(meshes, model, 512, batch_size=2, seed=9)
    assert zs.shape == (3, 32, 3) and bounds.shape == (3, 3, 2) and clouds.shape == (3, 1, 512, 3) and centres.shape == (3, 3)
    assert all(t.is_cuda and t.dtype == torch.float32 for t in (zs, bounds, clouds, centres))
    assert torch.equal(zs, model.encoder(clouds))                                  # bit for bit
    zs2 = shapemol_amd.get_pointAE_shape_emb(meshes, model.encoder, 512, batch_size=2, seed=9)[0]
    assert torch.equal(zs, zs2)
    for b, (v, _) in enumerate(meshes):
        c = centres[b].cpu().numpy().astype(np.float64)
        want = np.stack([v.min(0) - c, v.max(0) - c], 1)
        assert np.abs(bounds[b].cpu().numpy() - want).max() <= np.spacing(np.float32(np.abs(want).max()))
        assert (bounds[b, :, 0] < bounds[b, :, 1]).all()
    # sample_diffusion's box check takes the (B,3,2) tensor (its bounds[0] clamps the atoms)
    m = hip_model(cond_mask_prob=0.1)
    bb = synth.synthetic_batch(3, seed=3)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    args = (T(bb["init_pos"]), T(bb["init_v"]), T(bb["batch"]), T(bb["shape"]).view(3, -1))
    kw = dict(num_steps=2, center_pos_mode="none", guide_stren=0.5, threshold_type="reference_threshold", seed=1)
    r = m.sample_diffusion(*args, **kw, bounds=bounds)
    assert torch.isfinite(r["pos"]).all()
    with pytest.raises(ValueError):
        m.sample_diffusion(*args, **kw, bounds=bounds.transpose(1, 2))          # the check is live: a (B,2,3) box is refused
