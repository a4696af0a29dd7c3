"""The shape-data builder without a GPU: self-checks of its oracle (tests/shape_data_oracle.py) on the meshes and draws the GPU
tests use, the argument checks of the public surface (the library's host check touches no device), and what the host uploads
(areas' running sum, projected bounds, bounding boxes; the projected faces and their boxes are built on the device) from a
stand-alone program, built plain and with the address and undefined-behaviour sanitizers (host code only)."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mesh_oracle as M  # noqa: E402
import shape_data_oracle as S  # noqa: E402
from util import ROOT  # noqa: E402

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("name", ["umesh", "tetra"])
def test_oracle_cloud_points_lie_on_their_faces(name):
    v, f = S.named_mesh(name)
    tab = S.host_tables(v, f)
    assert M.check_closed(f)
    c32, k, p, w = S.surface_cloud(tab, S.draws((512, 3), 5))
    assert (w >= 0.0).all() and (w <= 1.0).all()
    assert np.abs(w.sum(1) - 1.0).max() <= 4 * EPS
    A, B, C = tab["A"][k], tab["B"][k], tab["C"][k]
    n = np.cross(B - A, C - A)
    scale = np.abs(v).max()
    plane = np.abs(np.einsum("ij,ij->i", p - A, n)) / np.linalg.norm(n, axis=1)
    assert plane.max() <= 16 * EPS * scale                        # a sum of three products of magnitude <= scale
    assert np.abs(c32.astype(np.float64) - p).max() <= np.spacing(np.float32(scale)) / 2
    # the face follows the cdf rule, and the areas weight it: faces of zero area are never chosen
    x = S.draws((512, 3), 5)[:, 0] * tab["cdf"][-1]
    assert (tab["cdf"][k] > x).all() and ((k == 0) | (tab["cdf"][np.maximum(k - 1, 0)] <= x)).all()
    assert (tab["area"][k] > 0).all()


@pytest.mark.parametrize("name", sorted(S.FED_CASES))
def test_oracle_selection_and_containment(name):
    """On every fed-draw case of the GPU suite: the selected rows are the first n_in inside / n_out outside candidates in
    candidate order; ray parity agrees with the winding number outside its margin, and at most 2 % of the candidates lie within."""
    meshes, P, T, loss, cd, qd, res = S.fed_case(name)
    for (v, f), r in zip(meshes, res):
        assert not r["short"]
        flags, sel, n_in = r["flags"], r["sel"], r["n_in"]
        assert len(sel) == T and n_in == min(T // 2, int(flags.sum())) and r["n_out"] == T - n_in
        assert flags[sel[:n_in]].all() and not flags[sel[n_in:]].any()
        assert (np.diff(sel[:n_in]) > 0).all() and (np.diff(sel[n_in:]) > 0).all()
        if n_in:
            assert int(flags[:sel[n_in - 1] + 1].sum()) == n_in            # no inside candidate skipped
        assert int((~flags[:sel[-1] + 1]).sum()) == T - n_in               # no outside candidate skipped
        if T >= 100:
            skipped, agree = S.winding_check(v, f, r["cand"], flags)
            assert agree and skipped <= S.WINDING_SKIP_CAP, (skipped, agree)
        if loss == "occupancy":
            assert set(np.unique(r["values"])) <= {0.0, 1.0}
        else:
            assert (r["values"][:n_in] >= 0).all() and (r["values"][n_in:] <= 0).all()
    if name == "tetra":
        assert 0 < res[0]["n_in"] < T // 2
    if name.startswith("tile"):
        assert len(meshes[0][1]) == int(name[4:7])
    if name == "batch3_twice":
        assert np.array_equal(res[0]["points"], res[2]["points"]) and np.array_equal(res[0]["values"], res[2]["values"])


def test_tile_meshes_straddle_the_face_tile():
    counts = sorted(len(S.tile_mesh(n)[1]) for n in S.TILE_PARAMS)
    assert counts == [508, 512, 520] and counts[0] < 512 < counts[2]       # kMeshFaceTile = 512
    for n in S.TILE_PARAMS:
        assert M.check_closed(S.tile_mesh(n)[1])


def test_cube_is_short_of_outside_candidates():
    """The 40 A cube of the GPU error-path test: (40 / 42)^3 = 0.86 of the candidates fall inside, too few remain outside."""
    meshes, P, T, cd, qd = S.short_case()
    v, f = meshes[1]
    assert M.check_closed(f)
    r = S.build(v, f, cd[1], qd[1], T)
    assert r["short"] and r["n_in"] == T // 2 and r["counts"][1] < T - r["n_in"]
    assert not S.build(*meshes[0], cd[0], qd[0], T)["short"]


def test_pillbox_face_holds_half_the_area():
    v, f = S.pillbox()
    assert M.check_closed(f)
    area = S.host_tables(v, f)["area"]
    assert abs(area[0] / area.sum() - 0.5) < 1e-9


# ---- the public surface's argument checks (no device is touched before they pass) ---------------------------------------------
def _cfg(**kw):
    c = dict(shape_type="point_cloud", point_cloud_samples=16, num_samples=8, loss_type="signed_distance")
    c.update(kw)
    return c


def test_bad_arguments_raise_value_error():
    from shapemol_amd.shape_data import ShapeData, build_batch, collate_fn
    v, f = S.tetrahedron()
    good = [{"mesh": (v, f)}]
    bad_face, neg_face, nan_vert = f.copy(), f.copy(), v.copy()
    bad_face[2, 1] = 4
    neg_face[0, 0] = -1
    nan_vert[1, 2] = np.nan
    inf_vert = v.copy()
    inf_vert[0, 0] = np.inf
    cases = [
        ([{"mesh": (v, bad_face)}], _cfg(), "face"),
        ([{"mesh": (v, neg_face)}], _cfg(), "face"),
        ([{"mesh": (nan_vert, f)}], _cfg(), "finite"),
        ([{"mesh": (inf_vert, f)}], _cfg(), "finite"),
        ([{"mesh": (v, f[:0])}], _cfg(), "at least 1 face"),
        (good, _cfg(point_cloud_samples=0), "point_cloud_samples"),
        (good, _cfg(point_cloud_samples=2049), "2048"),
        (good, _cfg(num_samples=1), "num_samples"),
        (good, _cfg(num_samples=0), "num_samples"),
        (good, _cfg(loss_type="chamfer"), "loss_type"),
        ([good[0], {"mesh": (v, bad_face)}], _cfg(), "shape 1"),
    ]
    for batch, cfg, word in cases:
        with pytest.raises(ValueError, match=word):
            ShapeData(batch, cfg, device="cuda:0")
    with pytest.raises(ValueError, match="num_samples"):
        build_batch([(v, f)], 16, 1, device="cuda:0")
    with pytest.raises(NotImplementedError):
        ShapeData(good, _cfg(shape_type="voxel"), device="cuda:0")
    with pytest.raises(NotImplementedError):
        collate_fn(good, type("Cfg", (), _cfg(shape_type="voxel")), device="cuda:0")
    import shapemol_amd
    assert shapemol_amd.ShapeData is ShapeData and shapemol_amd.get_pointAE_shape_emb is not None


# ---- the host image ----------------------------------------------------------------------------------------------------------
def _compile(tmp, name, extra):
    hipcc = shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    exe = str(tmp / name)
    r = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", *extra, "-o", exe,
                        os.path.join(ROOT, "tests", "shape_data_probe.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.fixture(scope="module")
def probes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("shape_data_probe")
    return tmp, [_compile(tmp, "plain", []),
                 _compile(tmp, "sanitized", ["-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def _write(path, meshes):
    vo = np.cumsum([0] + [len(v) for v, _ in meshes]).astype(np.int64)
    fo = np.cumsum([0] + [len(f) for _, f in meshes]).astype(np.int64)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<q", len(meshes)))
        fh.write(vo.tobytes() + fo.tobytes())
        fh.write(np.concatenate([np.asarray(v, np.float64).reshape(-1, 3) for v, _ in meshes]).tobytes())
        fh.write(np.concatenate([np.asarray(f, np.int32).reshape(-1, 3) for _, f in meshes]).tobytes())


def _run(exe, path, P=16, T=8, loss=0):
    return subprocess.run([exe, path, str(P), str(T), str(loss)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))


def test_host_image_matches_numpy(probes):
    tmp, exes = probes
    meshes = [S.tetrahedron(), S.u_mesh(), S.tile_mesh(512), S.pillbox()]
    path = str(tmp / "batch.bin")
    _write(path, meshes)
    outs = []
    for exe in exes:
        r = _run(exe, path)
        assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    rows = {}
    for line in outs[0].splitlines():
        w = line.split()
        rows.setdefault(w[0], []).append([float(x) for x in w[2:]])
    cdf = np.array(rows["cdf"])[:, 0]
    off, voff = np.array(rows["off"]).astype(int).T
    assert list(off) == list(np.cumsum([0] + [len(f) for _, f in meshes]))
    assert list(voff) == list(np.cumsum([0] + [len(v) for v, _ in meshes]))
    for b, (v, f) in enumerate(meshes):
        tab, mt = S.host_tables(v, f), M.MeshTables(v, f)
        sl = slice(off[b], off[b + 1])
        assert np.array_equal(cdf[sl], tab["cdf"])                                   # the same operations in the same order
        assert np.array_equal(rows["lohi"][b], np.concatenate([tab["lo"], tab["hi"]]))
        assert np.array_equal(rows["pbounds"][b], np.array(mt.bounds))


def test_host_check_refuses(probes):
    tmp, exes = probes
    v, f = S.tetrahedron()
    bad = f.copy()
    bad[3, 0] = 9
    nanv = v.copy()
    nanv[0, 0] = np.nan
    path = str(tmp / "bad.bin")
    for meshes, args, word in (([(v, bad)], {}, "face 3"), ([(nanv, f)], {}, "not finite"), ([(v, f[:0])], {}, "at least 1 face"),
                               ([(v, f)], dict(P=0), "point_cloud_samples"), ([(v, f)], dict(P=2049), "2048"), ([(v, f)], dict(T=1), "num_samples"),
                               ([(v, f)], dict(loss=2), "loss_type")):
        _write(path, meshes)
        for exe in exes:
            r = _run(exe, path, **args)
            assert r.returncode == 1 and r.stderr == "" and r.stdout.startswith("error ") and word in r.stdout, r.stdout + r.stderr
