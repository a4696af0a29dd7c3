#!/usr/bin/env python3
"""Times the shape-data builder (shapemol_amd/shape_data.py: surface clouds, query points and signed distances of a batch of
meshes on the device) at the shipped auto-encoder configuration, B = 32 meshes, P = 512 cloud points, T = 1024 query points,
on closed test meshes of its own -- subdivided icosahedra stretched to ellipsoids of 8-12 A, 1280 / 5120 / 20480 faces -- and,
in the same session, one forward + backward of PointCloud_AE.get_generator_train_loss at the same B, T: the step the batch feeds.

  builder_ms        host clock around ShapeData(...) (the call ends in a stream synchronise), warm, median of --reps; it
                    includes the host's part (packing, checks, the areas' running sum, projected bounds) and the upload
  train_step_ms     host clock around loss.backward() + device synchronise, warm, median of --reps
  oracle_ms         a numpy float64 restatement of the same stages IN THIS FILE (not tests/shape_data_oracle.py: ray parity with a
                    box prefilter and without the canonical edge rule, brute-force nearest cloud point), one process, on
                    --oracle-shapes meshes, scaled to B; the ratio is ORACLE-relative: the reference's trimesh / pytorch3d / sklearn path is not installed here and not measured
  kernels           per-kernel totals of a `rocprofv3 --kernel-trace --stats` run of this tool's --profile-pass (a child process
                    of its own, --profile-reps builds of the middle mesh size), copied to kernel_stats_<faces>.csv

    python tools/shape_data_bench.py [--out profiles/shape_data] [--reps 20] [--warmup 3] [--no-profile]
"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, P, T = 32, 512, 1024
ROT = np.array([[0.8, -0.6, 0.0], [0.36, 0.48, -0.8], [0.48, 0.64, 0.6]])      # csrc/sm_mesh.h kMeshRot


def icosphere(level):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, dtype=np.int32)


def meshes(level, n, seed):
    """n closed meshes: the icosphere stretched to ellipsoids with half-axes in 4..6 A, moved off the origin."""
    v, f = icosphere(level)
    rng = np.random.RandomState(seed)
    return [(v * rng.uniform(4.0, 6.0, 3) + rng.uniform(-20.0, 20.0, 3), f) for _ in range(n)]


# ---- the oracle's stages, restated (this tool imports nothing from tests/) ----------------------------------------------------
def oracle_build(verts, faces, cd, qd):
    faces = faces.astype(np.int64)
    A, Bv, C = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    cdf = np.add.accumulate(0.5 * np.linalg.norm(np.cross(Bv - A, C - A), axis=1))
    k = np.minimum(np.searchsorted(cdf, cd[:, 0] * cdf[-1], side="right"), len(cdf) - 1)
    s = np.sqrt(cd[:, 1])
    cloud = (((1 - s)[:, None] * A[k] + (s * (1 - cd[:, 2]))[:, None] * Bv[k]) + (s * cd[:, 2])[:, None] * C[k]).astype(np.float32)
    lo, hi = verts.min(0), verts.max(0)
    cand = ((qd * ((hi - lo) + 2.0)) + lo) - 1.0
    # ray parity along +w of the rotated frame, every candidate against the faces whose projected box holds it
    pu, pv, pw = (verts @ ROT.T).T
    qu, qv, qw = (cand @ ROT.T).T
    fu, fv, fw = pu[faces], pv[faces], pw[faces]
    inside = np.zeros(len(cand), dtype=bool)
    for c0 in range(0, len(cand), 256):
        sl = slice(c0, c0 + 256)
        u, w_, d = qu[sl, None], qv[sl, None], qw[sl]
        inbox = (u >= fu.min(1)) & (u <= fu.max(1)) & (w_ >= fv.min(1)) & (w_ <= fv.max(1))
        pi, fi = np.nonzero(inbox)
        e = [(fu[fi, (j + 1) % 3] - fu[fi, j]) * (qv[sl][pi] - fv[fi, j]) - (fv[fi, (j + 1) % 3] - fv[fi, j]) * (qu[sl][pi] - fu[fi, j]) for j in range(3)]
        same = ((e[0] >= 0) == (e[1] >= 0)) & ((e[1] >= 0) == (e[2] >= 0))
        depth = e[1] * (fw[fi, 0] - d[pi]) + e[2] * (fw[fi, 1] - d[pi]) + e[0] * (fw[fi, 2] - d[pi])
        cross = same & np.where(e[0] >= 0, depth > 0, depth < 0)
        inside[sl] = (np.bincount(pi, weights=cross, minlength=len(d)).astype(np.int64) & 1) == 1
    c64 = cloud.astype(np.float64)
    dist = np.sqrt(((cand[:, None, :] - c64[None]) ** 2).sum(-1).min(1))
    n_in = min(T // 2, int(inside.sum()))
    sel = np.concatenate([np.where(inside)[0][:n_in], np.where(~inside)[0][:T - n_in]])
    off = cloud.astype(np.float64).mean(0).astype(np.float32)
    return cloud - off, (cand[sel] - off).astype(np.float32), (np.where(np.arange(len(sel)) < n_in, 1.0, -1.0) * dist[sel]).astype(np.float32)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def profile_pass(level, reps):
    from shapemol_amd.shape_data import ShapeData
    cfg = dict(shape_type="point_cloud", point_cloud_samples=P, num_samples=T, loss_type="signed_distance")
    batch = [{"mesh": m} for m in meshes(level, B, 1)]
    for r in range(reps):
        ShapeData(batch, cfg, device="cuda:0", seed=r)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shape_data"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--oracle-shapes", type=int, default=2)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-pass", type=int, default=-1, help="(child of the rocprofv3 run) subdivision level to build")
    ap.add_argument("--profile-reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("shape_data_bench: no HIP device (a measurement without one would not be a measurement)")
    if a.profile_pass >= 0:
        return profile_pass(a.profile_pass, a.profile_reps)
    import shapemol_amd
    from shapemol_amd.shape_data import ShapeData
    os.makedirs(a.out, exist_ok=True)
    cfg = dict(shape_type="point_cloud", point_cloud_samples=P, num_samples=T, loss_type="signed_distance")
    res = {"device": torch.cuda.get_device_name(0), "B": B, "P": P, "T": T, "reps": a.reps, "warmup": a.warmup, "sizes": {}}

    torch.manual_seed(1)
    model = shapemol_amd.PointCloud_AE(dict(encoder="VN_DGCNN", hidden_dim=128, latent_dim=128, layer_num=4, num_k=20, point_dim=3,
                                            loss_type="signed_distance")).cuda()
    for level in (3, 4, 5):
        ms = meshes(level, B, 1)
        batch = [{"mesh": m} for m in ms]
        n_faces = len(ms[0][1])
        seeds = iter(range(10 ** 6))
        build = lambda: ShapeData(batch, cfg, device="cuda:0", seed=next(seeds))  # noqa: E731
        med, best, worst = timed(build, a.reps, a.warmup)
        data = build()
        z = model.encoder(data.point_cloud[:, None]).detach()

        def step():
            for q in model.generator.parameters():
                q.grad = None
            model.get_generator_train_loss(data.point_cloud, data.points, data.values, z_vector=z).backward()
        smed, sbest, sworst = timed(step, a.reps, a.warmup)

        def step_enc():
            for q in model.generator.parameters():
                q.grad = None
            model.get_generator_train_loss(data.point_cloud, data.points, data.values).backward()
        emed, ebest, eworst = timed(step_enc, a.reps, a.warmup)
        entry = {"faces": n_faces, "builder_ms": {"median": med, "min": best, "max": worst},
                 "train_step_ms": {"median": smed, "min": sbest, "max": sworst, "what": "get_generator_train_loss forward + backward, latent given"},
                 "train_step_with_encoder_ms": {"median": emed, "min": ebest, "max": eworst, "what": "the same with the frozen encoder's forward"},
                 "builder_over_train_step": med / smed, "inside_counts_min_max": [int(data.counts[:, 0].min()), int(data.counts[:, 0].max())]}
        if a.oracle_shapes > 0:
            rng = np.random.RandomState(2)
            t0 = time.perf_counter()
            for v, f in ms[:a.oracle_shapes]:
                oracle_build(v, f, rng.random_sample((P, 3)), rng.random_sample((3 * T, 3)))
            o_ms = (time.perf_counter() - t0) * 1e3 * B / a.oracle_shapes
            entry["oracle_ms"] = {"scaled_to_B": o_ms, "measured_shapes": a.oracle_shapes, "what": "this tool's numpy float64 restatement, one process (numpy's own threading), scaled linearly in the shapes"}
            entry["oracle_over_builder"] = o_ms / med
        res["sizes"][str(n_faces)] = entry
        print(json.dumps({str(n_faces): entry}), flush=True)

    if not a.no_profile:
        rp = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        for level in (4,):
            n_faces = 20 * 4 ** level
            d = os.path.join(a.out, f"rocprof_{n_faces}")
            shutil.rmtree(d, ignore_errors=True)
            r = subprocess.run([rp, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "sdata", "--", sys.executable,
                                os.path.abspath(__file__), "--profile-pass", str(level), "--profile-reps", str(a.profile_reps)],
                               capture_output=True, text=True, timeout=300)
            stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if r.returncode != 0 or not stats:
                res["profile_error"] = (r.stdout + r.stderr)[-2000:]
            else:
                shutil.copy(stats[0], os.path.join(a.out, f"kernel_stats_{n_faces}.csv"))
                res["kernel_stats"] = {"file": f"kernel_stats_{n_faces}.csv", "builds": a.profile_reps, "faces": n_faces}
            shutil.rmtree(d, ignore_errors=True)
    with open(os.path.join(a.out, "bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
