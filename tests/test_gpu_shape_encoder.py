"""The device shape encoder (shapemol_se_*, csrc/sm_shape.h) stage by stage: every kNN read back and checked as a kNN, every stage
recomposed in float64 from the device's own input to it (tests/shape_encoder_f64.py), at the shapes and configurations where the
kernels take another path, plus the tie rule, batch composition, context reuse and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import shape_encoder_f64 as S
from util import golden, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# clouds for which the 20th-to-21st neighbour gap is at least 4 slacks in every row of every kNN of the float64 evaluation with
# layer_num 4, latent_dim 32 (found on the CPU; the tests assert it): the float32 kNN then chooses the float64 sets.  (1, 32) and
# (3, 32) are plain seeded clouds; no seeded batch of five independent 48-point clouds has such a margin (none of 18000 tried,
# one single cloud in a hundred), so (5, 48) is the seeded cloud 213 and four random rotations of it (S.rotated_copies).
SAFE_SEED = {(1, 32): 3, (5, 48): 213, (3, 32): 42}


@functools.lru_cache(maxsize=None)
def _encoder(L, LAT):
    import shapemol_amd
    enc = shapemol_amd.VN_DGCNN_Encoder(128, LAT, L, S.K)
    missing, unexpected = enc.load_state_dict(S.state_dict(L, LAT), strict=False)
    assert not unexpected and all(k.endswith(("running_mean", "running_var", "num_batches_tracked")) for k in missing)
    return enc.to(DEV)


def _n_max():
    return _encoder(2, 32).max_points(DEV)


def _buffers(enc, pts):
    """(stops, final) of shape_encoder_f64.all_gates from the device: one encode per stop, all buffers of a stop from one run."""
    x = pts.to(DEV)
    P = x.shape[0] * x.shape[1]
    stops = []
    try:
        for l in range(enc.layer_num + 1):
            enc.debug_stop_after(DEV, l)
            enc(x)
            stops.append({n: torch.from_numpy(enc.debug_read(DEV, n, P)) for n in ("idx", "h0", "hcat") + (("y", "xx") if l else ())})
    finally:
        enc.debug_stop_after(DEV, -1)
    out = enc(x).cpu()
    return stops, dict(hcat=torch.from_numpy(enc.debug_read(DEV, "hcat", P)), pd=torch.from_numpy(enc.debug_read(DEV, "pd", P)), out=out)


def _points(B, N):
    return torch.from_numpy(golden("shape_encoder.npz")["points"]) if (B, N) == (3, 512) else S.clouds(B, N, 1000 + N)


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "-".join("Nmax" if v is None else str(v) for v in s))
def test_stage_gates_and_knn_validity(shape):
    """(B, N, layer_num, latent_dim): the minimum N; 3 column tiles for 4 waves and P = 240, no multiple of 16; the fixture's clouds;
    both upper ends of layer_num and latent_dim; the full LDS row (value gates of the edge stages on 1024 evenly spread rows there,
    every other check on all rows)."""
    B, N, L, LAT = shape
    N = N or _n_max()
    enc, sd, pts = _encoder(L, LAT), S.state_dict(L, LAT), _points(B, N)
    stops, final = _buffers(enc, pts)
    problems, gates = S.all_gates(sd, pts, L, stops, final)
    for k, (eh, e32, ok) in gates.items():
        print(f"{shape} {k}: eH {eh:.3e} e32 {e32:.3e} bound {4 * e32 + 16 * S.U:.3e} {'ok' if ok else 'FAIL'}")
    record("shape_encoder_stage_gates", shape=[B, N, L, LAT], problems=len(problems), **{k: v[0] for k, v in gates.items()})
    assert not problems, problems[:5]
    assert all(v[2] for v in gates.values()), {k: v for k, v in gates.items() if not v[2]}


def test_knn_tie_rule():
    """Every point twice: the two smallest d2 of each row are exactly 0, so both copies come first, lower index first, and the rows
    of the two copies are the same.  Only the conv_pos neighbour list is read: no latent is asserted for such a cloud."""
    enc = _encoder(4, 32)
    a = S.clouds(1, 32, 77)
    pts = torch.cat([a, a], 1)
    try:
        enc.debug_stop_after(DEV, 0)
        enc(pts.to(DEV))
        idx = enc.debug_read(DEV, "idx", 64)
    finally:
        enc.debug_stop_after(DEV, -1)
    i = np.arange(64) % 32
    assert np.array_equal(idx[:, 0], i) and np.array_equal(idx[:, 1], i + 32)
    assert np.array_equal(np.sort(idx[:32], 1), np.sort(idx[32:], 1))
    assert not S.knn_problems(pts, torch.from_numpy(idx).reshape(1, 64, S.K))


def _safe(B, N, L=4):
    sd, pts = S.state_dict(L, 32), (S.rotated_copies if (B, N) == (5, 48) else S.clouds)(B, N, SAFE_SEED[(B, N)])
    f64 = S.forward(sd, pts, L, S.F64)
    assert S.least_margin(f64["feats"]) >= 4
    return sd, pts, f64


@pytest.mark.parametrize("shape", ((1, 32), (5, 48)))
def test_end_to_end_against_the_cpu_oracle(shape):
    from oracle import shape_encoder_oracle as SE
    sd, pts, _ = _safe(*shape)
    z = _encoder(4, 32)(pts.to(DEV)).cpu()
    err = float((z - SE.encode(sd, pts, 4, S.K)).abs().max())
    record("shape_encoder_oracle_small", shape=list(shape), max_err=err)
    assert err < 2e-5


def _close(a, b, e32, what):
    """Two correct float32 evaluations of one input: within 4 e32 + 16 u of each other, relative to the largest entry."""
    a, b = S.T(a, S.F64), S.T(b, S.F64)
    d = float((a - b).abs().max() / b.abs().max())
    record("shape_encoder_" + what, diff=d, bound=4 * e32 + 16 * S.U)
    assert d <= 4 * e32 + 16 * S.U, (what, d, e32)


def test_batch_composition_permutation():
    """Batch-norm pools the batch: permuting the shapes of a batch permutes the latents (the double atomics are order-dependent, so
    to float32 accuracy, not bit for bit), and a shape encoded alone gets another latent."""
    sd, pts, _ = _safe(3, 32)
    enc = _encoder(4, 32)
    e32, z64 = S.f32_latent_error(sd, pts, 4)
    z = enc(pts.to(DEV)).cpu()
    _close(z, z64, e32, "batch3")
    perm = [2, 0, 1]
    _close(enc(pts[perm].to(DEV)).cpu(), z[perm], e32, "permuted")
    alone = enc(pts[:1].to(DEV)).cpu()
    assert float((alone - z[:1]).abs().max() / z.abs().max()) > 1e-3


def test_rotation_rotates_every_stage():
    """Vector neurons: rotating the cloud rotates h0, every block's output, the conv_c products and the latent.  The allowance is
    four times what the float32 CPU evaluation itself misses equivariance by, plus 16 u."""
    sd, pts, _ = _safe(1, 32)
    ang = torch.tensor([0.3, -1.1, 2.0], dtype=S.F64)
    Q = torch.linalg.matrix_exp(torch.tensor([[0, -ang[2], ang[1]], [ang[2], 0, -ang[0]], [-ang[1], ang[0], 0]], dtype=S.F64))
    rot = (pts.double() @ Q.t()).float()
    assert S.least_margin(S.forward(sd, rot, 4, S.F64)["feats"]) >= 4
    enc = _encoder(4, 32)

    def run(x):
        z = enc(x.to(DEV)).cpu()
        return dict(h0=enc.debug_read(DEV, "h0", 32), hcat=enc.debug_read(DEV, "hcat", 32), pd=enc.debug_read(DEV, "pd", 32), out=z)

    def cpu(x):
        f = S.forward(sd, x, 4)
        return dict(h0=f["stops"][0]["h0"], **f["final"])
    (d0, d1), (c0, c1) = (run(pts), run(rot)), (cpu(pts), cpu(rot))
    for k in ("h0", "hcat", "pd", "out"):
        miss = lambda a, b: float((S.T(a, S.F64) @ Q.t() - S.T(b, S.F64)).abs().max() / S.T(b, S.F64).abs().max())      # noqa: E731
        e32, eh = miss(c0[k], c1[k]), miss(d0[k], d1[k])
        record("shape_encoder_rotation", tensor=k, eH=eh, e32=e32)
        assert eh <= 4 * e32 + 16 * S.U, (k, eh, e32)


def test_one_context_many_sizes_on_a_side_stream():
    """N = 512, N = 32, B = 4 at N = 512 (the workspace regrows), N = 32 again, all on one context and a non-default stream: each
    latent is a fresh context's, and encoding twice gives the same."""
    import shapemol_amd
    sd = S.state_dict(4, 32)
    fx = torch.from_numpy(golden("shape_encoder.npz")["points"])
    small = S.clouds(1, 32, SAFE_SEED[(1, 32)])
    inputs = [fx[:1], small, torch.cat([fx, fx[:1].flip(1) * 0.9]), small]

    def fresh():
        enc = shapemol_amd.VN_DGCNN_Encoder(128, 32, 4, S.K)
        enc.load_state_dict(sd, strict=False)
        return enc.to(DEV)
    # the float32 evaluation's own error, measured on the CPU for the one-cloud inputs; the batch of four 512-point clouds of the
    # same fixture takes the single fixture cloud's (its float64 evaluation alone would take ten seconds)
    e32 = {id(x): S.f32_latent_error(sd, x, 4)[0] for x in inputs[:2]}
    e32[id(inputs[2])] = e32[id(inputs[0])]
    one, stream = fresh(), torch.cuda.Stream(DEV)
    with torch.cuda.stream(stream):
        got = [(one(x.to(DEV)), one(x.to(DEV))) for x in inputs]
    stream.synchronize()
    for n, (x, (z1, z2)) in enumerate(zip(inputs, got)):
        _close(z1.cpu(), fresh()(x.to(DEV)).cpu(), e32[id(x)], f"reuse{n}")
        _close(z2.cpu(), z1.cpu(), e32[id(x)], f"twice{n}")


def test_refusals_return_before_any_launch():
    """Every refusal carries the library's own message, the N limit is named, and the context still encodes afterwards."""
    from shapemol_amd import _lib
    lib = _lib.load()
    enc = _encoder(4, 32)
    pts = S.clouds(1, 32, SAFE_SEED[(1, 32)])
    before = enc(pts.to(DEV)).cpu()
    ctx, n_max = enc._context(torch.device(DEV)), enc.max_points(DEV)
    assert n_max % 16 == 0 and n_max >= 512
    x = torch.zeros((1, n_max + 16, 3), device=DEV)
    out = torch.zeros((1, 32, 3), device=DEV)
    px, po = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())

    def refused(rc, *words):
        assert rc != 0
        msg = lib.shapemol_last_error().decode()
        assert all(w in msg for w in words), msg

    for B, N in ((1, 16), (1, 40), (1, n_max + 16), (0, 32), (65536, 32)):
        refused(lib.shapemol_se_encode(ctx, px, B, N, po, None), "shapemol_se_encode: need", f"[32, {n_max}]", f"N = {N}")
    refused(lib.shapemol_se_encode(ctx, None, 1, 32, po, None), "shapemol_se_encode: null argument")
    refused(lib.shapemol_se_encode(ctx, px, 1, 32, None, None), "shapemol_se_encode: null argument")
    refused(lib.shapemol_se_encode(None, px, 1, 32, po, None), "shapemol_se_encode: null argument")
    with pytest.raises(_lib.ShapeMolLibraryError, match=rf"\[32, {n_max}\]"):
        enc(x)
    with pytest.raises(RuntimeError, match="HIP device"):
        enc(pts)
    # creation
    w = enc._pack()
    pw, new = w.ctypes.data_as(C.c_void_p), C.c_void_p()
    count = lambda lat=32, L=4: lib.shapemol_se_weight_count(128, lat, L)      # noqa: E731
    refused(lib.shapemol_se_create(64, 32, 4, 20, pw, w.size, 0, C.byref(new)), "hidden_dim must be 128")
    refused(lib.shapemol_se_create(128, 32, 4, 16, pw, w.size, 0, C.byref(new)), "num_k must be 20")
    for lat, L in ((32, 0), (32, 9), (0, 4), (257, 4)):
        refused(lib.shapemol_se_create(128, lat, L, 20, pw, count(lat, L), 0, C.byref(new)), "latent_dim / layer_num out of range")
    refused(lib.shapemol_se_create(128, 32, 4, 20, pw, w.size - 1, 0, C.byref(new)), "weight count mismatch")
    refused(lib.shapemol_se_create(128, 32, 4, 20, None, w.size, 0, C.byref(new)), "null argument")
    refused(lib.shapemol_se_create(128, 32, 4, 20, pw, w.size, 0, None), "null argument")
    assert new.value is None
    # the read-back
    buf = np.empty(32 * S.K, np.int32)
    refused(lib.shapemol_se_debug_read(ctx, 6, buf.ctypes.data_as(C.c_void_p), buf.nbytes), "what must be one of")
    refused(lib.shapemol_se_debug_read(ctx, 0, buf.ctypes.data_as(C.c_void_p), buf.nbytes - 4), "n_bytes is")
    refused(lib.shapemol_se_debug_read(ctx, 0, None, buf.nbytes), "null argument")
    refused(lib.shapemol_se_debug_stop_after(ctx, 5), "n_blocks must be")
    assert torch.equal(out.cpu(), torch.zeros(1, 32, 3))
    e32, _ = S.f32_latent_error(S.state_dict(4, 32), pts, 4)
    _close(enc(pts.to(DEV)).cpu(), before, e32, "after_refusals")
