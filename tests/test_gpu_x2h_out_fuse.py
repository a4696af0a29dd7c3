"""The node output MLP in the tail of the streaming x2h kernel (option x2h_out_fuse = 1: stream_node_out_epilogue computes
h' = h + MLP_out([att | h]) for the workgroup's own atoms, node_out6_kernel is not launched) against the separate launch
(x2h_out_fuse = 0) on the same context and inputs.  The tail runs node_out6_kernel's own body on the same team layout, so a
column's arithmetic is the same whichever tile the atom lands in: h', the attention rows, the queries, the per-node products and
the evaluation's three outputs must agree to the bit.
The streaming kernels' tiles per workgroup are forced (option stream_chunk) instead of growing N.  Shapes: a half-used tile
(N = 1, 2, 3); two atoms per workgroup (chunk 1, N = 17 and 33: many workgroups, an odd last one); 16 and 18 atoms per workgroup
(chunk 8 and 9 at k = 8: one full column tile, then a second with two columns); chunk 11 (the benchmark's 22 atoms) with a short
last workgroup; k = 12 (KP = 16, one atom per tile) with 16 and 17 atoms; H = 128 and H = 32; molecules of 5, 3, 9, 2, 7 atoms, so
that every workgroup of more than a few atoms spans several molecules.  Not fused: x2h_out_fuse = 0, k > 16 (half-atom tiles),
and more than 96 atoms per workgroup (the host's boundary: three passes of the tail over 32 atoms each, the most that was
measured); x2h_out_fuse = 2 lifts the boundary.
Run on the GPU box:  pytest tests/test_gpu_x2h_out_fuse.py -m gpu"""
import numpy as np
import pytest
import torch

import chain_forms as CF
from util import T, hip_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODELS = {128: dict(num_layers=2), 32: dict(hidden_dim=32, n_heads=4, num_layers=2)}
REC = ("fused", "atoms_per_wg", "col_tiles_per_wg", "lds_bytes")
OPTION_DEFAULTS = {"x2h_out_fuse": 1, "stream_chunk": 0, "stop_layer": -1}
BOUNDARY = 96       # atoms per workgroup up to which the fused form is used (3 * CHAIN_COLS * 16: step_forms, csrc/sm_launch.h)
# (k, N, forced chunk): atoms per workgroup = chunk * 16 / KP
CASES = [(8, 1, 0), (8, 2, 0), (8, 3, 0), (8, 17, 1), (8, 33, 1), (8, 37, 8), (8, 37, 9), (8, 49, 11), (8, 44, 11), (8, 45, 16),
         (12, 35, 16), (12, 35, 17), (12, 3, 0)]


@pytest.fixture(autouse=True)
def _restore_options():
    """Every test leaves the cached models on the library defaults."""
    yield
    import util
    for key, m in list(util._cache.items()):
        if key[0] != "h":
            continue
        opts = m.__dict__.get("_options", {})
        for k, v in OPTION_DEFAULTS.items():
            if k in opts and opts[k] != v:
                m.set_option(k, v)


def _counts(n):
    """Molecule sizes 5, 3, 9, 2, 7, ... that sum to n: several molecules inside every 16-atom tile."""
    out, i = [], 0
    while sum(out) < n:
        out.append(min((5, 3, 9, 2, 7)[i % 5], n - sum(out)))
        i += 1
    return np.asarray(out, np.int64)


def _run(m, n, h, **options):
    """One evaluation: its three outputs and the buffers the layers left behind, plus the x2h tail's launch record."""
    for k, v in options.items():
        m.set_option(k, v)
    bb = CF.batch(_counts(n), seed=11)
    b = len(bb["counts"])
    t = (np.arange(b, dtype=np.int64) * 377 + 123) % 1000
    with torch.no_grad():
        out = m(T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV), T(t, DEV))
    got = {k: out[k].cpu().numpy() for k in ("pred_ligand_pos", "pred_ligand_h", "pred_ligand_v")}
    got["att"] = m.debug_read("att", (n, h), np.float32)          # x2h attention rows of the last layer run
    got["q_h"] = m.debug_read("q", (n, h), np.float32)
    got["q_x"] = m.debug_read("q_x", (n, h), np.float32)
    got["pre"] = m.debug_read("pre", (n, 8 * h), np.float32)      # per-node products (preAB)
    rec = dict(zip(REC, (int(x) for x in m.debug_read("launch_x2h_out", (4,), np.int64))))
    return got, rec


def _assert_equal(a, b):
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (k, float(np.abs(a[k] - b[k]).max()))


def _compare(m, n, h, kp, chunk, fuse=1, **options):
    new, rec1 = _run(m, n, h, x2h_out_fuse=fuse, stream_chunk=chunk, **options)
    old, rec0 = _run(m, n, h, x2h_out_fuse=0, stream_chunk=chunk, **options)
    print(n, h, kp, chunk, rec1)
    assert rec1["fused"] == 1 and rec0["fused"] == 0, (rec1, rec0)
    assert rec1["atoms_per_wg"] == rec0["atoms_per_wg"] and rec1["col_tiles_per_wg"] == CF.ceil_div(rec1["atoms_per_wg"], 16)
    if chunk:
        assert rec1["atoms_per_wg"] == chunk * (16 // kp), rec1
    if options.get("stop_layer") == 1:
        for got in (new, old):
            got["pre"] = got["pre"][:, :4 * h]      # (the other half is not written by a one-layer evaluation)
    _assert_equal(new, old)


@pytest.mark.parametrize("h", list(MODELS))
@pytest.mark.parametrize("k,n,chunk", CASES)
def test_fused_tail_equals_node_out6(k, n, chunk, h):
    """All layers (two: the second x2h kernel also folds the first layer's coordinate update in chains; here a score
    evaluation) and stop_layer = 1 (h' redirected to the caller's buffer)."""
    m = hip_model(knn=k, **MODELS[h])
    _compare(m, n, h, CF.kp_of(k), chunk)
    _compare(m, n, h, CF.kp_of(k), chunk, stop_layer=1)


@pytest.mark.parametrize("h", list(MODELS))
@pytest.mark.parametrize("k,n,chunk,fuse", [(8, 85, 17, 1), (8, 85, 20, 1), (8, 140, 33, 1), (12, 70, 33, 1), (8, 205, 48, 1), (8, 205, 49, 2)])
def test_several_passes(k, n, chunk, fuse, h):
    """34, 40, 66 and 33 atoms per workgroup are walked 32 at a time (a second pass of 2, 8 and 1 atoms; a third of 2), with a
    short last workgroup; 96 atoms are three full passes, and x2h_out_fuse = 2 lifts the boundary: 98 atoms, a fourth pass of 2."""
    _compare(hip_model(knn=k, **MODELS[h]), n, h, CF.kp_of(k), chunk, fuse=fuse)


def test_not_fused_outside_its_conditions():
    """The record says 0 under x2h_out_fuse = 0 (every case above), with k > 16, and beyond the boundary of 96 atoms per
    workgroup; at the boundary it says 1.  The outputs of the unfused forms are the existing suite's business."""
    m = hip_model(knn=8, **MODELS[128])
    _, rec = _run(m, 205, 128, stream_chunk=BOUNDARY // 2)
    assert rec["fused"] == 1 and rec["atoms_per_wg"] == BOUNDARY, rec
    _, rec = _run(m, 205, 128, stream_chunk=BOUNDARY // 2 + 1)
    assert rec["fused"] == 0 and rec["atoms_per_wg"] == BOUNDARY + 2, rec
    _, rec = _run(m, 85, 128, stream_chunk=0, node_levels=0)
    m.set_option("node_levels", 1)
    assert rec["fused"] == 0, rec
    m12 = hip_model(knn=12, **MODELS[128])
    _, rec = _run(m12, 205, 128, stream_chunk=BOUNDARY + 1)
    assert rec["fused"] == 0 and rec["atoms_per_wg"] == BOUNDARY + 1, rec
    m32 = hip_model(knn=32, **MODELS[128])
    _, rec = _run(m32, 70, 128)
    assert rec["fused"] == 0 and rec["atoms_per_wg"] == 0, rec


def test_stream_chunk_zero_is_automatic():
    """stream_chunk = 0 leaves the launch geometry alone: the "launch" record's tiles per workgroup and grid are the host
    formula's, and a forced chunk shows up in it."""
    m = hip_model(knn=8, **MODELS[128])
    _run(m, 49, 128, stream_chunk=0)
    rec = [int(x) for x in m.debug_read("launch", (8,), np.int64)]
    assert (rec[5], rec[6]) == (CF.stream_chunk(49, 8, rec[7]), CF.stream_grid(49, 8, rec[7])), rec
    _run(m, 49, 128, stream_chunk=3)
    rec = [int(x) for x in m.debug_read("launch", (8,), np.int64)]
    assert (rec[5], rec[6]) == (3, CF.ceil_div(CF.stream_jobs(49, 8), 3)), rec
