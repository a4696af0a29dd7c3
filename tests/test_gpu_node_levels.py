"""The exact-mode node stage in two dependency levels (option node_levels = 1: node_out6_kernel, then node_after6_kernel with
the follow-up MLPs and the per-node products side by side) against node_chain6_kernel + node_linear6_kernel (node_levels = 0)
on the same context and inputs.  Every output element keeps its MFMA accumulation order, so everything must agree to the bit:
h', the queries q_h and q_x, the atom-type head and the per-node products, and with them the evaluation's three outputs.
Both forms call the same device functions (Team6 and node_out6_pair in csrc/sm_node.h), so this file no longer compares two
independent statements of the arithmetic, only two schedules and LDS layouts of one; that the arithmetic itself is the
reference's is what test_gpu_parity.py::test_forward_alternative_kernels_golden holds both forms to.
Shapes are the ones where the new indexing can go wrong: a single partial tile, a full tile, odd tile counts (the last pair of
column tiles has one tile), a pair plus one; H = 128 (8 waves per follow-up job) and the reduced H = 32 model (2 waves), in workgroups of 16:
the other waves leave before the first barrier; molecules of mixed sizes inside a tile.
Run on the GPU box:  pytest tests/test_gpu_node_levels.py -m gpu"""
import numpy as np
import pytest
import torch

import chain_forms as CF
from util import T, hip_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 15, 16, 17, 31, 32, 33, 49)
MODELS = {128: dict(num_layers=2), 32: dict(hidden_dim=32, n_heads=4, num_layers=2)}
REC = ("levels", "follow_jobs", "linear_jobs", "waves", "order", "tiles_per_job", "chunk", "lds_bytes")
OPTION_DEFAULTS = {"node_levels": 1, "after_order": 2, "after_waves": 16, "stop_layer": -1}


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
    """One evaluation: its three outputs and the node stage's buffers left behind, plus the node-stage launch record."""
    for k, v in options.items():
        m.set_option(k, v)
    bb = CF.batch(_counts(n), seed=11)
    b = len(bb["counts"])
    t = (np.arange(b, dtype=np.int64) * 377 + 123) % 1000
    with torch.no_grad():
        out = m(T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV), T(t, DEV))
    got = {k: out[k].cpu().numpy() for k in ("pred_ligand_pos", "pred_ligand_h", "pred_ligand_v")}
    got["q_h"] = m.debug_read("q", (n, h), np.float32)            # h2x queries of the last layer run
    got["q_x"] = m.debug_read("q_x", (n, h), np.float32)          # x2h queries for layer 1 (layer 0's second follow-up), or the prologue's
    got["pre"] = m.debug_read("pre", (n, 8 * h), np.float32)      # per-node products: [:, :4H] of the last layer run, [:, 4H:] of layer 0
    rec = dict(zip(REC, (int(x) for x in m.debug_read("launch_node", (8,), np.int64))))
    return got, rec


def _assert_equal(a, b):
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (k, float(np.abs(a[k] - b[k]).max()))


@pytest.mark.parametrize("h", list(MODELS))
@pytest.mark.parametrize("n", SIZES)
def test_two_levels_equal_chain_and_linear(n, h):
    """Two layers: layer 0 with two follow-up MLPs and 8 H / 16 product tiles, the last with the atom-type head (15 classes:
    the scalar-store tail) and 4 H / 16 tiles."""
    m = hip_model(**MODELS[h])
    new, rec1 = _run(m, n, h, node_levels=1)
    old, rec0 = _run(m, n, h, node_levels=0)
    print(n, h, rec1)
    assert rec1["levels"] == 1 and rec0["levels"] == 0
    _assert_equal(new, old)


@pytest.mark.parametrize("h", list(MODELS))
def test_stop_layer_one(h):
    """stop_layer = 1: layer 0 is the last one run (q_h2x and the head; 4 H / 16 tiles; h' redirected to the caller's buffer)."""
    m = hip_model(**MODELS[h])
    new, _ = _run(m, 33, h, node_levels=1, stop_layer=1)
    old, _ = _run(m, 33, h, node_levels=0, stop_layer=1)
    for got in (new, old):
        got["pre"] = got["pre"][:, :4 * h]          # (the other half is not written by a one-layer evaluation)
    _assert_equal(new, old)


@pytest.mark.parametrize("order,waves", [(0, 8), (1, 8), (2, 8), (0, 16), (1, 16)])
@pytest.mark.parametrize("h", list(MODELS))
def test_job_orders_and_workgroup_sizes(h, order, waves):
    """The other grid orders and the 8-wave workgroup (two per CU) compute the same bits as the default (linear jobs first,
    16 waves)."""
    m = hip_model(**MODELS[h])
    old, _ = _run(m, 49, h, node_levels=0)
    new, rec = _run(m, 49, h, node_levels=1, after_order=order, after_waves=waves)
    assert (rec["levels"], rec["order"], rec["waves"]) == (1, order, max(waves, h // 16))
    _assert_equal(new, old)


def test_two_level_form_is_the_one_launched():
    """The launch record of the node stage: the default runs the two-level form with one follow-up job per (MLP, pair of
    column tiles) -- the last layer has two MLPs (q_h2x and the head) --, linear jobs first, in 16-wave workgroups of which a
    follow-up job uses H / 16."""
    for h in MODELS:
        m = hip_model(**MODELS[h])
        _, rec = _run(m, 49, h)
        n_ct = CF.ceil_div(49, 16)
        assert rec["levels"] == 1 and rec["follow_jobs"] == 2 * CF.ceil_div(n_ct, 2), rec
        assert (rec["waves"], rec["order"]) == (16, 2) and rec["linear_jobs"] >= CF.ceil_div(4 * (h // 16), 16), rec
        assert rec["chunk"] * 3 * h * 32 <= rec["lds_bytes"], rec
