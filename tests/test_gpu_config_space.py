"""The score model at the edges of the configuration space shapemol_create accepts (tests/config_space.py; the buffer audit
and the measured errors are in profiles/config_space/README.md): k = 17 on half-atom tiles, the reduced model at k = 9 and 16 and at every limit it supports, one neighbour,
one shape point, shape-latent sizes other than 32 (the non-tiled shape-term kernel), the limits of S, SL, D and C, one layer.
Hidden width 32 with k > 16 is refused by shapemol_create, and that is tested.

Per case, batch and precision mode one forward against the CPU oracle on the same inputs.  `exact`: the float64 gate of
tests/precision.py unchanged (eH <= 4 e32 + 16 u per output; per-layer taps on the `full` batch).  `f16x2`: that mode's gate
FWD_TOL of tests/test_gpu_parity.py.  tests/test_config_space_cpu.py shows that the oracle moves by more than 100 gate bounds
when the last element of any dimension is dropped, so these gates can fail.  Run on the GPU box: pytest tests -m gpu -k config_space"""
import numpy as np
import pytest
import torch

import config_space as CS
import precision as P
from test_gpu_parity import FWD_TOL, MODE_IDS, POS_TOL, set_mode
from test_gpu_precision import hip_outputs
from util import T, hip_model, maxabs, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_IDS = list(CS.CASES)


@pytest.fixture(params=MODE_IDS)
def mode(request):
    return request.param


@pytest.fixture(autouse=True)
def _restore_modes():
    """Every test starts from the library defaults on every cached model, whatever the previous test selected."""
    yield
    import util
    from shapemol_amd.molopt_score_model import DEFAULT_OPTIONS
    for key, m in list(util._cache.items()):
        if key[0] != "h":
            continue
        opts = m.__dict__.get("_options", {})
        for k in ("feat_f16", "node_f16", "edge_bf16"):
            if k in opts and opts[k] != DEFAULT_OPTIONS[k]:
                m.set_option(k, DEFAULT_OPTIONS[k])


def hip(name, mode):
    return set_mode(hip_model(seed=CS.weight_seed(name), num_classes=CS.classes(name), **CS.overrides(name)), mode)


def forward3(m, bt, scale=1.0):
    """The three outputs of one forward as float64 ndarrays (positions scaled by `scale`)."""
    with torch.no_grad():
        out = m(T(bt["pos"] * np.float32(scale), DEV), T(bt["v"], DEV), T(bt["batch"], DEV), T(bt["shape"], DEV), T(bt["t"], DEV))
    m.check_status()
    return {k: out[k].double().cpu().numpy() for k in CS.OUTPUTS}


def check(name, which, mode, res, label):
    """Apply the mode's gate to `res` (the outputs of a forward on the case's batch), print and record the figures."""
    bt, r32, r64 = CS.refs(name, which)
    for k in CS.OUTPUTS:
        assert np.isfinite(res[k]).all(), (k, "not finite")
    if mode == "exact":
        g = P.gate(res, r32, r64)
        print(label, name, which, mode, {k: f"eH {v[0]:.2e} e32 {v[1]:.2e} x{v[2]:.2f}" for k, v in g.items()})
        record(label, config=name, batch=which, mode=mode, worst_over_bound=max(v[2] for v in g.values()),
               **{f"{k}_eH": v[0] for k, v in g.items()}, **{f"{k}_e32": v[1] for k, v in g.items()})
        bad = {k: f"eH {v[0]:.2e} > 4 e32 + 16u (e32 {v[1]:.2e}): {v[2]:.2f}x" for k, v in g.items() if v[2] > 1.0}
        assert not bad, bad
    else:
        errs = {k: maxabs(res[k], r32[k]) for k in CS.OUTPUTS}
        print(label, name, which, mode, errs)
        record(label, config=name, batch=which, mode=mode, **errs)
        assert max(errs.values()) < FWD_TOL, errs


def check_half_tiles(m, name, n_atoms, mode):
    """KP = 32: the launch records of the last forward show two half-atom tiles per atom and one combine per attention."""
    L, H = CS.overrides(name)["num_layers"], CS.overrides(name)["hidden_dim"]
    assert int(m.debug_read("dims", (8,), np.int64)[2]) == 32
    rec, erec = m.debug_read("launch", (8,), np.int64), m.debug_read("launch_edge", (4,), np.int64)
    assert list(erec) == [1, 2 * n_atoms, 2 * L, H], erec
    assert rec[2] == 0 and rec[3] == 0 and rec[4] == 0, rec          # no fold, no fused x2h + node launch: those are single-tile forms
    if mode == "exact":      # streaming kernels: whole rounds of two tiles over 2 N tiles
        chunk, grid = int(rec[5]), int(rec[6])
        assert chunk >= 2 and chunk % 2 == 0 and grid == (2 * n_atoms + chunk - 1) // chunk, rec
    else:
        assert rec[5] == 0 and rec[6] == 0, rec


@pytest.mark.parametrize("name", CASE_IDS)
def test_forward_full_batch(name, mode):
    """Every atom has k neighbours: the three outputs, in exact mode also h and dx after 1, 2 layers and e_w, within the mode's
    gate; the neighbour lists equal the oracle's and e_w is within 1e-6."""
    m = hip(name, mode)
    bt, r32, r64 = CS.refs(name, "full")
    res = hip_outputs(m, bt)
    assert np.array_equal(res["nbr"], r64["nbr"]), "HIP neighbour lists differ from the oracle's edge lists"
    assert np.abs(res["ew"] - r64["ew"]).max() < 1e-6
    check(name, "full", mode, res, "config_space_forward")
    if name in CS.KP32:
        check_half_tiles(m, name, len(bt["batch"]), mode)
    else:
        assert m.debug_read("launch_edge", (4,), np.int64)[0] == 0


@pytest.mark.parametrize("name", CASE_IDS)
def test_forward_ragged_batch(name, mode):
    """Molecules of 1, 2, 9, 16, 17, 18, 33 and 40 atoms: empty and one-slot half tiles, an atom without neighbours; finite
    outputs within the mode's gate."""
    m = hip(name, mode)
    bt = CS.refs(name, "ragged")[0]
    check(name, "ragged", mode, forward3(m, bt), "config_space_forward")
    if name in CS.KP32:
        check_half_tiles(m, name, len(bt["batch"]), mode)


@pytest.mark.parametrize("name", CS.KP32)
def test_combine_does_not_depend_on_what_the_workspace_held(name, mode):
    """KP = 32: a forward on the full batch with positions scaled by 8 (large attention rows in every half-tile row), then the
    ragged batch on the same context and workspace: its result is the oracle's, so no half-tile row of an atom with an empty
    tile (the one- and two-atom molecules have both or one) carries over."""
    m = hip(name, mode)
    big, bt = CS.refs(name, "full")[0], CS.refs(name, "ragged")[0]
    assert len(big["batch"]) > len(bt["batch"])      # the second forward does not grow (and so clear) the workspace
    forward3(m, big, scale=8.0)
    res = forward3(m, bt)
    assert int(m.debug_read("dims", (8,), np.int64)[6]) >= len(big["batch"])
    check(name, "ragged", mode, res, "config_space_after_full")


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", CS.CHAIN_CASES)
def test_short_chain(name, use_graph, mode):
    """Three reverse steps with host-fed noise against the oracle's chain: coordinates within POS_TOL, atom types exact; eagerly
    and as a captured step (which holds the half-tile buffer's addresses and, at 32 atom types, the C > 16 posterior kernel)."""
    m = hip(name, mode)
    bt, eps, u, ref = CS.chain_ref(name)
    r = m.sample_diffusion(T(bt["pos"], DEV), T(bt["v"], DEV), T(bt["batch"], DEV), T(bt["shape"], DEV).view(len(bt["shape"]), -1),
                           num_steps=CS.CHAIN_STEPS, center_pos_mode="none", noise=(T(eps, DEV), T(u, DEV)), use_graph=use_graph)
    m.check_status()
    err = maxabs(r["pos"], ref["pos"])
    mism = int((r["v"].cpu().numpy() != ref["v"].numpy()).sum())
    print("config_space_chain", name, mode, use_graph, err, mism)
    record("config_space_chain", config=name, mode=mode, use_graph=use_graph, pos=err, v_mismatch=mism)
    assert mism == 0 and err < POS_TOL, (err, mism)
    if name in CS.KP32:
        assert m.debug_read("launch_edge", (4,), np.int64)[0] == 1


def test_single_tile_edge_kernels_refuse_k_above_16():
    """edge_bf16 = 0 / 1 (kernels of single-tile jobs) are refused for k > 16, and the context keeps its mode.  (At hidden width
    128: no context exists for k > 16 at width 32, see below.)"""
    from shapemol_amd._lib import ShapeMolLibraryError
    m = hip("h128_k17", "exact")
    for v in (0, 1):
        with pytest.raises(ShapeMolLibraryError, match="k > 16"):
            m.set_option("edge_bf16", v)
    check("h128_k17", "ragged", "exact", forward3(m, CS.refs("h128_k17", "ragged")[0]), "config_space_after_refusal")


@pytest.mark.parametrize("name", list(CS.REFUSED))
def test_model_with_k_above_16_at_hidden_width_32_is_refused(name):
    """The rows of the grid that shapemol_create refuses: the module reports the library's message, which names the limit, when
    its context would be created; nothing is launched."""
    import shapemol_amd
    from shapemol_amd import synth
    from shapemol_amd._lib import ShapeMolLibraryError
    cfg, C = CS.config(name), CS.classes(name)
    m = shapemol_amd.ScorePosNet3D(cfg, C)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synthetic_state_dict(cfg, seed=7, num_classes=C).items()}, strict=True)
    bt = CS.ragged_batch("h32_k9")
    with pytest.raises(ShapeMolLibraryError, match="knn > 16 needs hidden_dim 128"):
        m = m.to(DEV)
        m(T(bt["pos"], DEV), T(bt["v"] % C, DEV), T(bt["batch"], DEV), T(synth.hash_normal((8, cfg["shape_dim"], 3), 203, 1), DEV), T(bt["t"], DEV))
