"""Precision gates of the HIP forward against a float64 oracle: the default exact mode (and every option variant that claims
float32 precision) must stay within a small multiple of the float32 oracle's own error on every stress profile of
tests/precision.py, and the two-piece f16 modes must not (negative controls: the gate can tell the modes apart).

Per output Y (e_w; h and dx = x_l - pos_in after stop_layer 1, 2, 4, 8; the final pred_ligand_pos / _h / _v):
e32 = max|Y32 - Y64| / max|Y64|, eH = max|YHIP - Y64| / max|Y64|, and the gate is eH <= 4 e32 + 16 * 2^-24 (precision.bound
states the error model it comes from).  The kernels' neighbour lists must equal the oracle's edge lists.  Run on the GPU box:
pytest tests -m gpu -k precision"""
import numpy as np
import pytest
import torch

import precision as P
from util import O, T, record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

F16X2 = {"f16x2": {"edge_bf16": 3, "node_f16": 1}, "edge_f16x2": {"edge_bf16": 3, "node_f16": 0},
         "node_f16x2": {"edge_bf16": 2, "node_f16": 1}}
EXACT_VARIANTS = {"edge_fp32": {"edge_bf16": 0}, "edge_bf16x6_phase": {"edge_bf16": 1}, "node_fp32": {"lin_bf16": 0, "chain_bf16": 0},
                  "vn_separate": {"vn_fuse": 0}, "vn_grid_barrier": {"vn_fuse": 1}}

_models, _refs = {}, {}


def _restore():
    """The library defaults, in a safe order (feat_f16 first: it needs the f16 kernels while it is set)."""
    from shapemol_amd.molopt_score_model import DEFAULT_OPTIONS as D
    return (("feat_f16", D["feat_f16"]), ("edge_bf16", D["edge_bf16"]), ("node_f16", D["node_f16"]), ("lin_bf16", 1), ("chain_bf16", 1),
            ("vn_fuse", 2), ("stop_layer", -1))


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    for m in _models.values():
        m._release()
    _models.clear()
    _refs.clear()


def model(profile, cname):
    """The HIP model of a profile's weights (P3 has P0's), built once per module."""
    key = ("P0" if profile == "P3" else profile, cname)
    if key not in _models:
        import shapemol_amd
        cfg = P.config(cname)
        sdn, _ = P.state_dict(key[0], cfg, num_classes=P.classes(cname))
        m = shapemol_amd.ScorePosNet3D(cfg, P.classes(cname))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=True)
        _models[key] = m.to(DEV)
    return _models[key]


def refs(profile, cname):
    """(batch, float32 oracle outputs, float64 oracle outputs), computed once per module."""
    key = (profile, cname)
    if key not in _refs:
        cfg = P.config(cname)
        sdn, _ = P.state_dict("P0" if profile == "P3" else profile, cfg, num_classes=P.classes(cname))
        sd, dm = O.state_dict_from_numpy(sdn), O.Dims(cfg, P.classes(cname))
        bt = P.batch(profile, cname)
        _refs[key] = (bt, P.oracle_outputs(sd, dm, bt, torch.float32), P.oracle_outputs(sd, dm, bt, torch.float64))
    return _refs[key]


def hip_outputs(m, bt):
    """The gate's outputs of the HIP forward: one evaluation per stop_layer, then the full one (whose nbr / ew are read)."""
    args = tuple(T(bt[k], DEV) for k in ("pos", "v", "batch", "shape", "t"))
    pos = bt["pos"].astype(np.float64)
    r = {}
    try:
        for nl in P.stop_layers(m.dims.L):
            m.set_option("stop_layer", nl)
            with torch.no_grad():
                out = m(*args)
            r[f"h@{nl}"] = out["pred_ligand_h"].double().cpu().numpy()
            r[f"dx@{nl}"] = out["pred_ligand_pos"].double().cpu().numpy() - pos
    finally:
        m.set_option("stop_layer", -1)
    with torch.no_grad():
        out = m(*args)
    m.check_status()
    for key in ("pred_ligand_pos", "pred_ligand_h", "pred_ligand_v"):
        r[key] = out[key].double().cpu().numpy()
    n, kp, k = len(bt["batch"]), int(m.debug_read("dims", (8,), np.int64)[2]), m.dims.k
    nbr = m.debug_read("nbr", (n, kp), np.int32)[:, :k].astype(np.int64)
    ew = m.debug_read("ew", (n, kp), np.float32)[:, :k].astype(np.float64)
    r["nbr"], r["ew"] = P._by_neighbour(nbr, ew)
    return r


def run_gate(profile, cname, opts, label):
    """Set `opts` on the profile's model, evaluate, restore the defaults; returns ({output: (eH, e32, eH / bound)}, nbr equal?)."""
    m = model(profile, cname)
    bt, r32, r64 = refs(profile, cname)
    try:
        for k, v in opts.items():
            m.set_option(k, v)
        res = hip_outputs(m, bt)
    finally:
        for k, v in _restore():
            m.set_option(k, v)
    g = P.gate(res, r32, r64)
    record("precision_gate", config=cname, profile=profile, mode=label, worst_over_bound=max(v[2] for v in g.values()),
           **{f"{k}_eH_over_e32": (v[0] / v[1] if v[1] > 0 else float("inf")) for k, v in g.items()})
    return g, np.array_equal(res["nbr"], r64["nbr"])


def _fails(g):
    return {k: f"eH {v[0]:.2e} > 4 e32 + 16u (e32 {v[1]:.2e}): {v[2]:.2f}x" for k, v in g.items() if v[2] > 1.0}


@pytest.mark.parametrize("profile", P.PROFILES)
@pytest.mark.parametrize("cname", list(P.CONFIGS))
def test_exact_mode_within_float32_floor(cname, profile):
    """The library default (every product on exactly split bf16 operands) at H = 128, k = 8, B = 4 and 256; k = 24 (the KP > 16
    half-tile path); k = 32 with 40-80-atom molecules; the H = 32 reduced model; 23 atom types (two output tiles of the
    atom-type head, 16 molecules) -- on every profile."""
    g, same_graph = run_gate(profile, cname, {}, "exact")
    assert same_graph, "HIP neighbour lists differ from the oracle's edge lists"
    assert not _fails(g), _fails(g)


@pytest.mark.parametrize("variant", list(EXACT_VARIANTS))
def test_exact_option_variants_within_float32_floor(variant):
    """The optional kernels that claim float32 precision (fp32 edge MFMA, bf16x6 phase edge kernels, fp32 node Linears, the two
    vector-neuron launch forms), on the small-operand profile P1 at B = 256."""
    g, same_graph = run_gate("P1", "b256", EXACT_VARIANTS[variant], variant)
    assert same_graph
    assert not _fails(g), _fails(g)


@pytest.mark.parametrize("variant", list(F16X2))
def test_f16x2_modes_fail_the_gate(variant):
    """Negative controls: the two-piece f16 products (all of them, the edge kernels' only, the node kernels' only) exceed the
    gate by at least 3x on some profile at B = 256 (P1: the residuals of small weights are fp16 subnormals).  A profile whose
    weights the mode's fp16 range guard rejects does not count."""
    worst = {}
    for profile in P.PROFILES:
        try:
            g, same_graph = run_gate(profile, "b256", F16X2[variant], variant)
        except RuntimeError as e:           # ShapeMolLibraryError of the range guard: the mode refused these weights
            if "fp16 range" not in str(e):
                raise
            worst[profile] = str(e)
            continue
        assert same_graph
        worst[profile] = max(v[2] for v in g.values())
    record("precision_gate_negative_control", mode=variant, **{p: w for p, w in worst.items()})
    assert max(w for w in worst.values() if isinstance(w, float)) >= 3.0, worst


def test_f16x2_mode_fails_the_gate_at_23_classes():
    """The negative control on the 23-type configuration (16 molecules): the two-piece f16 products exceed the gate by at least
    3x on some profile there too, so the c23 gates of test_exact_mode_within_float32_floor can tell the modes apart."""
    worst = {}
    for profile in P.PROFILES:
        try:
            g, same_graph = run_gate(profile, "c23", F16X2["f16x2"], "f16x2")
        except RuntimeError as e:           # ShapeMolLibraryError of the range guard: the mode refused these weights
            if "fp16 range" not in str(e):
                raise
            worst[profile] = str(e)
            continue
        assert same_graph
        worst[profile] = max(v[2] for v in g.values())
    record("precision_gate_negative_control", mode="f16x2", config="c23", **{p: w for p, w in worst.items()})
    assert max(w for w in worst.values() if isinstance(w, float)) >= 3.0, worst


def test_f16_features_mode_fails_the_gate():
    """feat_f16 (the leading f16 piece only) is far outside the gate already with the natural weights."""
    g, _ = run_gate("P0", "b256", {"edge_bf16": 3, "node_f16": 1, "feat_f16": 1}, "feat_f16")
    worst = max(v[2] for v in g.values())
    record("precision_gate_negative_control", mode="feat_f16", P0=worst)
    assert worst >= 3.0, worst
