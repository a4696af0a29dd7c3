"""CPU side of the configuration-space gates (tests/test_gpu_config_space.py): the batches of tests/config_space.py have
unambiguous kNN graphs, and the float64 oracle of every case responds to the LAST element of every dimension the kernels loop
over -- so a kernel that drops or mis-indexes a tail element cannot pass the GPU gate."""
import numpy as np
import pytest
import torch

import config_space as CS
import precision as P
from util import O, T, record, synth

SENSITIVITY = 100.0        # a change must move an output by more than this many gate bounds


def test_table_matches_the_grid():
    """The configurations of the grid (three of its nine rows refused by shapemol_create, one added in their place), the two
    batches of each, and the sizes the suite is allowed to spend on them."""
    assert len(CS.CASES) == 7 and set(CS.REFUSED) == {"h32_k32", "h32_k17", "h32_max_k32"} and not set(CS.REFUSED) & set(CS.CASES)
    assert all(c[0]["hidden_dim"] == 32 and c[0]["knn"] > 16 for c in CS.REFUSED.values())
    for name in CS.CASES:
        ov, C = CS.overrides(name), CS.classes(name)
        assert ov["num_layers"] <= 3 and ov["n_heads"] * 8 == ov["hidden_dim"]
        for which in CS.BATCHES:
            bt = CS.batch(name, which)
            assert 6 <= len(bt["counts"]) <= 8 and len(bt["batch"]) <= 300
            assert bt["shape"].shape == (len(bt["counts"]), ov["shape_dim"], 3) and bt["v"].max() < C and bt["t"].shape == bt["counts"].shape
        assert CS.batch(name, "full")["counts"].min() >= max(ov["knn"] + 2, 6)
        assert tuple(CS.batch(name, "ragged")["counts"]) == CS.RAGGED_COUNTS
    assert set(CS.KP32) == {"h128_k17"}
    assert set(CS.batch("h32_max_k16", "full")["v"].tolist()) == set(range(32))


@pytest.mark.parametrize("which", CS.BATCHES)
@pytest.mark.parametrize("name", list(CS.CASES))
def test_batches_have_unambiguous_knn_graphs(name, which):
    """Every molecule with more than k + 1 atoms has a relative kNN margin of at least precision.MARGIN, the recorded seed is the
    first from the case's base that has, and the float32 kNN graph equals the one from float64 distances."""
    k = CS.overrides(name)["knn"]
    bt = CS.batch(name, which)
    assert P.knn_margin(bt, k) >= P.MARGIN
    assert CS.first_seed(name, which) == CS.CASES[name][3 if which == "full" else 4]
    s32, d32 = O.knn_edges(T(bt["pos"]), T(bt["batch"]), k)
    s64, d64 = O.knn_edges(T(bt["pos"]).double(), T(bt["batch"]), k)
    assert np.array_equal(d32.numpy(), d64.numpy()) and len(d32) == int(np.minimum(bt["counts"] - 1, k).dot(bt["counts"]))
    o32, o64 = np.lexsort((s32.numpy(), d32.numpy())), np.lexsort((s64.numpy(), d64.numpy()))
    assert np.array_equal(s32.numpy()[o32], s64.numpy()[o64])


def _moved(changed, r64, r32):
    """{output: movement / gate bound} of the three outputs under a change of the inputs or weights."""
    return {k: P.rel_err(changed[k], r64[k]) / P.bound(P.rel_err(r32[k], r64[k])) for k in CS.OUTPUTS}


@pytest.mark.parametrize("name", list(CS.CASES))
def test_oracle_is_sensitive_to_the_last_element_of_every_dimension(name):
    """On the full batch, each of (a) the last shape point zeroed, (b) the last shape-latent column of layer 0's x2h value
    MLP zeroed (the value MLP: with k = 1 the softmax over one neighbour is 1 whatever the key MLP computes), (c) the last time-embedding column of the atom embedding zeroed, (d) for k > 16 the farthest neighbour dropped
    (knn = k - 1, same weights) moves one of the three outputs by more than 100 gate bounds (4 e32 + 16 u of that output)."""
    bt, r32, r64 = CS.refs(name, "full")
    sdn, cfg, C = CS.state_dict(name), CS.config(name), CS.classes(name)
    dm = O.Dims(cfg, C)
    k, S, SL, D, H, G = cfg["knn"], cfg["shape_dim"], cfg["shape_latent_dim"], cfg["time_emb_dim"], cfg["hidden_dim"], cfg["num_r_gaussian"]
    for key in CS.OUTPUTS:
        assert np.isfinite(r64[key]).all() and 0 < P.rel_err(r32[key], r64[key]) < 64 * P.U, key

    def with_weight(key, col):
        sd2 = dict(sdn)
        w = sdn[key].copy()
        assert w.shape[1] == col + 1 and np.abs(w[:, col]).max() > 0
        w[:, col] = 0
        sd2[key] = w
        return CS.score3(O.state_dict_from_numpy(sd2), dm, bt)

    moved = {}
    b2 = dict(bt)
    b2["shape"] = bt["shape"].copy()
    b2["shape"][:, S - 1] = 0
    sd = CS.oracle(name)[0]
    moved["shape_point"] = _moved(CS.score3(sd, dm, b2), r64, r32)
    moved["shape_latent_col"] = _moved(with_weight("refine_net.base_block.0.x2h_layers.0.hv_func.net.0.weight", G + 2 * H + SL - 1), r64, r32)
    moved["time_emb_col"] = _moved(with_weight("ligand_atom_emb.weight", C + D - 1), r64, r32)
    if k > 16:
        cfg2 = dict(cfg)
        cfg2["knn"] = k - 1
        moved["farthest_neighbour"] = _moved(CS.score3(sd, O.Dims(cfg2, C), bt), r64, r32)
    record("config_space_sensitivity", config=name, weight_seed=CS.weight_seed(name), **{c: max(m.values()) for c, m in moved.items()})
    weak = {c: m for c, m in moved.items() if max(m.values()) <= SENSITIVITY}
    assert not weak, weak


def _create(cfg, C):
    """(return code, error message) of shapemol_create for a model configuration with hash-filled weights.  The validator runs
    before the library touches a device."""
    import ctypes
    from shapemol_amd import _lib, pack_state_dict
    from shapemol_amd.spec import ModelDims
    d = ModelDims(cfg, C)
    packed = np.ascontiguousarray(pack_state_dict(synth.synthetic_state_dict(cfg, seed=7, num_classes=C), d.L), np.float32)
    conf = _lib.Config(d.H, d.heads, d.L, d.k, d.G, d.S, d.S_latent, d.temb, d.C, d.T)
    lib, ctx = _lib.load(), ctypes.c_void_p()
    rc = lib.shapemol_create(ctypes.byref(conf), packed.ctypes.data_as(ctypes.c_void_p), packed.size, 0, ctypes.byref(ctx))
    msg = lib.shapemol_last_error().decode()
    if rc == 0:
        lib.shapemol_destroy(ctx)
    return rc, msg


@pytest.mark.parametrize("name", list(CS.REFUSED))
def test_create_refuses_k_above_16_at_hidden_width_32(name):
    """shapemol_create refuses the reduced model with k > 16 before it touches a device, and names the limit: the h2x half-atom
    tiles store rows of 48 floats where the workspace has rows of hidden_dim floats."""
    rc, msg = _create(CS.config(name), CS.classes(name))
    assert rc != 0
    assert all(w in msg for w in ("knn > 16", "hidden_dim 128", "knn 1..16")), msg


def test_create_refusal_is_about_the_combination():
    """k = 17 at hidden width 32 is refused for the combination alone: the same message does not come for k = 16 at width 32 (that
    configuration passes the validator: with a device the context is created, without one the call fails later, with another message)."""
    from util import model_cfg
    rc, msg = _create(model_cfg(hidden_dim=32, n_heads=4, num_layers=1, knn=16), 15)
    assert rc == 0 or "knn > 16" not in msg      # (a call that succeeds leaves the previous message in place)
    rc, msg = _create(model_cfg(hidden_dim=32, n_heads=4, num_layers=1, knn=17), 15)
    assert rc != 0 and "knn > 16" in msg
