"""CPU side of the precision gates (tests/test_gpu_precision.py): the float64 oracle against the reference's own goldens, the
stress profiles of tests/precision.py, and the gate itself on emulated operand formats."""
import json

import numpy as np
import pytest
import torch

import precision as P
from util import O, T, golden, oracle_model, record


def _score(sd, dm, f, pos, v, tkey, dtype):
    return O.score(sd, dm, T(f[pos]), T(f[v]), T(f["batch"]), T(f["shape"]), T(f[tkey]), dtype=dtype)


@pytest.mark.parametrize("case", ["b4_t999", "b4_t500", "b4_t0", "b4_tmix", "small", "k32"])
def test_float64_oracle_reproduces_reference_goldens(case):
    """The reference's float32 outputs lie within the gate of the float64 oracle (the reference is a float32 implementation
    too), the float64 oracle differs from the float32 one by a non-zero amount of float32 size, and both use one graph."""
    if case.startswith("b4"):
        sd, dm, _, _ = oracle_model()
        f, tkey, pos, v, pre = golden("forward_b4.npz"), case[3:] + "_t", "pos", "v", case[3:] + "_"
    else:
        f = golden(f"forward_{case}.npz")
        sd, dm, _, _ = oracle_model(seed=9, **json.loads(str(f["overrides"])))
        tkey, pos, v, pre = "t", "init_pos", "init_v", ""
    r64 = _score(sd, dm, f, pos, v, tkey, torch.float64)
    r32 = _score(sd, dm, f, pos, v, tkey, torch.float32)
    for k in ("pred_ligand_pos", "pred_ligand_h", "pred_ligand_v"):
        assert r64[k].dtype == torch.float64
        e_ref, e32 = P.rel_err(f[pre + k], r64[k].numpy()), P.rel_err(r32[k].numpy(), r64[k].numpy())
        assert 0 < e32 < 64 * P.U, (k, e32)
        assert e_ref <= P.bound(e32), (k, e_ref, e32)


def test_float32_path_unchanged_by_the_dtype_argument():
    """dtype=float32 is the plain oracle, bit for bit."""
    sd, dm, _, _ = oracle_model()
    f = golden("forward_b4.npz")
    a = O.score(sd, dm, T(f["pos"]), T(f["v"]), T(f["batch"]), T(f["shape"]), T(f["tmix_t"]))
    b = _score(sd, dm, f, "pos", "v", "tmix_t", torch.float32)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_profiles_are_deterministic_and_carry_their_scales():
    cfg = P.config("b4")
    p0, _ = P.state_dict("P0", cfg)
    for prof in P.PROFILES:
        a, sa = P.state_dict(prof, cfg)
        b, sb = P.state_dict(prof, cfg)
        assert sa == sb and all(np.array_equal(a[k], b[k]) and a[k].dtype == p0[k].dtype for k in a), prof
        ba, bb = P.batch(prof, "b4"), P.batch(prof, "b4")
        assert all(np.array_equal(ba[k], bb[k]) for k in ba), prof
    p1, s1 = P.state_dict("P1", cfg)
    net0 = [k for k in p0 if ".net.0." in k]
    assert set(s1) == set(net0) and len(net0) >= 6 * 8 * 2
    for k in p0:
        assert np.array_equal(p1[k], p0[k] * np.float32(P.SMALL) if k in s1 else p0[k]), k
    p2, s2 = P.state_dict("P2", cfg)
    exps = {int(np.log2(s)) for s in s2.values()}
    assert exps <= set(range(P.P2_EXP[0], P.P2_EXP[1] + 1)) and min(exps) == P.P2_EXP[0] and max(exps) == P.P2_EXP[1]
    for k, s in s2.items():
        w = p2[k].astype(np.float64) / s
        assert np.isfinite(w).all() and np.abs(p2[k]).max() < 6e4
        if w.size >= 4096:       # heavy tails: kurtosis of Laplace (6) with outliers, against 1.8 for the uniform fill
            z = w - w.mean()
            assert (z ** 4).mean() / (z ** 2).mean() ** 2 > 6, k
    for k in p0:
        if k not in s2:
            assert np.array_equal(p2[k], p0[k]), k
    b3 = P.batch("P3", "b256")
    start = np.concatenate([[0], np.cumsum(b3["counts"])[:-1]])
    cen = np.stack([b3["pos"][s:s + c].mean(0) for s, c in zip(start, b3["counts"])])
    assert np.abs(cen).min() > 15 and np.abs(cen).max() < 65
    gap = np.linalg.norm(b3["pos"][start + 1].astype(np.float64) - b3["pos"][start], axis=1)
    assert gap.min() > 0.004 and gap.max() < 0.021
    assert (b3["t"] == 0).any() and (b3["t"] == 999).any() and ((b3["t"] > 0) & (b3["t"] < 999)).any()


@pytest.mark.parametrize("profile", ["base", "P3"])
@pytest.mark.parametrize("cname", list(P.CONFIGS))
def test_profile_batches_have_unambiguous_knn_graphs(cname, profile):
    """Every atom's k-th and (k+1)-th neighbours differ by at least MARGIN relative in squared distance, and the float32
    kNN graph equals the one from float64 distances (P0-P2 share one batch)."""
    bt = P.batch("P0" if profile == "base" else profile, cname)
    k = P.config(cname)["knn"]
    assert P.knn_margin(bt, k) >= P.MARGIN
    assert bt["counts"].min() > k + 1       # every atom has k neighbours: the gates compare full rows
    s32, d32 = O.knn_edges(T(bt["pos"]), T(bt["batch"]), k)
    s64, d64 = O.knn_edges(T(bt["pos"]).double(), T(bt["batch"]), k)
    n = len(bt["batch"])
    assert np.array_equal(d32.numpy(), d64.numpy())
    assert np.array_equal(np.sort(s32.numpy().reshape(n, k), 1), np.sort(s64.numpy().reshape(n, k), 1))


@pytest.mark.parametrize("cname", ["b4", "small"])
def test_gate_separates_emulated_operand_formats(cname):
    """Matrix operands rounded to the kernels' formats, the rest in float64: the exactly split bf16 operands pass the gate on
    every profile, two-piece f16 operands exceed it at least 3x on P1.  Also checks that the float32 and float64 oracles see
    one edge list and that P2 keeps the residual stream far inside the fp16 range of the two-piece node kernels."""
    cfg = P.config(cname)
    dm = O.Dims(cfg)
    worst = {}
    for prof in P.PROFILES:
        sd = O.state_dict_from_numpy(P.state_dict(prof, cfg)[0])
        bt = P.batch(prof, cname)
        r64 = P.oracle_outputs(sd, dm, bt)
        r32 = P.oracle_outputs(sd, dm, bt, torch.float32)
        assert np.array_equal(r32["nbr"], r64["nbr"])
        assert max(np.abs(r32[k]).max() for k in r32 if k.startswith("h@")) < 6e4 / 64
        ex = P.gate(P.oracle_outputs(sd, dm, bt, operands=P.bf16x3), r32, r64)
        assert max(v[2] for v in ex.values()) <= 1.0, (prof, ex)
        worst[prof] = max(v[2] for v in P.gate(P.oracle_outputs(sd, dm, bt, operands=P.f16x2), r32, r64).values())
    assert worst["P1"] >= 3.0, worst


def test_c23_profiles_cover_the_vocabulary_and_record_e32():
    """The 23-type configuration of the gates: every class among the atom types of both batches, the state dicts sized by it, and
    the float32 oracle's own error e32 per profile and output (recorded: the bound the kernels are held to is 4 e32 + 16 u)."""
    cfg, C = P.config("c23"), P.classes("c23")
    assert C == 23 and all(P.classes(n) == 15 for n in P.CONFIGS if n != "c23")
    dm = O.Dims(cfg, C)
    for prof in P.PROFILES:
        sdn, _ = P.state_dict(prof, cfg, num_classes=C)
        assert sdn["v_inference.2.weight"].shape == (C, dm.H) and sdn["ligand_atom_emb.weight"].shape == (dm.H, C + dm.temb)
        bt = P.batch(prof, "c23")
        assert set(bt["v"].tolist()) == set(range(C))
        sd = O.state_dict_from_numpy(sdn)
        r64, r32 = P.oracle_outputs(sd, dm, bt), P.oracle_outputs(sd, dm, bt, torch.float32)
        assert np.array_equal(r32["nbr"], r64["nbr"]) and r64["pred_ligand_v"].shape[1] == C
        e32 = {k: P.rel_err(r32[k], r64[k]) for k in r64 if k != "nbr"}
        record("precision_cpu_e32", config="c23", profile=prof, **e32)
        assert 0 < e32["pred_ligand_v"] < 64 * P.U and 0 < e32["pred_ligand_pos"] < 64 * P.U, e32
