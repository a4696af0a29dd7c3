"""The shape encoder's float64 stage recompositions (tests/shape_encoder_f64.py) tested on the CPU: they must accept a correct
float32 evaluation -- one whose latent is the CPU oracle's -- and reject the faults they exist to find."""
import functools

import pytest
import torch

import shape_encoder_f64 as S
from oracle import shape_encoder_oracle as SE

# (B, N, layer_num, latent_dim, seed of the clouds): the two smallest shapes of the GPU stage gates
CASES = ((1, 32, 4, 32, 3), (5, 48, 1, 7, 1))


@functools.lru_cache(maxsize=None)
def _case(B, N, L, LAT, seed):
    sd, pts = S.state_dict(L, LAT), S.clouds(B, N, seed)
    return sd, pts, S.forward(sd, pts, L)


@pytest.mark.parametrize("case", CASES)
def test_float32_evaluation_is_the_oracles(case):
    """The float32 evaluation in the device's formulation (per-point products, then an add per edge) gives the oracle's latent:
    the clouds are chosen so that the 20th-to-21st neighbour gap is at least 4 slacks in every row of every kNN."""
    B, N, L, LAT, seed = case
    sd, pts, f = _case(*case)
    assert S.least_margin(S.forward(sd, pts, L, S.F64)["feats"]) >= 4
    ref = SE.encode(sd, pts, L, S.K)
    assert tuple(ref.shape) == (B, LAT, 3) and float((f["final"]["out"] - ref).abs().max()) < 2e-5


@pytest.mark.parametrize("case", CASES)
def test_gates_accept_float32_and_the_oracles_topk(case):
    """Every kNN check accepts the oracle's topk, every value gate accepts float32, and at most 0.1 % of a stage's elements are
    left out (asserted by the gate itself)."""
    sd, pts, f = _case(*case)
    problems, gates = S.all_gates(sd, pts, case[2], f["stops"], f["final"])
    assert not problems, problems
    assert all(ok for _, _, ok in gates.values()), {k: v for k, v in gates.items() if not v[2]}
    assert {"conv_pos", "linear0", "edge0", "head_linear", "head"} <= set(gates)


def test_knn_check_rejects_wrong_neighbours():
    sd, pts, f = _case(*CASES[0])
    B, N = pts.shape[:2]
    feat, idx = f["feats"][2], f["stops"][2]["idx"].reshape(B, N, S.K)         # the kNN of block 1, in feature space
    assert not S.knn_problems(feat, idx)
    d2, _ = S.d2_and_slack(feat[0])
    far = idx.clone()
    far[0, 5, 7] = int(d2[5].argmax())                                         # one neighbour replaced by the farthest point
    assert any("nearest set" in m for m in S.knn_problems(feat, far))
    dup = idx.clone()
    dup[0, 9, 3] = dup[0, 9, 11]
    assert any("duplicate" in m for m in S.knn_problems(feat, dup))
    for bad in (N, -1):
        oob = idx.clone()
        oob[0, 0, 19] = bad
        assert any("out of range" in m for m in S.knn_problems(feat, oob))
    swapped = idx.clone()
    swapped[0, 4, [1, 18]] = idx[0, 4, [18, 1]]                                # a valid set in the wrong order
    assert any("ascending" in m for m in S.knn_problems(feat, swapped))
    no_self = idx.clone()
    row = no_self[0, 6]
    row[row == 6] = [j for j in range(N) if j not in row.tolist()][0]          # the point itself dropped from its own list
    assert S.knn_problems(feat, no_self)


def _failed(gates):
    return {k for k, v in gates.items() if not v[2]}


def test_value_gates_reject_wrong_operands():
    """Two weight rows swapped, Wf2 in place of Wf2 - Wf1, a block written at the neighbouring h_off, a wrong row of conv_c."""
    case = CASES[0]
    sd, pts, f = _case(*case)
    L, C = case[2], 128
    st = S.Stages(sd, pts, L)
    buf = f["stops"][2]                                                        # block 1
    assert not _failed(st.block(1, buf))
    # the device multiplies by a weight image with rows 3 and 4 of map_to_feat's first half exchanged
    wf = sd["blocks.1.map_to_feat.weight"].clone()
    wf[[3, 4]] = wf[[4, 3]]
    y = S.point_linear(st.block_input(1, buf, None), wf, sd["blocks.1.map_to_dir.weight"], S.F32)
    assert torch.nonzero((y != buf["y"]).any(0).any(1))[:, 0].tolist() == [3, 4, C + 3, C + 4]      # rows of Yf1 and Yf2
    assert "linear1" in _failed(st.block(1, dict(buf, y=y)))
    # Wf2 instead of Wf2 - Wf1
    wf = sd["blocks.1.map_to_feat.weight"].clone()
    wf[:, C:] += wf[:, :C]
    y = S.point_linear(st.block_input(1, buf, None), wf, sd["blocks.1.map_to_dir.weight"], S.F32)
    assert "linear1" in _failed(st.block(1, dict(buf, y=y)))
    # the output of block 1 written to the slice of block 2 (hcat of a complete evaluation, where every slice is filled)
    full = f["stops"][L]
    moved = full["hcat"].clone()
    moved[:, [1, 2]] = moved[:, [2, 1]]
    assert "edge1" in _failed(st.block(1, dict(buf, hcat=moved)))
    # conv_c: two product rows, two latent rows exchanged
    fin = f["final"]
    assert not _failed(st.head(fin))
    pd = fin["pd"].clone()
    pd[:, [0, 1]] = pd[:, [1, 0]]
    assert "head_linear" in _failed(st.head(dict(fin, pd=pd)))
    out = fin["out"].clone()
    out[:, [0, 1]] = out[:, [1, 0]]
    assert "head" in _failed(st.head(dict(fin, out=out)))


def test_edge_gate_uses_the_pooled_batch_statistics():
    """A batch of B shapes is not B batches of one: normalising each shape by its own statistics must fail the edge gate."""
    case = CASES[1]
    sd, pts, f = _case(*case)
    B, N = pts.shape[:2]
    st = S.Stages(sd, pts, case[2])
    buf = f["stops"][0]
    assert not _failed(st.conv_pos(buf))
    alone = torch.cat([S.forward(sd, pts[b:b + 1], case[2])["stops"][0]["h0"] for b in range(B)])
    assert "conv_pos" in _failed(st.conv_pos(dict(buf, h0=alone)))
