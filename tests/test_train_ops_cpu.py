"""What makes the gates of tests/test_gpu_train_ops.py meaningful, on the CPU: every case of tests/train_ops_cases.py is
well-posed (zero offenders of the mask conditions, from the float64 oracle alone), the float32 oracle is sane on it, no gated
gradient is identically zero, the graphs have the features their reasons name, and the partial counts written beside the cases
are what the host code computes."""
import math
import os
import re

import numpy as np
import pytest

import train_ops_cases as TC
import train_ops_f64 as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(kind, case) for kind, cases in TC.ALL.items() for case in cases]
IDS = [kind + "-" + TC.case_id(case) for kind, case in CASES]


# The formulas of shapemol_amd/csrc/train_ops.hip, restated once: row_splits (line 52), real_splits (lines 54-58, the chunk
# rounding of gemm(), line 20, with kGemmKC = 16 of sm_train.h:32), the 64-row blocks kLnRows (sm_train.h:261, train_ops.hip:77)
# and the VN workgroups (train_ops.hip:278-279).
def row_splits(rows):
    return max(1, min(256, rows // 256))


def real_splits(rows):
    sp = row_splits(rows)
    kchunk = (-(-rows // sp) + 15) // 16 * 16
    return -(-rows // kchunk)


def row_blocks(rows):
    return -(-rows // 64)


def vn_blocks(atoms, channels):
    return -(-atoms // (256 // channels))


def test_the_restated_constants_are_the_sources():
    """The three constants the restatement depends on, read from the sources it mirrors."""
    src = open(os.path.join(ROOT, "shapemol_amd", "csrc", "sm_train.h")).read()
    ops = open(os.path.join(ROOT, "shapemol_amd", "csrc", "train_ops.hip")).read()
    assert re.search(r"constexpr int kGemmKC = 16;", src)
    assert re.search(r"constexpr int kLnRows = 64,", src)
    assert "std::max<int64_t>(1, std::min<int64_t>(256, rows / 256))" in ops
    assert "kchunk = ((rows + sp - 1) / sp + kGemmKC - 1) / kGemmKC * kGemmKC" in ops


def test_the_boundaries_the_cases_are_there_for():
    assert [row_splits(r) for r in (511, 512, 513)] == [1, 2, 2] and [real_splits(r) for r in (511, 512, 513)] == [1, 2, 2]
    assert (row_splits(8448), real_splits(8448)) == (33, 33) and (row_splits(8449), real_splits(8449)) == (33, 32)
    assert (row_splits(65536), real_splits(65536)) == (256, 256) and (row_splits(65537), real_splits(65537)) == (256, 241)
    assert (row_blocks(2048), row_blocks(2049)) == (32, 33)


@pytest.mark.parametrize("kind,case", CASES, ids=IDS)
def test_case_is_well_posed(kind, case):
    inp, r32, r64, bad, taps = TO.evaluate(kind, case)
    assert bad == 0, f"{bad} offenders of the well-posedness conditions: move the seed (python tests/train_ops_f64.py)"
    zero = TC.zero_by_construction(kind, case)
    for key, ref in r64.items():
        assert np.isfinite(ref).all() and np.isfinite(r32[key]).all(), key
        if ref.size == 0:
            continue
        if key in zero:       # exact zeros of the mathematics: the oracles leave rounding noise there, nothing to gate against
            assert np.abs(ref).max() < 1e-9, key      # float64 noise times rstd = 1e-5 ** -0.5 = 316
            continue
        assert np.abs(ref).max() > 0, f"{key}: an all-zero reference makes its gate vacuous"
        e32 = TO.rel_err(r32[key], ref)
        assert math.isfinite(e32) and e32 < TO.SANE_E32, (key, e32)
    assert len(case.reason) > 20 and re.search(r"\b[ST]:\d+", case.reason), "every case names the line it is there for"


@pytest.mark.parametrize("kind,case", CASES, ids=IDS)
def test_expected_partial_counts(kind, case):
    if kind == "mlp":
        assert (case.splits, case.blocks) == (real_splits(case.rows), row_blocks(case.rows))
    elif kind == "edge":
        E = TO.evaluate(kind, case)[0]["src"].numel()
        assert case.n_edges in (None, E)
        assert (case.splits_e, case.splits_n) == (real_splits(E), real_splits(case.n_atoms))
    elif kind == "vn":
        assert case.blocks == vn_blocks(case.atoms, case.C)
        assert int(TO.vn_counts(case).sum()) == case.atoms
    else:
        assert (case.n_atoms * case.heads * 8) % 64 != 0 or case.heads == 16, "a wave with dead 8-lane groups"


def test_the_cases_cover_what_they_claim():
    """The values the issue of these gates lists, each present in the cases file."""
    rows = {c.rows for c in TC.MLP}
    assert {1, 63, 64, 65, 511, 512, 513, 2048, 2049, 8448, 8449, 65536, 65537} <= rows
    assert {15, 16, 17, 20, 308} <= {c.k_in for c in TC.MLP} and {1, 63, 64, 65, 100, 128, 256} <= {c.hidden for c in TC.MLP}
    assert {1, 65, 100, 300, 128} <= {c.n_out for c in TC.MLP}
    widths = {(c.k_edge, c.k_node, c.k_shape) for c in TC.EDGE}
    assert {(20, 128, 32), (4, 6, 4), (4, 6, 0), (7, 24, 0), (20, 6, 2)} <= widths
    assert {c.dh for c in TC.ATTN} == {1, 5, 8} and {c.W for c in TC.ATTN} == {1, 3, 8} and {c.heads for c in TC.ATTN} == {1, 3, 16}
    assert {c.C for c in TC.VN} == {1, 3, 16, 24, 64}
    for ch in (1, 3, 16, 24, 64):
        per, atoms = 256 // ch, {c.atoms for c in TC.VN if c.C == ch}
        assert {per - 1, per, per + 1} <= atoms and any(a > 32 * per for a in atoms), ch
    assert {255, 256, 257} <= {c.atoms for c in TC.VN if c.C == 16}
    assert any(c.rows_o == 0 for c in TC.VN) and any(c.rows_s == 0 for c in TC.VN) and any(not c.training for c in TC.VN)
    assert any(c.atoms == 2 and c.training for c in TC.VN)
    assert len({(k, c[:-1]) for k, cs in TC.ALL.items() for c in cs}) == len(CASES)


def test_graph_features():
    """The graphs have what their reasons say: empty centre segments, an atom that is nobody's neighbour, one long segment."""
    by = {TC.case_id(c): c for c in TC.EDGE}
    for c in TC.EDGE:
        inp = TO.evaluate("edge", c)[0]
        deg_in = np.diff(inp["ptr"].numpy())
        deg_out = np.bincount(inp["src"].numpy(), minlength=c.n_atoms)
        assert np.array_equal(inp["dst"].numpy(), np.repeat(np.arange(c.n_atoms), deg_in))
        if c.degrees[0] in ("rand", "set") and c.n_atoms > 2:
            assert (deg_in == 0).any() and deg_out[2] == 0
        if c.degrees[0] == "hub":
            assert deg_out[0] == inp["src"].numel() and (deg_out[1:] == 0).all()
    assert any(TO.evaluate("edge", c)[0]["src"].numel() == 1 for c in TC.EDGE) and len(by) == len(TC.EDGE)
    deg = np.diff(TO.evaluate("attn", next(c for c in TC.ATTN if c.degrees[0] == "set"))[0]["ptr"].numpy())
    assert set(deg.tolist()) == {0, 1, 40}


def test_big_logits_case():
    """About +-100 on eight atoms, the largest on the first edge of four and on the last edge of the other four; a softmax
    without its running maximum would overflow float32 (exp(100) > 3.4e38), and with it each of those atoms' weights is one-hot."""
    case = next(c for c in TC.ATTN if c.big_logits)
    inp, r32, r64, _, taps = TO.evaluate("attn", case)
    logit, ptr = taps["logit"], inp["ptr"].numpy()
    first = last = 0
    for i in range(case.n_atoms):
        seg = logit[ptr[i]:ptr[i + 1], 0]
        if seg.size and seg.max() > 99.0:
            assert abs(seg.max() - 100.0) < 1e-3 and abs(seg.min() + 100.0) < 1e-3
            first += int(seg.argmax() == 0 and seg.argmin() == seg.size - 1)
            last += int(seg.argmax() == seg.size - 1 and seg.argmin() == 0)
    assert first == 4 and last == 4
    with np.errstate(over="ignore"):
        assert np.exp(np.float32(100.0)) == np.inf
    assert np.abs(logit).max() < 101.0 and np.percentile(np.abs(logit), 50) < 10.0      # the other atoms keep ordinary logits


def test_gate_rejects_what_it_should():
    """The gate itself: the float32 oracle passes, an error of 1e-5 of the largest entry in one element does not, nor a NaN."""
    case = TC.MLP[3]
    inp, r32, r64, _, _ = TO.evaluate("mlp", case)
    assert all(g[3] for g in TO.gate(r32, r32, r64).values())
    bad = {k: v.copy() for k, v in r32.items()}
    bad["dW2"].flat[0] += 1e-5 * np.abs(r64["dW2"]).max()
    gates = TO.gate(bad, r32, r64)
    assert [k for k, g in gates.items() if not g[3]] == ["dW2"]
    bad["y"].flat[0] = np.nan
    assert not TO.gate(bad, r32, r64)["y"][3]
    assert TO.worst(gates)[0] == "dW2" and TO.worst(gates)[1] > 1.0
