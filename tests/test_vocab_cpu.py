"""The CPU oracle at class counts other than 15, against the reference's own runs (tests/golden/make_golden_vocab.py: the 10-type
and the 23-type vocabulary), before tests/test_gpu_vocab.py leans on it; the default of the new num_classes arguments; and the
float32 oracle inside the posterior-step gate of the GPU test on that test's own inputs."""
import numpy as np
import pytest
import torch

import precision as P
import vocab as V
from test_oracle_golden import FWD_TOL
from util import O, T, golden, hash_noise, maxabs, oracle_model, record, synth


def _fixture_batch(f):
    C = int(f["num_classes"])
    return C, synth.synthetic_batch(int(f["B"]), seed=int(f["seed"]), num_classes=C)


def test_num_classes_default_gives_the_same_bits():
    """synthetic_batch(num_classes=15) is the batch every existing fixture was made from (forward_small.npz stores its
    init_v), other class counts change init_v alone, and every class is present in the vocabulary fixtures' batches."""
    f = golden("forward_small.npz")
    a, b = synth.synthetic_batch(6, seed=33), synth.synthetic_batch(6, seed=33, num_classes=15)
    assert np.array_equal(a["init_v"], f["init_v"]) and a["init_v"].dtype == f["init_v"].dtype
    for k in a:
        assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
    c = synth.synthetic_batch(6, seed=33, num_classes=23)
    assert all(np.array_equal(a[k], c[k]) for k in a if k != "init_v") and c["init_v"].max() > 14
    sd15, sdd = synth.synthetic_state_dict(oracle_model()[2], seed=7), oracle_model()[3]
    assert all(np.array_equal(sd15[k], sdd[k]) for k in sd15)
    for C in (10, 23):
        _, bb = _fixture_batch(golden(f"forward_vocab_c{C}.npz"))
        assert set(bb["init_v"].tolist()) == set(range(C))


@pytest.mark.parametrize("C", [10, 23])
def test_forward_vocab_oracle_golden(C):
    f = golden(f"forward_vocab_c{C}.npz")
    _, bb = _fixture_batch(f)
    sd, dm, _, _ = oracle_model(num_classes=C)
    assert dm.C == C and (f["t"] == 0).any() and (f["t"] == 999).any()
    out = O.score(sd, dm, T(bb["init_pos"]), T(bb["init_v"]), T(bb["batch"]), T(bb["shape"]), T(f["t"]))
    assert out["pred_ligand_v"].shape[1] == C
    for k in ("pred_ligand_pos", "pred_ligand_h", "pred_ligand_v"):
        assert maxabs(out[k], f[k]) < FWD_TOL, k


@pytest.mark.parametrize("C", [10, 23])
def test_chain_vocab_oracle_golden(C):
    """20 reverse steps on hash noise: atom types exact at every step, positions within 1e-4; the fixture is robust (kNN margin
    and Gumbel gap as its generator demands)."""
    c = golden(f"chain_vocab_c{C}_b4_s20.npz")
    _, bb = _fixture_batch(c)
    S, seed = int(c["S"]), int(c["seed"])
    assert float(c["knn_margin"]) >= P.MARGIN and float(c["gumbel_gap"]) >= 1e-4
    sd, dm, _, _ = oracle_model(num_classes=C)
    eps, u = hash_noise(len(bb["batch"]), S, seed, c=C)
    r = O.sample_chain(sd, dm, T(bb["init_pos"]), T(bb["init_v"]), T(bb["batch"]), T(bb["shape"]), S, lambda s: (eps[s], u[s]))
    assert np.array_equal(r["v"].numpy(), c["v"])
    assert np.array_equal(torch.stack(r["v_traj"]).numpy(), c["v_traj"].astype(np.int64))
    assert c["v_traj"].max() == C - 1
    assert maxabs(r["pos"], c["pos"]) < 1e-4
    assert maxabs(torch.stack(r["pos_traj"]), c["pos_traj"]) < 1e-4
    assert maxabs(torch.stack(r["v0_traj"]), c["v0_traj"]) < 1e-4
    assert maxabs(torch.stack(r["vt_traj"]), c["vt_traj"]) < 1e-4


@pytest.mark.parametrize("C", V.POSTERIOR_CLASSES)
def test_posterior_step_gate_holds_for_the_float32_oracle(C):
    """The inputs of test_gpu_vocab.test_posterior_step_recomposed (N = 131, t = 2, 1, 0) through the float32 oracle: every class
    is among the atom types, and at most 1 % of the (step, atom) pairs have a top-two score gap too small to demand the float64
    arg-max; where it is demanded the float32 oracle samples it."""
    bb = V.counts_batch(V.POSTERIOR_COUNTS, C, V.POSTERIOR_SEED, V.POSTERIOR_STEPS)
    n = len(bb["batch"])
    assert n == 131 and set(bb["init_v"].tolist()) == set(range(C))
    sd, dm, _, _ = oracle_model(num_classes=C)
    batch = T(bb["batch"])
    pos, v = T(bb["init_pos"]), T(bb["init_v"])
    excluded = wrong = 0
    for s in range(V.POSTERIOR_STEPS):
        t = torch.full((len(bb["counts"]),), V.POSTERIOR_STEPS - 1 - s, dtype=torch.long)
        pr = O.score(sd, dm, pos, v, batch, T(bb["shape"]), t)
        args = (pos.numpy(), v.numpy(), pr["pred_ligand_pos"].numpy(), pr["pred_ligand_v"].numpy(), batch, t, bb["eps"][s], bb["u"][s])
        r32, r64 = V.posterior_step32(sd, dm, *args), V.posterior_step64(sd, C, *args)
        g, w, ex = V.step_gate(r32, r32, r64)
        record("posterior_step_cpu", C=C, step=s, **{k: val[1] for k, val in g.items()}, excluded=ex)
        wrong, excluded = wrong + w, excluded + ex
        pos, v = T(r32["x"]), T(r32["v"])
    assert wrong == 0
    assert excluded <= 0.01 * V.POSTERIOR_STEPS * n, excluded
