"""Checks on the reference alone that keep tests/test_gpu_chain_forms.py honest: its batches sit on the boundaries they claim, the
lattice profile really ties at the k-th neighbour, the recomposition harness reports the float32 oracle inside the gate, and every
case's oracle outputs are finite.  The shapes that depend on the CU count are checked at 256, the MI355X's."""
import numpy as np
import pytest
import torch

import chain_forms as CF
import precision as P
from util import O, T, oracle_model

NUM_CU = 256
SEED = 5


@pytest.mark.parametrize("k", CF.GRAPH_KS)
def test_graph_counts_sit_on_the_chunk_edges(k):
    """Odd N (the last wave of a two-atom tile holds one atom), both sides of every candidate-chunk edge and of the cap, and --
    two atoms per wave -- a wave whose molecules have fewer | more chunks and one with more | fewer."""
    counts = CF.graph_counts(k)
    lanes = CF.graph_lanes(k)
    assert int(counts.sum()) % 2 == 1 and counts.max() == CF.GRAPH_CAP and CF.graph_fused_expected(counts)
    for edge in range(lanes, CF.GRAPH_CAP + 1, lanes):
        assert edge in counts and (edge - 1 in counts or edge + 1 in counts), edge
        assert edge == CF.GRAPH_CAP or edge + 1 in counts, edge
    for c in (1, 2, k, k + 1):
        assert c in counts
    if CF.kp_of(k) == 8:
        assert k + 2 in counts and 31 in counts and 127 in counts
        pairs = CF.wave_pairs(counts, k)
        assert any(a < b for a, b in pairs) and any(a > b for a, b in pairs), pairs
    assert not CF.graph_fused_expected(CF.graph_counts(k, extra=(129,)))


@pytest.mark.parametrize("k", CF.GRAPH_KS)
def test_lattice_profile_ties_at_the_kth_neighbour(k):
    """Every molecule with more than k + 1 atoms has an atom whose k-th and (k + 1)-th squared distances are equal in float32 (the
    'lower index first' rule decides its list), and the batch holds zero distances."""
    counts = CF.graph_counts(k)
    bb = CF.batch(counts, SEED, "lattice")
    off = np.concatenate([[0], np.cumsum(counts)])
    zeros = 0
    for m, c in enumerate(counts):
        ties, z = CF.kth_ties(bb["init_pos"][off[m]:off[m + 1]], k)
        zeros += z
        assert c <= k + 1 or ties > 0, (m, int(c))
    assert zeros > 0
    assert np.array_equal(bb["init_pos"], np.round(bb["init_pos"])) and np.abs(bb["init_pos"]).max() <= 4


def test_fold_cases_fill_the_table_exactly():
    """Each `full` case has a workgroup whose molecule span is the whole table and folds; its `over` partner is one row over and
    does not; the streaming cases have the chunk they claim."""
    cases = CF.fold_cases(NUM_CU)
    assert set(cases) == {f"{p}_{s}" for p in ("exact_k8_chunk1", "exact_k8_chunk2", "exact_k12_chunk2", "f16x2_k8") for s in ("full", "over")}
    assert cases["exact_k8_chunk1_full"][2].tolist() == [1, 128, 128] and cases["exact_k8_chunk1_over"][2].tolist() == [1, 128, 129]
    for name, (mode, k, counts, on) in cases.items():
        n, kp = int(counts.sum()), CF.kp_of(k)
        a = CF.fold_atoms(mode, n, kp, NUM_CU)
        assert CF.fold_expected(mode, counts, k, NUM_CU) == on, name
        assert CF.straddled_span(counts, a) == CF.FOLD_CAP + (0 if on else 1), name
        assert n <= 1100
        if mode == "exact" and "chunk" in name:
            assert CF.stream_chunk(n, kp, NUM_CU) == int(name.split("chunk")[1][0]), name
    assert 513 <= int(cases["exact_k8_chunk2_full"][2].sum()) <= 1024 and cases["exact_k8_chunk2_full"][2].max() == 127
    assert cases["f16x2_k8_full"][2].max() == 121


@pytest.mark.parametrize("kp", [8, 16, 32])
def test_stream_sizes_hit_the_tails(kp):
    s = CF.stream_sizes(kp, NUM_CU)
    step = 2 if kp > 16 else 1
    for c in (1, 2):
        assert [CF.stream_jobs(s[f"c{c}{d}"], kp) - NUM_CU * c for d in "mep"] == [-step, 0, step]
    n = s["chunk3_short"]
    chunk, jobs = CF.stream_chunk(n, kp, NUM_CU), CF.stream_jobs(n, kp)
    assert chunk == (3 if kp <= 16 else 4) and jobs % chunk != 0 and CF.stream_grid(n, kp, NUM_CU) == jobs // chunk + 1
    assert [CF.stream_chunk(s[f"c{c}e"], kp, NUM_CU) for c in (1, 2)] == ([1, 2] if kp <= 16 else [2, 2])
    assert max(s.values()) <= 1100 and (kp != 8 or all(v % 2 == 1 for v in s.values()))


def test_recompose_reports_the_float32_oracle_inside_the_gate():
    """The harness's self-test: fed with O.sample_chain's own trajectory, every step's predictions are the float32 oracle's at that
    state -- eH = e32 -- and the posterior recomposition (tests/vocab.py) holds the oracle's own step."""
    import vocab as V
    sd, dm, _, _ = oracle_model()
    bb = CF.batch([1, 30, 17, 9], SEED, steps=3)
    r = O.sample_chain(sd, dm, T(bb["init_pos"]), T(bb["init_v"]), T(bb["batch"]), T(bb["shape"]), 3, lambda s: (bb["eps"][s], bb["u"][s]))
    for s in range(3):
        r32, r64, t = CF.recompose(sd, dm, bb, r, s)
        g = CF.score_gate(r["pos_cond_traj"][s], r["v_cond_traj"][s], r32, r64)
        for key, (eh, e32, over) in g.items():
            assert eh == e32 and over <= 1.0, (s, key, eh, e32)
        pos, v = CF.step_state(bb, r, s)
        args = (pos, v, r["pos_cond_traj"][s].numpy(), r["v_cond_traj"][s].numpy(), T(bb["batch"]), t, bb["eps"][s], bb["u"][s])
        got = {"x": r["pos_traj"][s].numpy(), "v0": r["v0_traj"][s].numpy(), "vt": r["vt_traj"][s].numpy(), "v": r["v_traj"][s].numpy()}
        pg, wrong, _ = V.step_gate(got, V.posterior_step32(sd, dm, *args), V.posterior_step64(sd, 15, *args))
        assert max(x[2] for x in pg.values()) <= 1.0 and wrong == 0


def _finite(sd, dm, bb, dtypes=(torch.float32, torch.float64)):
    t = torch.full((len(bb["counts"]),), dm.T - 1, dtype=torch.long)
    for dt in dtypes:
        o = O.score(sd, dm, T(bb["init_pos"]), T(bb["init_v"]), T(bb["batch"]), T(bb["shape"]), t, dtype=dt)
        assert all(bool(torch.isfinite(o[k]).all()) for k in ("pred_ligand_pos", "pred_ligand_h", "pred_ligand_v")), dt


@pytest.mark.parametrize("profile", CF.PROFILES)
@pytest.mark.parametrize("k", CF.GRAPH_KS)
def test_graph_cases_have_finite_oracle_outputs(k, profile):
    """Float32 and float64 score of every graph-stage batch (zero distances included), its reference lists and edge weights."""
    sd, dm, _, _ = oracle_model(knn=k)
    bb = CF.batch(CF.graph_counts(k), SEED, profile)
    _finite(sd, dm, bb)
    nbr, valid, ew32, ew64 = CF.graph_reference(sd, dm, bb)
    assert np.isfinite(ew32).all() and np.isfinite(ew64).all()
    assert valid.sum(1).tolist() == np.minimum(k, np.repeat(bb["counts"], bb["counts"]) - 1).tolist()
    assert P.rel_err(ew32, ew64) < 1e-5


def test_fold_cases_have_finite_oracle_outputs():
    for name, (mode, k, counts, _) in CF.fold_cases(NUM_CU).items():
        sd, dm, _, _ = oracle_model(knn=k)
        _finite(sd, dm, CF.batch(counts, SEED))


@pytest.mark.parametrize("k", sorted(CF.STREAM_KS))
def test_stream_cases_have_finite_oracle_outputs(k):
    sd, dm, _, _ = oracle_model(knn=k)
    for name, n in CF.stream_sizes(CF.kp_of(k), NUM_CU).items():
        bb = CF.stream_batch(k, n)
        assert len(bb["batch"]) == n and bb["counts"].min() >= 1
        _finite(sd, dm, bb)
