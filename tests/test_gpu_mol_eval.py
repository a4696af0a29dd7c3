"""The geometry scores on the device (shapemol_amd.evaluation, csrc/sm_mol_eval.h) against the reference's
stored results (tests/golden/mol_eval.npz) and the numpy oracle (tests/mol_eval_oracle.py, itself held to the reference by
tests/test_mol_eval_cpu.py).  Every output is an integer and must be equal: there is no tolerance in this file."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mol_eval_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("nr_bonds", "n_stable_atoms", "mol_stable", "hist_cc", "hist_all", "class_counts")


@pytest.fixture(scope="module")
def golden():
    return O.load_golden()


@pytest.fixture(scope="module")
def rule():
    from shapemol_amd import StabilityRule
    return StabilityRule.from_json(O.RULE_JSON)


@pytest.fixture(scope="module")
def orule():
    return O.Rule.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(report, expected, single=False):
    """Every output tensor of the report equals the oracle's array, dtype included."""
    for k in KEYS:
        e = torch.from_numpy(expected[k][0] if single else expected[k])
        t = getattr(report, k).cpu()
        assert t.dtype == e.dtype and t.shape == e.shape, (k, t.dtype, e.dtype, t.shape, e.shape)
        assert torch.equal(t, e), (k, int((t != e).sum()))


def chain(rng, n, lo=1.1, hi=1.6):
    """A random walk with steps of lo..hi A: compact enough that bonds of every order and crowded atoms occur."""
    u = rng.standard_normal((n, 3))
    u *= (rng.uniform(lo, hi, n) / np.linalg.norm(u, axis=1))[:, None]
    return np.cumsum(u, 0).astype(np.float32)


def batch_of(sizes):
    return np.repeat(np.arange(len(sizes)), sizes), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def by_mode(g, mode):
    """The fixture's molecules of one vocabulary as a packed batch: (molecule ids, pos, classes, batch, off)."""
    ids = np.flatnonzero(g["mode"] == O.MODES.index(mode))
    rows = np.concatenate([np.arange(g["off"][m], g["off"][m + 1]) for m in ids])
    batch, off = batch_of(np.diff(g["off"])[ids])
    return ids, rows, g["pos"][rows], g["classes"][rows], batch, off


def test_fixture_set_against_the_reference(golden, rule, orule):
    """Single frames, one call per vocabulary: the reference's stored check_stability results for hs False and True, its two
    profiles and Jensen-Shannon distances bit for bit, and the script's two validity fractions."""
    from shapemol_amd import evaluate_geometry
    g = golden
    n_atoms = np.diff(g["off"])
    for hs, tag in ((False, "nohs"), (True, "hs")):
        hist_cc = hist_all = 0
        stable_mols = stable_atoms = 0
        for mode in O.MODES:
            ids, rows, pos, cls, batch, off = by_mode(g, mode)
            r = evaluate_geometry(dev(pos), dev(cls), dev(batch), rule, mode=mode, hs=hs)
            assert np.array_equal(r.nr_bonds.cpu().numpy(), g[f"nr_bonds_{tag}"][rows])
            assert np.array_equal(r.n_stable_atoms.cpu().numpy(), g[f"n_stable_{tag}"][ids])
            assert np.array_equal(r.mol_stable.cpu().numpy(), g[f"mol_stable_{tag}"][ids])
            assert np.array_equal(r.class_counts.cpu().numpy(), np.bincount(cls, minlength=len(g["vocab"][mode])))
            same(r, O.evaluate(pos[None], cls[None], off, orule, orule.slots(g["vocab"][mode]), hs=hs), single=True)
            v = r.validity()
            assert v["mol_stable"] == g[f"mol_stable_{tag}"][ids].sum() / len(ids) and v["atm_stable"] == g[f"n_stable_{tag}"][ids].sum() / n_atoms[ids].sum()
            hist_cc, hist_all = hist_cc + r.hist_cc, hist_all + r.hist_all
            stable_mols, stable_atoms = stable_mols + int(r.mol_stable.sum()), stable_atoms + int(r.n_stable_atoms.sum())
            last = r
        assert stable_mols == g[f"mol_stable_{tag}"].sum() and stable_atoms == g[f"n_stable_{tag}"].sum()
        last.single, last.hist_cc, last.hist_all = False, hist_cc[None], hist_all[None]      # the set's histograms in one report
        prof = last.pair_length_profile()
        metrics = last.jsd({k: g[f"empirical_{k}"] for k in prof})
        for k in prof:
            assert prof[k].tobytes() == g[f"profile_{k}"].tobytes()
            assert np.float64(metrics[f"JSD_{k}"]).tobytes() == g[f"jsd_{k}"].tobytes()
        print(f"hs={hs}: stable molecules {stable_mols}/40, stable atoms {stable_atoms}/{n_atoms.sum()}, JSD {metrics}")


def test_fixture_set_as_a_trajectory(golden, rule, orule):
    """All 40 molecules as one packed batch over 8 frames: frame 0 as stored, the others moved and with other types."""
    from shapemol_amd import evaluate_trajectory
    g, rng = golden, np.random.default_rng(5)
    N = len(g["pos"])
    pos = np.stack([g["pos"]] + [g["pos"] + rng.uniform(-0.25, 0.25, (N, 3)).astype(np.float32) for _ in range(7)])
    cls = np.stack([g["classes"] % 15] + [rng.choice(15, N, p=np.r_[0.1, 0.5, np.full(13, 0.4 / 13)]) for _ in range(7)])
    batch, off = batch_of(np.diff(g["off"]))
    for hs in (False, True):
        exp = O.evaluate(pos, cls, off, orule, orule.slots(g["vocab"]["add_aromatic"]), hs=hs)
        r = evaluate_trajectory(dev(pos), dev(cls), dev(batch), rule, hs=hs, details=True)
        same(r, exp)
        assert r.forms == ["wave"] * 40
    steps = evaluate_trajectory([dev(p) for p in pos], [dev(c).to(torch.int32) for c in cls], batch, rule, hs=True)      # per-step tensors, int32 classes
    same(steps, exp)
    one = steps.validity(frame=3)
    assert one["mol_stable"] == exp["mol_stable"][3].mean() and one["atm_stable"] == exp["n_stable_atoms"][3].sum() / N
    assert steps.pair_length_profile(frame=slice(2, 5))["All_12A"].tobytes() == O.profile(exp["hist_cc"][2:5].sum(0), exp["hist_all"][2:5].sum(0))["All_12A"].tobytes()
    assert len(set(map(bytes, exp["nr_bonds"]))) == 8                            # the frames do differ


def test_form_boundaries(rule, orule, golden):
    """Molecules on both sides of every size at which the code takes another path, in one mixed batch of two frames."""
    from shapemol_amd import evaluate_trajectory
    sizes = [1, 2, 63, 64, 65, 255, 256, 257, 1024]
    rng = np.random.default_rng(11)
    pos = np.stack([np.concatenate([chain(rng, n) for n in sizes]) for _ in range(2)])
    cls = rng.choice(10, pos.shape[:2], p=np.r_[0.15, 0.45, 0.15, 0.15, np.full(6, 0.1 / 6)])
    batch, off = batch_of(sizes)
    r = evaluate_trajectory(dev(pos), dev(cls), dev(batch), rule, mode="basic", details=True)
    assert r.forms == ["wave"] * 4 + ["block"] * 5
    exp = O.evaluate(pos, cls, off, orule, orule.slots(golden["vocab"]["basic"]))
    same(r, exp)
    assert exp["orders"] == {0, 1, 2, 3} and exp["hist_cc"].sum() > 0 and exp["hist_all"][:, 0].sum() == 0
    assert exp["hist_all"].sum() < 2 * sum(n * (n - 1) // 2 for n in sizes)     # some pairs lie beyond the cut-off
    print("bonds per atom up to", int(exp["nr_bonds"].max()), "; stable atoms per molecule", exp["n_stable_atoms"][0].tolist())


def element_pairs(orule):
    """55 two-atom molecules, one per unordered pair of the rule's 10 elements, 0.9 .. 1.9 A apart."""
    rng = np.random.default_rng(3)
    E = len(orule.elements)
    pairs = [(a, b) for a in range(E) for b in range(a, E)]
    pos = np.zeros((len(pairs), 2, 3), np.float32)
    pos[:, 0] = rng.uniform(-5, 5, (len(pairs), 3))
    u = rng.standard_normal((len(pairs), 3))
    pos[:, 1] = pos[:, 0] + u * (rng.uniform(0.9, 1.9, len(pairs)) / np.linalg.norm(u, axis=1))[:, None]
    d = np.array([O.distances(p)[0, 1] for p in pos])
    return pairs, pos.reshape(-1, 3), np.array(pairs).reshape(-1), d


@pytest.mark.parametrize("level", [1, 2, 3])
def test_threshold_equality(rule, orule, level):
    """A threshold equal to the oracle's 100 * d is no bond of that level (strict <); the next float64 above it is.  A distance
    formed with a fused multiply-add, in another order or in float32 differs in the last bits for most of the 55 pairs."""
    from shapemol_amd import evaluate_geometry
    pairs, pos, slots, d = element_pairs(orule)
    p = 100 * d
    batch, _ = batch_of([2] * len(pairs))
    for bump, order in ((False, level - 1), (True, level)):
        r = copy.deepcopy(rule)
        r.margins[:] = 0
        r.bonds1[:], r.bonds2[:], r.bonds3[:] = 1000.0, 1000.0, 1000.0             # every lower level passes
        table = (r.bonds1, r.bonds2, r.bonds3)[level - 1]
        for (a, b), t in zip(pairs, np.nextafter(p, np.inf) if bump else p):
            table[a, b] = table[b, a] = t
        for t in (r.bonds1, r.bonds2, r.bonds3)[level:]:
            t[:] = -1.0                                                             # no higher level
        # "basic" lists the rule's ten elements in the rule's order, so an atom's class is its row of the rule
        rep = evaluate_geometry(dev(pos), dev(slots.astype(np.int64)), batch, r, mode="basic")
        assert rep.nr_bonds.cpu().tolist() == [order] * (2 * len(pairs)), (level, bump)


@pytest.mark.parametrize("which", ["cc", "all"])
def test_bin_edge_equality(rule, orule, which):
    """Edges equal to the pairs' own distances: side='left' puts d == edge[k] into bin k, not k + 1."""
    from shapemol_amd import evaluate_geometry
    rng = np.random.default_rng(8)
    M, reach = 120, (1.95 if which == "cc" else 11.9)
    pos = np.zeros((M, 2, 3), np.float32)
    pos[:, 0] = rng.uniform(-5, 5, (M, 3))
    u = rng.standard_normal((M, 3))
    pos[:, 1] = pos[:, 0] + u * (rng.uniform(0.3, reach, M) / np.linalg.norm(u, axis=1))[:, None]
    d = np.array([O.distances(q)[0, 1] for q in pos])
    edges = np.sort(d)
    assert len(np.unique(edges)) == M and edges[-1] < reach + 0.05
    batch, off = batch_of([2] * M)
    cls = np.full(2 * M, 1 if which == "cc" else 3)                             # carbon | oxygen
    kw = {"cc_bins": (edges, 2.0)} if which == "cc" else {"all_bins": (edges, 12.0)}
    r = evaluate_geometry(dev(pos.reshape(-1, 3)), dev(cls), batch, rule, mode="basic", **kw)
    h = (r.hist_cc if which == "cc" else r.hist_all).cpu().numpy()
    assert h.tolist() == [1] * M + [0]
    assert np.array_equal(h, np.bincount(np.searchsorted(edges, d, side="left"), minlength=M + 1))
    if which == "all":
        assert int(r.hist_cc.sum()) == 0                                        # no carbon


def test_minus_one_entries_and_nearly_coincident_atoms(rule, orule, golden):
    """A -1 entry is the threshold -1 + margin pm: H-H has thresholds 84 / 4 / 2 pm, Br-N 9 / 4 / 2 pm."""
    from shapemol_amd import evaluate_geometry
    gaps = [0.0, 0.01, 0.03, 0.05, 0.085, 0.1]
    pos = np.zeros((2 * len(gaps), 2, 3), np.float32)
    pos[:, 1, 0] = np.tile(gaps, 2)
    cls = np.array([[0, 0]] * len(gaps) + [[8, 2]] * len(gaps)).reshape(-1)        # basic: H H | Br N
    batch, off = batch_of([2] * (2 * len(gaps)))
    r = evaluate_geometry(dev(pos.reshape(-1, 3)), dev(cls), batch, rule, mode="basic")
    assert r.nr_bonds.cpu().view(-1, 2)[:, 0].tolist() == [3, 3, 2, 1, 1, 1] + [3, 3, 2, 1, 1, 0]
    same(r, O.evaluate(pos.reshape(1, -1, 3), cls[None], off, orule, orule.slots(golden["vocab"]["basic"])), single=True)
    assert int(r.hist_all[0]) == 2                                              # d == 0 lands in bin 0


def test_nan_and_coincident_atoms(rule, orule, golden):
    from shapemol_amd import evaluate_geometry
    pos = np.array([[0, 0, 0], [0, 0, 0], [np.nan, 0, 0], [1.5, 0, 0], [0, np.nan, 1], [2.5, 0.5, 0]], np.float32)
    cls = np.array([1, 1, 1, 1, 5, 1])
    r = evaluate_geometry(dev(pos), dev(cls), np.zeros(6, np.int64), rule)
    same(r, O.evaluate(pos[None], cls[None], [0, 6], orule, orule.slots(golden["vocab"]["add_aromatic"])), single=True)
    assert r.nr_bonds.cpu().tolist()[2] == 0 and r.nr_bonds.cpu().tolist()[4] == 0          # NaN atoms bond with nobody
    assert int(r.hist_all.sum()) == 6 and int(r.hist_all[0]) == 1 and int(r.hist_cc[0]) == 1   # 4 finite atoms: 6 pairs, one with d == 0


def test_class_past_the_add_aromatic_table(rule, orule, golden):
    from shapemol_amd import evaluate_geometry
    rng = np.random.default_rng(2)
    pos = chain(rng, 30)
    cls = rng.integers(0, 18, 30)
    cls[:3] = [15, 16, 17]
    slots = np.concatenate([orule.slots(golden["vocab"]["add_aromatic"]), orule.slots([6, 6, 6])])
    r = evaluate_geometry(dev(pos), dev(cls), np.zeros(30, np.int64), rule, num_classes=18)
    same(r, O.evaluate(pos[None], cls[None], [0, 30], orule, slots), single=True)
    assert r.class_counts.shape == (18,) and int(r.class_counts[15:].sum()) >= 3
    with pytest.raises(ValueError, match="outside"):
        evaluate_geometry(dev(pos), dev(cls), np.zeros(30, np.int64), rule)                # 15 classes by default


def raw_run(frames, off, pos, cls, rule, slots, outs):
    """shapemol_eval_run itself, with the caller's output tensors."""
    from shapemol_amd import _lib, evaluation as EV
    from shapemol_amd._native import ptr, stream_ptr
    thr, allowed, slots = rule.thresholds(), np.ascontiguousarray(rule.allowed_bonds), np.ascontiguousarray(slots, np.int32)
    off = np.ascontiguousarray(off, np.int64)
    with torch.cuda.device(DEV):
        return _lib.load().shapemol_eval_run(
            EV._contexts.of(torch.device(DEV)), frames, len(off) - 1, ptr(off), ptr(pos), ptr(cls), 1, len(rule.elements), ptr(thr), ptr(allowed), 1,
            len(slots), ptr(slots), ptr(O.CC_BINS), 100, 2.0, ptr(O.ALL_BINS), 100, 12.0, 0, *(ptr(t) for t in outs), stream_ptr(torch.device(DEV)))


def poisoned(F, N, B, C):
    """The six output tensors, every byte 0xFF."""
    shapes = (((F, N), torch.int32), ((F, B), torch.int32), ((F, B), torch.uint8), ((F, 101), torch.int64), ((F, 101), torch.int64), ((F, C), torch.int64))
    return [torch.full(s, -1 if t != torch.uint8 else 255, dtype=t, device=DEV) for s, t in shapes]


def test_poisoned_memory_growth_and_reuse(rule, orule, golden):
    """The library writes every output and reads nothing it has not written: over 0xFF-filled outputs and workspace a run gives
    the same bits; the context serves a small call, a large one (its workspace grows) and the small one again."""
    from shapemol_amd import evaluation as EV
    rng = np.random.default_rng(4)
    slots = orule.slots(golden["vocab"]["add_aromatic"])
    calls = []
    for sizes, F in (([5, 70, 3], 2), ([40] * 300 + [200] * 4, 3)):
        batch, off = batch_of(sizes)
        pos = np.stack([np.concatenate([chain(rng, n) for n in sizes]) for _ in range(F)])
        cls = rng.choice(15, pos.shape[:2], p=np.r_[0.1, 0.5, np.full(13, 0.4 / 13)])
        calls.append((F, off, dev(pos), dev(cls), O.evaluate(pos, cls, off, orule, slots)))
    first = None
    for k in (0, 1, 0, 0):
        F, off, pos, cls, exp = calls[k]
        outs = poisoned(F, pos.shape[1], len(off) - 1, 15)
        EV._debug_fill(torch.device(DEV), 0xFF)
        assert raw_run(F, off, pos, cls, rule, slots, outs) == 0
        outs[2] = outs[2].view(torch.bool)
        for key, t in zip(KEYS, outs):
            assert torch.equal(t.cpu(), torch.from_numpy(exp[key])), (k, key)
        if k == 0:
            first = first or outs
            assert all(torch.equal(a, b) for a, b in zip(first, outs))


def test_refusals_launch_nothing(rule, orule, golden):
    """A refused call returns an error with every output byte as it was: neither the memsets nor a kernel ran; the context then
    serves the next call.  The Python surface refuses classes outside the vocabulary on device tensors too."""
    from shapemol_amd import _lib, evaluate_geometry
    slots = orule.slots(golden["vocab"]["add_aromatic"])
    pos, cls = torch.zeros(1, 1100, 3, device=DEV), torch.ones(1, 1100, dtype=torch.int64, device=DEV)
    for off in ([0, 1025, 1100], [0, 50, 50, 1100], [1, 1100]):
        outs = poisoned(1, 1100, len(off) - 1, 15)
        assert raw_run(1, off, pos, cls, rule, slots, outs) == 1
        assert _lib.load().shapemol_last_error().decode().startswith("molecule evaluation:")
        torch.cuda.synchronize()
        assert all(bool((t.view(torch.uint8) == 255).all()) for t in outs)
    for bad in (15, -1):
        v = torch.ones(40, dtype=torch.int64, device=DEV)
        v[7] = bad
        with pytest.raises(ValueError, match="outside"):
            evaluate_geometry(torch.zeros(40, 3, device=DEV), v, np.zeros(40, np.int64), rule)
    with pytest.raises(ValueError, match="limit is 1024"):
        evaluate_geometry(pos[0], cls[0], np.zeros(1100, np.int64), rule)
    r = evaluate_geometry(torch.zeros(2, 3, device=DEV), torch.ones(2, dtype=torch.int64, device=DEV), np.zeros(2, np.int64), rule)
    assert r.nr_bonds.cpu().tolist() == [3, 3]                                  # two coincident carbons: a triple bond


def test_check_stability_and_evaluate_samples_agree(golden, rule):
    from shapemol_amd import check_stability, evaluate_geometry, evaluate_samples
    g = golden
    ids, rows, pos, cls, batch, off = by_mode(g, "add_aromatic")
    whole = evaluate_geometry(dev(pos), dev(cls), batch, rule, details=True)
    mols = [(pos[off[k]:off[k + 1]].astype(np.float64), cls[off[k]:off[k + 1]]) for k in range(len(ids))]
    samples = evaluate_samples(([p for p, _ in mols], [c for _, c in mols], "the rest of the tuple"), rule, details=True)
    for k in KEYS:
        assert torch.equal(getattr(whole, k), getattr(samples, k)), k
    assert samples.forms == whole.forms and samples.validity() == whole.validity()
    for hs in (False, True):
        tag = "hs" if hs else "nohs"
        for k, (p, c) in enumerate(mols):
            z = g["vocab"]["add_aromatic"][c]
            stable, n_stable, n, nr = check_stability(p, z, rule, hs=hs, return_nr_bonds=True)
            s = slice(g["off"][ids[k]], g["off"][ids[k] + 1])
            assert (stable, n_stable, n) == (bool(g[f"mol_stable_{tag}"][ids[k]]), int(g[f"n_stable_{tag}"][ids[k]]), len(c))
            assert np.array_equal(nr, g[f"nr_bonds_{tag}"][s])
    assert check_stability(torch.from_numpy(mols[3][0]).float().to(DEV), g["vocab"]["add_aromatic"][mols[3][1]], rule) == \
        (bool(g["mol_stable_nohs"][ids[3]]), int(g["n_stable_nohs"][ids[3]]), len(mols[3][1]))
