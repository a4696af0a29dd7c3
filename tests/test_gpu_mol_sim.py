"""The molecule similarity on the device (shapemol_amd.similarity, csrc/sm_mol_sim.h) against the
reference's stored results (tests/golden/mol_sim.npz) and the numpy oracle (tests/mol_sim_oracle.py, itself held to the
reference by tests/test_mol_sim_cpu.py).

Tolerances.  An integral: (n_terms + 16) * 2^-52 * sum |term| against the oracle (the float64 summation bound plus a few ulp
per exp); against the stored reference twice that, the oracle's own distance to the reference being bounded by the same
figure.  A score: exactly the stated IEEE expression of the device's own integrals.  get_rocs against the stored get_ROCS:
2e-7 -- the reference forms B = alpha^2 / (2 alpha) in float32, three roundings of 2^-24 each on alpha, the product and the
quotient, so B r^2 is off by at most 1.8e-7 relative; a term changes by B r^2 exp(-B r^2) <= 0.37 of that relative to the
largest term, and the Tanimoto ratio at most doubles it: 1.3e-7 (the common factor A cancels in the ratio).  The overlay:
O.OVERLAY_TOL, ten times the oracle's own disagreement between a case and its rigidly moved copy (measured by
test_mol_sim_cpu.py::test_overlay_tolerance), in frame invariance and against the oracle alike.  Only the self-consistency
test, which scores one pose twice, uses the fixed-pose bound of the score."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mol_sim_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    g = O.load_golden()
    P = len(g["kind"])
    sl = lambda off, m: slice(off[m], off[m + 1])  # noqa: E731
    g["A"] = [g["pos_a"][sl(g["off_a"], m)] for m in range(P)]
    g["B"] = [g["pos_b"][sl(g["off_b"], m)] for m in range(P)]
    for k in ("alpha", "p", "w"):
        g[f"{k}A"] = [g[f"{k}_a"][sl(g["off_a"], m)] for m in range(P)]
        g[f"{k}B"] = [g[f"{k}_b"][sl(g["off_b"], m)] for m in range(P)]
    return g


def cpu(t):
    return t.cpu().numpy()


def ieee_scores(metric, integ):
    saa, sbb, sab = integ[:, 0], integ[:, 1], integ[:, 2]
    return O.metric(metric, saa, sbb, sab)


def same_bits(x, y):
    return np.asarray(x, np.float64).tobytes() == np.asarray(y, np.float64).tobytes()


def check_integrals(integ, expected, what):
    """integ (P, 3) of the device against expected[p] = three (sum, sum |term|, terms) of the oracle."""
    worst = 0.0
    for p, three in enumerate(expected):
        for k, (s, sabs, n) in enumerate(three):
            err, b = abs(integ[p, k] - s), O.bound(n, sabs)
            assert err <= b, (what, p, k, integ[p, k], s, err, b)
            worst = max(worst, err / max(b, 1e-300))
    print(f"{what}: largest error / bound {worst:.3f}")


def test_shape_fixture_against_the_reference(golden):
    from shapemol_amd import shape_tanimoto
    g = golden
    r = shape_tanimoto(g["A"], g["B"], g["alphaA"], g["alphaB"], g["pA"], g["pB"], details=True, device=DEV)
    integ, score, flag = cpu(r.integrals), cpu(r.score), cpu(r.zero_denominator)
    assert set(r.forms) == {"wave"}
    exp = [(O.shape_integral(a, a, ua, va, ua, va), O.shape_integral(b, b, ub, vb, ub, vb), O.shape_integral(a, b, ua, va, ub, vb))
           for a, b, ua, va, ub, vb in zip(g["A"], g["B"], g["alphaA"], g["pA"], g["alphaB"], g["pB"])]
    check_integrals(integ, exp, "shape")
    for p, three in enumerate(exp):
        for k, key in enumerate(("vaa", "vbb", "vab")):
            assert abs(integ[p, k] - g[key][p]) <= 2 * O.bound(three[k][2], three[k][1]), (p, key)
    e, f = ieee_scores("tanimoto", integ)
    assert same_bits(score, e) and np.array_equal(flag, f)
    assert flag.tolist() == [k == "zero-prefactors" for k in g["kind"]] and np.isnan(score[flag]).all()
    for p, three in enumerate(exp):
        if not flag[p]:
            tb = O.tanimoto_bound(*(x[0] for x in three), *(O.bound(x[2], x[1]) for x in three))
            assert abs(score[p] - g["tanimoto"][p]) <= 2 * tb, (p, score[p], g["tanimoto"][p])
    under = [p for p, k in enumerate(g["kind"]) if k == "underflow"]
    assert (integ[under, 2] == 0).all() and (score[under] == 0).all()


def test_get_rocs_fixture(golden):
    from shapemol_amd import get_rocs
    g = golden
    score = cpu(get_rocs(g["A"], g["B"], device=DEV))
    assert score.dtype == np.float64 and np.abs(score - g["rocs"]).max() <= 2e-7
    for p in (14, 30):                                       # and the float64 oracle within the fixed-pose bound
        a, b = g["A"][p], g["B"][p]
        pa, pb = O.rocs_parameters(len(a)), O.rocs_parameters(len(b))
        three = (O.shape_integral(a, a, *pa, *pa), O.shape_integral(b, b, *pb, *pb), O.shape_integral(a, b, *pa, *pb))
        t = O.metric("tanimoto", *(x[0] for x in three))[0]
        assert abs(score[p] - t) <= O.tanimoto_bound(*(x[0] for x in three), *(O.bound(x[2], x[1]) for x in three))
    print(f"get_rocs against the stored get_ROCS: {np.abs(score - g['rocs']).max():.3e}")


@pytest.mark.parametrize("metric", ["carbo", "tanimoto"])
def test_esp_fixture_against_the_reference(golden, metric):
    from shapemol_amd import esp_similarity
    g = golden
    cA, cB = O.gaussint_terms()
    r = esp_similarity(g["A"], g["B"], g["wA"], g["wB"], (cA, -cB), metric=metric, details=True, device=DEV)
    integ, score, flag = cpu(r.integrals), cpu(r.score), cpu(r.zero_denominator)
    exp = [(O.esp_integral(a, a, wa, wa, cA, cB), O.esp_integral(b, b, wb, wb, cA, cB), O.esp_integral(a, b, wa, wb, cA, cB))
           for a, b, wa, wb in zip(g["A"], g["B"], g["wA"], g["wB"])]
    check_integrals(integ, exp, "esp")
    for p, three in enumerate(exp):
        for k, key in enumerate(("esp_aa", "esp_bb", "esp_ab")):
            assert abs(integ[p, k] - g[key][p]) <= 2 * O.bound(three[k][2], three[k][1]), (p, key)
    e, f = ieee_scores(metric, integ)
    assert same_bits(score, e) and np.array_equal(flag, f)
    assert flag.tolist() == [k == "zero-charges" and metric == "carbo" for k in g["kind"]]
    ok = ~flag
    assert np.abs(score[ok] - g[f"esp_{metric}"][ok]).max() <= 1e-9 and np.isnan(g[f"esp_{metric}"][flag]).all()


@pytest.fixture(scope="module")
def sized():
    """Molecules of 1, 2, 3, 63, 64, 65, 255 and 256 atoms in both sets, per-atom widths and prefactors, charges."""
    rng = np.random.default_rng(11)
    ns = (1, 2, 3, 63, 64, 65, 255, 256)
    mk = lambda: [O.walk(rng, n) + rng.uniform(-2, 2, 3) for n in ns]  # noqa: E731
    par = lambda lo, hi: [rng.uniform(lo, hi, n) for n in ns]  # noqa: E731
    return dict(ns=ns, A=mk(), B=mk(), alphaA=par(0.5, 1.2), alphaB=par(0.5, 1.2), pA=par(0.5, 1.0), pB=par(0.5, 1.0),
                wA=[0.4 * rng.standard_normal(n) for n in ns], wB=[0.4 * rng.standard_normal(n) for n in ns])


def test_all_pairs_of_every_size_both_forms(sized):
    """64 pairs over the sizes at which the form changes; then a workspace filled with 0xFF and the same bits again."""
    from shapemol_amd import shape_tanimoto, similarity
    s = sized
    r = shape_tanimoto(s["A"], s["B"], s["alphaA"], s["alphaB"], s["pA"], s["pB"], pairs="all", details=True, device=DEV)
    assert len(r.pairs) == 64
    assert r.forms == ["block" if max(s["ns"][a], s["ns"][b]) > 64 else "wave" for a, b in r.pairs.tolist()]
    integ, score = cpu(r.integrals), cpu(r.score)
    self_a = [O.shape_integral(a, a, u, v, u, v) for a, u, v in zip(s["A"], s["alphaA"], s["pA"])]
    self_b = [O.shape_integral(b, b, u, v, u, v) for b, u, v in zip(s["B"], s["alphaB"], s["pB"])]
    exp = [(self_a[a], self_b[b], O.shape_integral(s["A"][a], s["B"][b], s["alphaA"][a], s["pA"][a], s["alphaB"][b], s["pB"][b])) for a, b in r.pairs.tolist()]
    check_integrals(integ, exp, "shape, all sizes")
    assert same_bits(score, ieee_scores("tanimoto", integ)[0]) and not cpu(r.zero_denominator).any()
    similarity._debug_fill(DEV, 0xFF)
    again = shape_tanimoto(s["A"], s["B"], s["alphaA"], s["alphaB"], s["pA"], s["pB"], pairs="all", details=True, device=DEV)
    assert same_bits(cpu(again.integrals), integ) and same_bits(cpu(again.score), score)


def test_mixed_pair_lists_and_n_to_one(sized):
    """A few hundred pairs in random order over both forms equal the all-pairs call bit for bit; so do N-to-1 and a single pair."""
    from shapemol_amd import shape_tanimoto
    s = sized
    args = (s["A"], s["B"], s["alphaA"], s["alphaB"], s["pA"], s["pB"])
    full = cpu(shape_tanimoto(*args, pairs="all", details=True, device=DEV).integrals).reshape(8, 8, 3)
    pairs = np.random.default_rng(2).integers(0, 8, (300, 2))
    r = shape_tanimoto(*args, pairs=pairs, details=True, device=DEV)
    assert {"wave", "block"} == set(r.forms) and same_bits(cpu(r.integrals), full[pairs[:, 0], pairs[:, 1]])
    one = shape_tanimoto(s["A"], s["B"][5], s["alphaA"], s["alphaB"][5], s["pA"], s["pB"][5], details=True, device=DEV)
    assert one.pairs.tolist() == [[k, 0] for k in range(8)] and same_bits(cpu(one.integrals), full[:, 5])
    single = shape_tanimoto(s["A"][7], s["B"][0], s["alphaA"][7], s["alphaB"][0], s["pA"][7], s["pB"][0], details=True, device=DEV)
    assert same_bits(cpu(single.integrals)[0], full[7, 0])


def test_esp_sixteen_terms_every_size(sized):
    from shapemol_amd import esp_similarity
    s = sized
    rng = np.random.default_rng(4)
    cA, cB = rng.uniform(0.5, 20, 16), rng.uniform(0.001, 0.3, 16)
    pairs = np.array([[0, 0], [1, 2], [2, 1], [3, 4], [4, 4], [4, 5], [5, 3], [6, 7], [7, 6], [7, 7], [0, 7]])
    r = esp_similarity(s["A"], s["B"], s["wA"], s["wB"], (cA, -cB), metric="tanimoto", pairs=pairs, details=True, device=DEV)
    exp = [(O.esp_integral(s["A"][a], s["A"][a], s["wA"][a], s["wA"][a], cA, cB), O.esp_integral(s["B"][b], s["B"][b], s["wB"][b], s["wB"][b], cA, cB),
            O.esp_integral(s["A"][a], s["B"][b], s["wA"][a], s["wB"][b], cA, cB)) for a, b in pairs.tolist()]
    check_integrals(cpu(r.integrals), exp, "esp, 16 terms")
    assert same_bits(cpu(r.score), ieee_scores("tanimoto", cpu(r.integrals))[0])


# ---- the overlay ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    return O.overlay_cases()


@pytest.fixture(scope="module")
def oracle_overlays(cases):
    return {name: O.align(a, b, *O.rocs_parameters(len(a)), *O.rocs_parameters(len(b))) for name, (a, b) in cases.items()}


def run_overlay(As, Bs, **kw):
    from shapemol_amd import align_shapes
    r = align_shapes(As, Bs, device=DEV, **kw)
    return dict(tanimoto=cpu(r.tanimoto), integrals=cpu(r.integrals), start=cpu(r.start), rot=cpu(r.rotation), trans=cpu(r.translation),
                iterations=cpu(r.iterations), converged=cpu(r.converged), flag=cpu(r.zero_denominator), forms=r.forms,
                aligned=[cpu(x) for x in r.aligned])


@pytest.fixture(scope="module")
def device_overlays(cases):
    """Every case in one call: mixed forms in one pair list."""
    return run_overlay([a for a, _ in cases.values()], [b for _, b in cases.values()])


def score_bound(a, b):
    pa, pb = O.rocs_parameters(len(a)), O.rocs_parameters(len(b))
    three = (O.shape_integral(a, a, *pa, *pa), O.shape_integral(b, b, *pb, *pb), O.shape_integral(a, b, *pa, *pb))
    return O.tanimoto_bound(*(x[0] for x in three), *(O.bound(x[2], x[1]) for x in three))


def test_overlay_known_answers(cases, device_overlays):
    """A rigidly moved (and permuted) copy overlaid on the original: 1, 2, 3 .. 256 atoms, both forms."""
    d = device_overlays
    assert d["forms"] == ["block" if max(len(a), len(b)) > 64 else "wave" for a, b in cases.values()]
    for k, name in enumerate(cases):
        if name.startswith("copy"):
            print(f"{name}: 1 - T = {1 - d['tanimoto'][k]:.3e}, start {d['start'][k]}, {d['iterations'][k]} iterations")
            assert d["tanimoto"][k] >= 1 - 1e-9 and d["converged"][k] and not d["flag"][k], name


def test_overlay_is_self_consistent(cases, device_overlays):
    """The returned motion, applied on the host in float64 and scored by the fixed-pose entry, reproduces the returned score."""
    from shapemol_amd import get_rocs
    d = device_overlays
    moved = [O.apply(d["rot"][k], d["trans"][k], a) for k, (a, _) in enumerate(cases.values())]
    r = get_rocs(moved, [b for _, b in cases.values()], details=True, device=DEV)
    score = cpu(r.score)
    exact = 0
    for k, (name, (a, b)) in enumerate(cases.items()):
        R = d["rot"][k]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12, name
        assert np.abs(d["aligned"][k] - moved[k]).max() <= 1e-13 * (1 + np.abs(moved[k]).max()), name
        assert abs(score[k] - d["tanimoto"][k]) <= score_bound(moved[k], b), (name, score[k], d["tanimoto"][k])
        exact += score[k] == d["tanimoto"][k]
    print(f"bit-equal scores: {exact} of {len(cases)}")


def test_overlay_is_frame_invariant(cases, device_overlays):
    rng = np.random.default_rng(7)
    moved = run_overlay([O.moved(rng, a)[0] for a, _ in cases.values()], [b for _, b in cases.values()])
    diff = np.abs(moved["tanimoto"] - device_overlays["tanimoto"])
    print(f"largest difference between a case and its moved copy: {diff.max():.3e} (allowed {O.OVERLAY_TOL:.1e})")
    assert moved["converged"].all()
    assert (diff <= O.OVERLAY_TOL).all(), dict(zip(cases, diff))


def test_overlay_against_the_oracle(cases, device_overlays, oracle_overlays):
    d = device_overlays
    worst, compared = 0.0, 0
    for k, (name, (a, b)) in enumerate(cases.items()):
        o = oracle_overlays[name]
        worst = max(worst, abs(d["tanimoto"][k] - o["tanimoto"]))
        assert abs(d["tanimoto"][k] - o["tanimoto"]) <= O.OVERLAY_TOL, (name, d["tanimoto"][k], o["tanimoto"])
        s = np.sort(o["start_scores"])[::-1]
        if name.startswith("pair") and s[0] - s[1] > O.START_GAP:
            compared += 1
            assert d["start"][k] == o["start"], (name, d["start"][k], o["start"], o["start_scores"])
            assert np.abs(d["rot"][k] - o["rot"]).max() < 1e-6 and np.abs(d["trans"][k] - o["trans"]).max() < 1e-5, name
    print(f"largest difference to the oracle: {worst:.3e}; winning start compared in {compared} cases")
    assert compared == 9                                     # every two-molecule case


def test_overlay_poses_are_stationary(cases, device_overlays):
    d = device_overlays
    assert d["converged"].all() and (d["iterations"] <= O.ITER_CAP).all()
    for k, (name, (a, b)) in enumerate(cases.items()):
        gmax, scale = O.pose_gradient(d["aligned"][k], b, *O.rocs_parameters(len(a)), *O.rocs_parameters(len(b)))
        assert gmax <= O.STATIONARITY_MARGIN * O.GTOL * scale, (name, gmax, O.GTOL * scale)


def test_given_pose_is_a_floor():
    """include_given: never below the fixed-pose score of the pose as given -- a random pose, the optimum itself, far apart."""
    from shapemol_amd import get_rocs
    rng = np.random.default_rng(3)
    b = [O.walk_well_posed(rng, n) for n in (20, 23, 64, 70, 5)]
    a = [O.walk_well_posed(rng, 22) + 1.0, b[1].copy(), b[2] + 0.3, O.walk_well_posed(rng, 30) + 45.0, b[4][::-1].copy()]
    fixed = cpu(get_rocs(a, b, device=DEV))
    d = run_overlay(a, b, include_given=True)
    print("given:", fixed, "overlaid:", d["tanimoto"], "starts:", d["start"])
    assert (d["tanimoto"] >= fixed).all() and d["converged"].all()
    assert d["tanimoto"][1] >= fixed[1] == 1.0 and d["tanimoto"][4] >= 1 - 1e-9 and fixed[3] == 0.0
    without = run_overlay(a, b)
    assert (d["tanimoto"] >= without["tanimoto"] - O.OVERLAY_TOL).all()
    for k in np.flatnonzero((d["start"] == 4) & (d["iterations"] == 0)):          # the pose as given, kept: the identity, exactly
        assert (d["rot"][k] == np.eye(3)).all() and (d["trans"][k] == 0).all()


def test_overlay_is_the_same_in_every_run(cases, device_overlays):
    from shapemol_amd import similarity
    similarity._debug_fill(DEV, 0xFF)
    again = run_overlay([a for a, _ in cases.values()], [b for _, b in cases.values()])
    for key in ("tanimoto", "integrals", "rot", "trans"):
        assert same_bits(again[key], device_overlays[key]), key
    assert np.array_equal(again["start"], device_overlays["start"]) and np.array_equal(again["iterations"], device_overlays["iterations"])
    assert all(same_bits(x, y) for x, y in zip(again["aligned"], device_overlays["aligned"]))


def test_iteration_cap_is_reported(cases):
    a, b = cases["pair22x27"]
    d = run_overlay(a, b, max_iter=2)
    assert not d["converged"][0] and d["iterations"][0] == 2 and 0 < d["tanimoto"][0] < 1


def test_positions_that_are_not_finite_never_converge(cases):
    """They are not refused (they live on the device): the score is NaN and no start reports converged."""
    a, b = cases["pair12x9"]
    bad = a.copy()
    bad[3, 1] = np.nan
    for kw in ({}, {"include_given": True}):
        d = run_overlay([bad, a], [b, b], **kw)
        assert np.isnan(d["tanimoto"][0]) and not d["converged"][0] and d["iterations"][0] == 0
        assert d["converged"][1] and 0 < d["tanimoto"][1] < 1


def test_similarity_to_condition():
    """The script's three figures over two groups; a sample that cannot be scored gets -1 and stays out of them."""
    from shapemol_amd import align_shapes, similarity_to_condition
    rng = np.random.default_rng(9)
    conds = [O.walk_well_posed(rng, 24), O.walk_well_posed(rng, 70)]
    groups = [[O.walk_well_posed(rng, int(n)).astype(np.float32) for n in rng.integers(18, 30, 6)] for _ in conds]
    groups[0][2] = np.zeros((0, 3), np.float32)
    groups[1][4] = np.full((5, 3), np.nan, np.float32)
    r = similarity_to_condition([(g, [np.zeros(len(p), np.int64) for p in g]) for g in groups], conds, device=DEV)
    assert r["scores"][0][2] == -1 and r["scores"][1][4] == -1 and r["aligned_positions"][0][2] is None
    means, maxima = [], []
    for g, c, s, al in zip(groups, conds, r["scores"], r["aligned_positions"]):
        keep = [k for k, p in enumerate(g) if len(p) and np.isfinite(p).all()]
        d = align_shapes([g[k] for k in keep], c, device=DEV)
        assert [s[k] for k in keep] == cpu(d.tanimoto).tolist() and all(0 < s[k] <= 1 for k in keep)
        assert all(same_bits(al[k], cpu(x)) for k, x in zip(keep, d.aligned))
        means.append(np.mean([x for x in s if x >= 0])); maxima.append(np.max([x for x in s if x >= 0]))
    assert r["avg_ref_shaep_rocssims"] == np.mean(means) and r["std_ref_shaep_rocssims"] == np.std(means)
    assert r["avg_ref_max_shaep_rocssims"] == np.mean(maxima)
    one = similarity_to_condition(groups[0], conds[0], device=DEV)
    assert one["scores"] == r["scores"][0] and one["std_ref_shaep_rocssims"] == 0.0
