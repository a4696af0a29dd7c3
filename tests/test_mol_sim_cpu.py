"""The molecule similarity without a GPU: the numpy oracle (tests/mol_sim_oracle.py) against the
reference's own results stored in tests/golden/mol_sim.npz (written by tests/golden/make_golden_mol_sim.py), the conditions
that make the fixture and the overlay cases worth testing against, the measurement behind the overlay tolerance, and the host
side of shapemol_amd.similarity: the refusals, the ABI names and the host plan (through tests/mol_sim_probe.cpp, a stand-alone
host program built with the address and undefined-behaviour sanitizers)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mol_sim_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return O.load_golden()


def pair_of(g, m):
    sa, sb = slice(g["off_a"][m], g["off_a"][m + 1]), slice(g["off_b"][m], g["off_b"][m + 1])
    return {"a": g["pos_a"][sa], "b": g["pos_b"][sb], **{k: g[k][sa if k.endswith("_a") else sb] for k in ("alpha_a", "p_a", "alpha_b", "p_b", "w_a", "w_b")}}


def three(fn, q, keys_a, keys_b):
    """fn over (a, a), (b, b), (a, b) -> three (sum, sum |term|, terms)."""
    A, B = [q[k] for k in keys_a], [q[k] for k in keys_b]
    return fn(q["a"], q["a"], *A, *A), fn(q["b"], q["b"], *B, *B), fn(q["a"], q["b"], *A, *B)


def test_oracle_meets_the_reference_within_the_summation_bound(golden):
    g = golden
    cA, cB = O.gaussint_terms()
    worst = 0.0
    for m in range(len(g["kind"])):
        q = pair_of(g, m)
        shape = three(lambda x, y, ax, px, ay, py: O.shape_integral(x, y, ax, px, ay, py), q, ("alpha_a", "p_a"), ("alpha_b", "p_b"))
        esp = three(lambda x, y, wx, wy: O.esp_integral(x, y, wx, wy, cA, cB), q, ("w_a",), ("w_b",))
        for (s, sabs, n), key in zip(shape + esp, ("vaa", "vbb", "vab", "esp_aa", "esp_bb", "esp_ab")):
            assert abs(s - g[key][m]) <= O.bound(n, sabs), (m, key, g["kind"][m], s, g[key][m])
            worst = max(worst, abs(s - g[key][m]) / max(O.bound(n, sabs), 1e-300))
        # the scores are the stated expressions; a zero denominator is flagged where the reference gives NaN or raises
        t, flag = O.metric("tanimoto", *(x[0] for x in shape))
        if np.isnan(g["tanimoto"][m]):
            assert flag and np.isnan(t) and g["kind"][m] == "zero-prefactors"
        else:
            assert not flag and abs(t - g["tanimoto"][m]) <= O.tanimoto_bound(*(x[0] for x in shape), *(O.bound(x[2], x[1]) for x in shape))
        for name in ("carbo", "tanimoto"):
            e, flag = O.metric(name, *(x[0] for x in esp))
            ref = g[f"esp_{name}"][m]
            if g["kind"][m] == "zero-charges" and name == "carbo":             # sqrt(S_aa * 0): SimilarityMetric raises
                assert np.isnan(ref) and flag and np.isnan(e)
            else:
                assert not flag and abs(e - ref) <= 1e-9 * abs(ref)            # charges of mixed sign cancel: no first-order bound is tight
    print(f"largest error / bound: {worst:.3f}")


def test_float32_coefficients_are_the_whole_gap_to_get_rocs(golden):
    g = golden
    gap = 0.0
    for m in range(len(g["kind"])):
        q = pair_of(g, m)
        q.update(zip(("alpha_a", "p_a"), O.rocs_parameters(len(q["a"]))), **dict(zip(("alpha_b", "p_b"), O.rocs_parameters(len(q["b"])))))
        f32 = three(lambda x, y, ax, px, ay, py: O.shape_integral(x, y, ax, px, ay, py, float32=True), q, ("alpha_a", "p_a"), ("alpha_b", "p_b"))
        f64 = three(lambda x, y, ax, px, ay, py: O.shape_integral(x, y, ax, px, ay, py), q, ("alpha_a", "p_a"), ("alpha_b", "p_b"))
        t32 = O.metric("tanimoto", *(x[0] for x in f32))[0]
        t64 = O.metric("tanimoto", *(x[0] for x in f64))[0]
        assert abs(t32 - g["rocs"][m]) <= O.tanimoto_bound(*(x[0] for x in f32), *(O.bound(x[2], x[1]) for x in f32)), (m, t32, g["rocs"][m])
        gap = max(gap, abs(t64 - g["rocs"][m]))
    print(f"float64 coefficients against get_ROCS: {gap:.3e}")
    assert 0 < gap < 2e-7                  # the float32 rounding of alpha / (2 alpha) * r2 in the exponent; see test_gpu_mol_sim.py


def test_fixture_conditions(golden):
    g = golden
    na, nb = np.diff(g["off_a"]), np.diff(g["off_b"])
    assert len(na) == 40 and min(na.min(), nb.min()) == 1 and max(na.max(), nb.max()) == 64 and g["pos_a"].dtype == np.float64
    kinds = g["kind"].tolist()
    assert {"walk", "identical", "coincident", "far", "underflow", "zero-prefactors", "zero-charges"} == set(kinds)
    for m, k in enumerate(kinds):
        q = pair_of(g, m)
        if k == "identical":
            assert np.array_equal(q["a"], q["b"]) and g["rocs"][m] == 1.0
        if k == "coincident":
            assert (O.r2_of(q["a"], q["a"])[0][np.triu_indices(len(q["a"]), 1)] == 0).any() and (O.r2_of(q["a"], q["b"])[0] == 0).any()
        if k == "far":
            assert 0 < g["vab"][m] < 1e-12 and g["vab"][m] > 1e-300 and max(na[m], nb[m]) <= 25
        if k == "underflow":
            assert g["vab"][m] == 0.0 and g["tanimoto"][m] == 0.0 and max(na[m], nb[m]) <= 25
    assert (g["w_a"] > 0).any() and (g["w_a"] < 0).any() and (g["esp_ab"] < 0).any() and (g["esp_ab"] > 0).any()
    cA, cB = O.gaussint_terms()
    assert len(cA) == 9 and (cB > 0).all() and (cA > 0).all()          # GaussInt's b are negative; the library's B are -b


@pytest.fixture(scope="module")
def overlays():
    """The oracle on every overlay case and on a rigidly moved copy of it: name -> (a, b, result, result of the moved copy)."""
    rng = np.random.default_rng(7)
    out = {}
    for name, (a, b) in O.overlay_cases().items():
        pa, pb = O.rocs_parameters(len(a)), O.rocs_parameters(len(b))
        out[name] = (a, b, O.align(a, b, *pa, *pb), O.align(O.moved(rng, a)[0], b, *pa, *pb))
    return out


def test_overlay_cases_are_well_posed(overlays):
    sizes = set()
    for name, (a, b, r, _) in overlays.items():
        sizes |= {len(a), len(b)}
        for mol in (a, b):
            if len(mol) >= 3:                                  # 1 and 2 atoms: symmetric about every principal frame
                m = O.moments(mol)
                assert m[0] > 0 and m[1] >= 1.2 * m[0] and m[2] >= 1.2 * m[1], (name, m)
    assert {1, 2, 3, 63, 64, 65, 255, 256} <= sizes
    compared = [n for n, (_, _, r, _) in overlays.items() if n.startswith("pair") and start_is_compared(r)]
    print("winning start compared in:", compared)
    assert compared == [n for n in overlays if n.startswith("pair")] and len(compared) == 9 and O.START_GAP == 100 * O.OVERLAY_TOL


def start_is_compared(r):
    s = np.sort(r["start_scores"])[::-1]
    return bool(s[0] - s[1] > O.START_GAP)


def test_overlay_tolerance(overlays):
    """The measurement behind OVERLAY_TOL: the oracle's own largest disagreement between a case and its rigidly moved copy."""
    measured = max(abs(r["tanimoto"] - r2["tanimoto"]) for _, _, r, r2 in overlays.values())
    print(f"largest disagreement between a case and its moved copy: {measured!r}; recorded {O.OVERLAY_MEASURED!r}; allowed {O.OVERLAY_TOL!r}")
    assert measured <= O.OVERLAY_MEASURED + 2.0 ** -53          # the recorded figure, give or take one step of a score near 1
    assert O.OVERLAY_TOL == 10 * O.OVERLAY_MEASURED


def test_oracle_overlays_converge_to_stationary_poses(overlays):
    for name, (a, b, r, r2) in overlays.items():
        pa, pb = O.rocs_parameters(len(a)), O.rocs_parameters(len(b))
        for x in (r, r2):
            assert x["converged"] and x["iterations"] <= O.ITER_CAP, name
            assert abs(np.linalg.det(x["rot"]) - 1) < 1e-12 and np.abs(x["rot"] @ x["rot"].T - np.eye(3)).max() < 1e-12
        gmax, scale = O.pose_gradient(r["aligned"], b, *pa, *pb)
        assert gmax <= O.STATIONARITY_MARGIN * O.GTOL * scale, (name, gmax, scale)
        if name.startswith("copy"):
            assert r["tanimoto"] >= 1 - 1e-9 and r2["tanimoto"] >= 1 - 1e-9, (name, r["tanimoto"])
            assert r["iterations"] == 0                        # the principal-frame start is exact; the optimiser does not leave it


def test_oracle_given_pose_is_a_floor():
    rng = np.random.default_rng(3)
    a, b = O.walk_well_posed(rng, 20), O.walk_well_posed(rng, 23)
    pa, pb = O.rocs_parameters(20), O.rocs_parameters(23)
    for shift in (0.0, 2.0, 40.0):
        r = O.align(a + shift, b, *pa, *pb, include_given=True)
        fixed = O.metric("tanimoto", r["s_aa"], r["s_bb"], O.shape_integral(a + shift, b, *pa, *pb)[0])[0]
        assert r["tanimoto"] >= fixed
    r = O.align(b.copy(), b, *pb, *pb, include_given=True)
    assert r["tanimoto"] == 1.0 or r["tanimoto"] >= O.metric("tanimoto", r["s_aa"], r["s_bb"], O.shape_integral(b, b, *pb, *pb)[0])[0]


# ---- the host side of the package ----------------------------------------------------------------------------------------------
def test_abi_names_are_exported_and_bound():
    from shapemol_amd import _lib
    names = ("shapemol_sim_sizes", "shapemol_sim_check", "shapemol_sim_create", "shapemol_sim_destroy", "shapemol_sim_score", "shapemol_sim_align",
             "shapemol_sim_debug_fill")
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "shapemol_hip.h")).read()
    for n in names:
        assert n in _lib.EXPORTS and getattr(lib, n).argtypes is not None and f" {n}(" in header
    assert len(lib.shapemol_sim_score.argtypes) == 21 and len(lib.shapemol_sim_align.argtypes) == 22 and len(lib.shapemol_sim_check.argtypes) == 15
    assert lib.shapemol_abi_version() == _lib.ABI_VERSION


def test_limits_match_the_library():
    from shapemol_amd import similarity as S
    z = S.sizes()
    assert tuple(z) == (O.WAVE_ATOMS, O.MAX_ATOMS, O.MAX_TERMS, O.MAX_STARTS, O.MAX_ITER, O.MAX_PAIRS)
    assert S.GIVEN_START == z.max_starts - 1


def test_refusals_need_no_device():
    from shapemol_amd import align_shapes, esp_similarity, get_rocs, shape_tanimoto
    a, b = np.zeros((5, 3)), np.ones((4, 3))
    coef = O.gaussint_terms()
    coef = (coef[0], -coef[1])
    for kw in (dict(c1=np.zeros((257, 3))), dict(c2=np.zeros((0, 3))), dict(c1=np.zeros((5, 2))), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=np.nan),
               dict(prefactor=np.inf), dict(pairs=np.array([[0, 1]])), dict(pairs=np.array([[-1, 0]])), dict(pairs=np.zeros((0, 2), np.int64)),
               dict(pairs=np.array([[0.0, 0.0]])), dict(pairs="some"), dict(c1=[a, a, a], c2=[b, b])):
        args = dict(dict(c1=a, c2=b, prefactor=0.8, alpha=0.81, pairs=None), **kw)
        for fn in (get_rocs, align_shapes):
            with pytest.raises(ValueError):
                fn(args["c1"], args["c2"], args["prefactor"], args["alpha"], pairs=args["pairs"])
    with pytest.raises(ValueError, match="limit is 256"):
        get_rocs(np.zeros((300, 3)), b)
    with pytest.raises(ValueError, match="no atoms"):
        get_rocs([a, np.zeros((0, 3))], b)
    with pytest.raises(ValueError, match="per-atom parameters"):
        shape_tanimoto(a, b, np.ones(4), np.ones(4), 0.8, 0.8)
    w1, w2 = np.ones(5), np.ones(4)
    with pytest.raises(ValueError, match="Unknown metric"):
        esp_similarity(a, b, w1, w2, coef, metric="cosine")
    with pytest.raises(ValueError, match="16"):
        esp_similarity(a, b, w1, w2, (np.ones(17), -np.ones(17)))
    with pytest.raises(ValueError, match="not finite"):
        esp_similarity(a, b, w1, w2, (np.ones(3), np.array([-1.0, np.nan, -1.0])))
    with pytest.raises(ValueError, match="charge"):
        esp_similarity(a, b, np.array([1, 1, np.inf, 1, 1.0]), w2, coef)
    with pytest.raises(ValueError):
        esp_similarity(a, b, w1, w2, (np.ones(3), -np.ones(4)))
    for kw in (dict(max_iter=-1), dict(max_iter=10001), dict(gtol=-1.0), dict(gtol=np.nan)):
        with pytest.raises(ValueError):
            align_shapes(a, b, **kw)


def test_no_cpu_path():
    from shapemol_amd import align_shapes, get_rocs
    for fn in (get_rocs, align_shapes):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(np.zeros((2, 3)), np.zeros((3, 3)), device="cpu")


def test_unscorable_samples_get_minus_one_without_a_device():
    from shapemol_amd import similarity_to_condition
    cond = np.zeros((4, 3))
    bad = [np.zeros((0, 3)), np.full((3, 3), np.nan), np.zeros((257, 3)), None]
    r = similarity_to_condition(bad, cond)
    assert r["scores"] == [-1.0] * 4 and r["aligned_positions"] == [None] * 4 and np.isnan(r["avg_ref_shaep_rocssims"])
    r = similarity_to_condition((bad, [np.zeros(0)] * 4, "driver"), cond)           # the sampling driver's tuple
    assert r["scores"] == [-1.0] * 4
    r = similarity_to_condition([bad, [np.zeros(0)] * 4], cond)                     # the same as a list, as evaluate_samples takes it
    assert r["scores"] == [-1.0] * 4
    r = similarity_to_condition([np.zeros((0, 3)), np.full((2, 3), np.inf)], cond)  # two samples, not a driver result
    assert r["scores"] == [-1.0] * 2
    r = similarity_to_condition([bad, bad[:2]], [cond, cond])
    assert r["scores"] == [[-1.0] * 4, [-1.0] * 2]
    with pytest.raises(ValueError):
        similarity_to_condition([bad], [cond, cond])
    with pytest.raises(ValueError):
        similarity_to_condition(bad, np.zeros((0, 3)))


# ---- the host plan, through a stand-alone program -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("mol_sim_probe") / "mol_sim_probe")
    r = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "mol_sim_probe.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(mode, na, nb, pairs, bad=None):
        args = [mode, len(na), *na, len(nb), *nb, len(pairs), *[x for p in pairs for x in p]] + ([bad] if bad else [])
        r = subprocess.run([exe] + [str(x) for x in args], capture_output=True, text=True)
        assert r.stderr == "", r.stderr[-2000:]                       # the sanitizers report nothing
        lines = [ln.split() for ln in r.stdout.splitlines()]
        if r.returncode:
            assert r.returncode == 1 and lines[0][0] == "error"
            return " ".join(lines[0][1:])
        return dict(pair=np.array([ln[1:] for ln in lines if ln[0] == "pair"], np.int64),
                    list={int(ln[1]): [int(x) for x in ln[2:]] for ln in lines if ln[0] == "list"},
                    aligned=int([ln for ln in lines if ln[0] == "aligned"][0][1]),
                    job=np.array([ln[1:] for ln in lines if ln[0] == "job"], np.int64))
    return run


def test_plan_puts_pairs_into_the_right_form(probe):
    na, nb = [1, 63, 64, 65, 256], [64, 65, 2]
    pairs = [(0, 0), (1, 0), (2, 0), (3, 0), (2, 1), (4, 2), (0, 2), (2, 2)]
    p = probe(0, na, nb, pairs)
    assert p["pair"][:, 1:3].tolist() == [list(x) for x in pairs]
    assert p["pair"][:, 3].tolist() == [0, 0, 0, 1, 1, 1, 0, 0]       # 64 and 64 atoms: a wave; 65 on either side: a workgroup
    assert p["list"][0] == [0, 1, 2, 6, 7] and p["list"][1] == [3, 4, 5]
    sizes = [na[a] for a, _ in pairs]
    assert p["pair"][:, 4].tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist() and p["aligned"] == sum(sizes)
    # the jobs of an overlay with include_given: every molecule's self overlap once, two cross integrals per pair, each in the
    # form of its own sizes, atoms inside their sets, output slots distinct and dense
    j = p["job"]
    off_a, off_b = np.concatenate([[0], np.cumsum(na)]), np.concatenate([[0], np.cumsum(nb)])
    assert len(j) == len(na) + len(nb) + 2 * len(pairs) and sorted(j[:, 10].tolist()) == list(range(len(j)))
    for stage, form, xs, xo, xp, xn, ys, yo, yp, yn, out in j.tolist():
        assert form == int(max(xn, yn) > 64) and 1 <= xn <= 256 and 1 <= yn <= 256
        assert xp + xn <= (off_b if xs == 1 else off_a)[-1] and yp + yn <= (off_b if ys == 1 else off_a)[-1]
        if stage == 0:
            assert (xs, xo, xp, xn) == (ys, yo, yp, yn) and out < len(na) + len(nb) and xo == (off_b if xs else off_a)[out - (len(na) if xs else 0)]
        else:
            k = (out - len(na) - len(nb)) % len(pairs)
            assert ys == 1 and (xp, xn, yo, yn) == (off_a[pairs[k][0]], na[pairs[k][0]], off_b[pairs[k][1]], nb[pairs[k][1]])
            assert (xs, xo) == ((2, p["pair"][k, 4]) if out < len(na) + len(nb) + len(pairs) else (0, xp))


def test_plan_refusals(probe):
    assert "limit is 256" in probe(0, [5, 257], [3], [(0, 0)])
    assert "no atoms" in probe(0, [5], [3, 0], [(0, 0)])
    assert "set a needs" in probe(0, [], [3], [(0, 0)])
    assert "pairs" in probe(0, [5], [3], [])
    assert "names molecule 2 of set a" in probe(0, [5, 4], [3], [(2, 0)])
    assert "names molecule -1 of set b" in probe(0, [5, 4], [3], [(1, -1)])
    assert "width" in probe(0, [5], [3], [(0, 0)], "alpha") and "prefactor" in probe(0, [5], [3], [(0, 0)], "nan")
    assert "charge" in probe(1, [5], [3], [(0, 0)], "nan") and "term 2" in probe(1, [5], [3], [(0, 0)], "term")
    assert "Gaussian terms" in probe(1, [5], [3], [(0, 0)], "terms") and "unknown mode" in probe(2, [5], [3], [(0, 0)])
    p = probe(1, [5, 70], [3], [(0, 0), (1, 0)])
    assert p["pair"][:, 3].tolist() == [0, 1]
