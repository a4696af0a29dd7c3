"""The geometry scores without a GPU: the numpy oracle (tests/mol_eval_oracle.py) against the reference's
own results stored in tests/golden/mol_eval.npz (written by tests/golden/make_golden_mol_eval.py), the conditions that make the
fixture worth testing against, and the host side of shapemol_amd.evaluation: the rule's JSON, the refusals, the ABI names and
the host plan's two launch forms (through tests/mol_eval_probe.cpp, a stand-alone host program built with the address and
undefined-behaviour sanitizers)."""
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
import mol_eval_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return O.load_golden()


@pytest.fixture(scope="module")
def oracle_results(golden):
    """The oracle on every fixture molecule, one call per molecule: {hs: [dict, ...]}."""
    g, rule = golden, O.Rule.load()
    res = {}
    for hs in (False, True):
        res[hs] = []
        for m in range(len(g["off"]) - 1):
            s = slice(g["off"][m], g["off"][m + 1])
            slots = rule.slots(g["vocab"][O.MODES[g["mode"][m]]])
            res[hs].append(O.evaluate(g["pos"][None, s], g["classes"][None, s], [0, s.stop - s.start], rule, slots, hs=hs))
    return res


def test_oracle_reproduces_the_reference_exactly(golden, oracle_results):
    g = golden
    for hs, tag in ((False, "nohs"), (True, "hs")):
        r = oracle_results[hs]
        assert np.array_equal(np.concatenate([x["nr_bonds"][0] for x in r]), g[f"nr_bonds_{tag}"])
        assert np.array_equal(np.array([x["n_stable_atoms"][0, 0] for x in r]), g[f"n_stable_{tag}"])
        assert np.array_equal(np.array([x["mol_stable"][0, 0] for x in r]), g[f"mol_stable_{tag}"])
    r = oracle_results[False]
    prof = O.profile(sum(x["hist_cc"][0] for x in r), sum(x["hist_all"][0] for x in r))
    emp = {k: g[f"empirical_{k}"] for k in prof}
    metrics = O.jsd(emp, prof)
    for k in prof:
        assert np.array_equal(g[f"bins_{k}"], {"CC_2A": O.CC_BINS, "All_12A": O.ALL_BINS}[k])
        assert prof[k].tobytes() == g[f"profile_{k}"].tobytes()                        # bit-equal
        assert np.float64(metrics[f"JSD_{k}"]).tobytes() == g[f"jsd_{k}"].tobytes()


def test_fixture_conditions(golden, oracle_results):
    g, r = golden, oracle_results[False]
    n = np.diff(g["off"])
    assert len(n) == 40 and n.min() == 1 and n.max() == 40 and g["pos"].dtype == np.float32
    assert set(g["mode"].tolist()) == {0, 1, 2}
    assert set().union(*(x["orders"] for x in r)) == {0, 1, 2, 3}
    assert g["mol_stable_nohs"].any() and not g["mol_stable_nohs"].all()
    frac = g["n_stable_nohs"].sum() / n.sum()
    print(f"stable atoms: {frac:.3f}")
    assert 0.1 <= frac <= 0.9
    assert sum(x["hist_cc"][0] for x in r).sum() > 0 and sum(x["hist_all"][0] for x in r).sum() > 0
    rule = O.Rule.load()
    beyond_cc = beyond_all = nan = zero = 0
    for m in range(len(n)):
        s = slice(g["off"][m], g["off"][m + 1])
        d = O.distances(g["pos"][s])
        iu = np.triu_indices(n[m], 1)
        z = g["vocab"][O.MODES[g["mode"][m]]][g["classes"][s]]
        cc = (z[iu[0]] == 6) & (z[iu[1]] == 6)
        with np.errstate(invalid="ignore"):
            beyond_cc += int((d[iu][cc] >= 2).sum())
            beyond_all += int((d[iu] >= 12).sum())
        nan += int(np.isnan(d[iu]).sum())
        zero += int((d[iu] == 0).sum())
    assert beyond_cc > 0 and beyond_all > 0 and nan > 0 and zero > 0
    assert (rule.bonds == -1).any()


def test_rule_round_trips_through_json(tmp_path):
    from shapemol_amd import StabilityRule
    rule = StabilityRule.from_json(O.RULE_JSON)
    ref = O.Rule.load()
    assert rule.elements.dtype == np.float64 and rule.bonds1.dtype == np.float64 and rule.allowed_bonds.dtype == np.float64
    assert rule.elements.tolist() == [1, 6, 7, 8, 9, 15, 16, 17, 35, 53]
    assert np.array_equal(rule.thresholds(), ref.thresholds()) and np.array_equal(rule.allowed_bonds, ref.allowed)
    assert rule.thresholds()[1, 0, 0] == -1 + 5                       # a -1 entry stays a number
    path = str(tmp_path / "rule.json")
    rule.to_json(path)
    again = StabilityRule.from_json(path)
    for k in ("elements", "bonds1", "bonds2", "bonds3", "margins", "allowed_bonds"):
        assert np.array_equal(getattr(rule, k), getattr(again, k))
    assert rule.slot_of([6, 1, 53]).tolist() == [1, 0, 9]
    with pytest.raises(ValueError, match="34"):
        rule.slot_of([6, 34])
    with pytest.raises(ValueError):
        StabilityRule([1, 6], np.zeros((2, 3)), np.zeros((2, 2)), np.zeros((2, 2)), [1, 2, 3], [1, 4])
    with pytest.raises(ValueError):
        StabilityRule([6, 6], np.zeros((2, 2)), np.zeros((2, 2)), np.zeros((2, 2)), [1, 2, 3], [4, 4])


def test_class_tables():
    from shapemol_amd import StabilityRule
    from shapemol_amd.evaluation import class_table
    rule = StabilityRule.from_json(O.RULE_JSON)
    assert [len(class_table(rule, m)) for m in O.MODES] == [10, 15, 23]
    t = class_table(rule, "add_aromatic", 18)
    assert t[:3].tolist() == [0, 1, 1] and t[15:].tolist() == [1, 1, 1]          # past the table: carbon
    for kw in (dict(mode="basic", num_classes=11), dict(mode="full", num_classes=24), dict(mode="add_aromatic", num_classes=14), dict(mode="nope")):
        with pytest.raises(ValueError):
            class_table(rule, **kw)
    few = StabilityRule([1, 6], np.full((2, 2), 100.0), np.full((2, 2), -1.0), np.full((2, 2), -1.0), [10, 5, 3], [1, 4])
    with pytest.raises(ValueError, match="atomic number"):                       # a class whose element the rule lacks
        class_table(few, "basic")


def test_limits_match_the_library():
    from shapemol_amd import evaluation as EV
    z = EV.sizes()
    assert tuple(z) == (O.WAVE_ATOMS, O.MAX_ATOMS, O.MAX_ELEMENTS, O.MAX_CLASSES, O.MAX_EDGES, O.THREADS)
    assert z.max_atoms % z.threads == 0 and z.threads % z.wave_atoms == 0
    # the LDS of the block form: the staged molecule, the thresholds, two sets of edges and counts, far below 64 KiB
    assert 25 * z.max_atoms + 24 * z.max_elements ** 2 + 2 * 12 * (z.max_edges + 1) < 48 * 1024


def test_refusals_need_no_device():
    from shapemol_amd import StabilityRule, check_stability, evaluate_geometry, evaluate_samples, evaluate_trajectory
    rule = StabilityRule.from_json(O.RULE_JSON)
    pos, v, batch = np.zeros((5, 3), np.float32), np.array([1, 1, 3, 5, 0]), np.array([0, 0, 0, 1, 1])
    big = np.zeros((1025, 3), np.float32)
    bad = [
        dict(pos=big, v=np.ones(1025, np.int64), batch=np.zeros(1025, np.int64)),                       # 1025 atoms
        dict(batch=np.array([0, 0, 0, 2, 2])),                                                          # molecule 1 is empty
        dict(batch=np.array([1, 1, 1, 2, 2])),                                                          # does not start at 0
        dict(batch=np.array([0, 1, 0, 1, 1])),                                                          # not packed
        dict(batch=np.array([0, 0, 0, 1])),                                                             # length
        dict(v=np.array([1, 1, 3, 15, 0])),                                                             # class outside add_aromatic
        dict(v=np.array([1, 1, -1, 5, 0])),
        dict(v=np.array([1, 1, 3, 10, 0]), mode="basic"),
        dict(num_classes=33),                                                                           # C <= 32
        dict(cc_bins=np.linspace(0, 2, 256)),                                                           # 255 edges
        dict(all_bins=np.linspace(0, 12, 256)),
        dict(all_bins=np.array([0.0, 2.0, 1.0])),                                                       # not ascending
        dict(cc_bins=np.array([0.0, np.nan])),
        dict(mode="aromatic"),
    ]
    for kw in bad:
        args = dict(dict(pos=pos, v=v, batch=batch), **kw)
        with pytest.raises(ValueError):
            evaluate_geometry(args.pop("pos"), args.pop("v"), args.pop("batch"), rule, **args)
    z17 = [1, 6, 7, 8, 9, 15, 16, 17, 35, 53, 2, 3, 4, 5, 10, 11, 12]
    wide = StabilityRule(z17, np.full((17, 17), 100.0), np.full((17, 17), -1.0), np.full((17, 17), -1.0), [10, 5, 3], [1] * 17)
    with pytest.raises(ValueError, match="16"):
        evaluate_geometry(pos, v, batch, wide, mode="basic")
    with pytest.raises(ValueError, match="limit is 1024"):
        check_stability(big, np.full(1025, 6), rule)
    with pytest.raises(ValueError, match="atomic number"):
        check_stability(pos, [6, 6, 6, 34, 6], rule)
    with pytest.raises(ValueError):
        evaluate_trajectory([pos, pos], [v], batch, rule)                                               # frames differ
    with pytest.raises(ValueError):
        evaluate_samples(([], []), rule)
    with pytest.raises(ValueError, match="no atoms"):
        evaluate_samples(([pos, np.zeros((0, 3))], [v, np.zeros(0, np.int64)]), rule)
    with pytest.raises(TypeError):
        evaluate_geometry(pos, v.astype(np.float32), batch, rule)


def test_no_cpu_path():
    from shapemol_amd import StabilityRule, evaluate_geometry
    rule = StabilityRule.from_json(O.RULE_JSON)
    with pytest.raises(RuntimeError, match="no CPU path"):
        evaluate_geometry(np.zeros((2, 3), np.float32), np.array([1, 1]), np.array([0, 0]), rule, device="cpu")


def test_abi_names_are_exported_and_bound():
    from shapemol_amd import _lib
    names = ("shapemol_eval_sizes", "shapemol_eval_check", "shapemol_eval_create", "shapemol_eval_destroy", "shapemol_eval_run",
             "shapemol_eval_debug_fill")
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "shapemol_hip.h")).read()
    for n in names:
        assert n in _lib.EXPORTS and getattr(lib, n).argtypes is not None and f" {n}(" in header
    assert len(lib.shapemol_eval_run.argtypes) == 27 and len(lib.shapemol_eval_check.argtypes) == 13
    assert lib.shapemol_abi_version() == _lib.ABI_VERSION


# ---- the host plan, through a stand-alone program -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("mol_eval_probe") / "mol_eval_probe")
    r = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "mol_eval_probe.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(frames, sizes, graph=False):
        r = subprocess.run([exe] + ["graph"] * graph + [str(frames)] + [str(s) for s in sizes], capture_output=True, text=True)
        assert r.stderr == "", r.stderr[-2000:]                       # the sanitizers report nothing
        lines = [ln.split() for ln in r.stdout.splitlines()]
        if r.returncode:
            assert r.returncode == 1 and lines[0][0] == "error"
            return " ".join(lines[0][1:])
        return dict(mol=np.array([ln[1:] for ln in lines if ln[0] == "mol"], np.int64),
                    form={ln[1]: [int(x) for x in ln[2:]] for ln in lines if ln[0] == "form"},
                    jobs={ln[1]: [int(x) for x in ln[2:]] for ln in lines if ln[0] == "jobs"})
    return run


def test_plan_puts_molecules_into_the_right_form(probe):
    sizes = [1, 63, 64, 65, 1024, 2, 256, 257]
    p = probe(1, sizes)
    assert p["mol"][:, 2].tolist() == sizes and p["mol"][:, 1].tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    assert p["mol"][:, 3].tolist() == [0, 0, 0, 1, 1, 0, 1, 1]        # 64 atoms: a wave; 65: a workgroup
    assert p["jobs"]["wave"] == [0, 1, 2, 5] and p["jobs"]["block"] == [3, 4, 6, 7]
    assert p["form"]["wave"] == [4, 1, 1] and p["form"]["block"] == [4, 4, 1]
    assert "limit is 1024" in probe(1, [5, 1025]) and "no atoms" in probe(1, [5, 0, 3]) and "frames" in probe(0, [5])


def test_bond_graph_plan_is_the_same_plan_with_its_own_limit(probe):
    sizes = [1, 64, 65, 256]
    g = probe(3, sizes, graph=True)
    assert g["mol"][:, 2].tolist() == sizes and g["mol"][:, 3].tolist() == [0, 0, 1, 1]
    assert "limit is 256" in probe(3, [5, 257], graph=True) and "bond graph:" in probe(3, [5, 257], graph=True)
    for frames, s in ((3, sizes), (1, [30] * 1000 + [100] * 3), (7, [30] * 40000 + [100] * 9), (1 << 20, [5, 200])):
        g, e = probe(frames, s, graph=True), probe(frames, s)
        assert g["form"] == e["form"] and g["jobs"] == e["jobs"] and np.array_equal(g["mol"], e["mol"])


@pytest.mark.parametrize("frames, n_small, n_large", [(1, 1, 0), (1, 0, 1), (1, 1000, 3), (1000, 256, 0), (7, 40000, 9), (1 << 20, 5, 2), (3, 70000, 9000)])
def test_plan_grids_cover_their_jobs(probe, frames, n_small, n_large):
    """Every job of a form falls to one workgroup iteration, no workgroup is idle, and a workgroup's 32-bit LDS counts hold."""
    p = probe(frames, [30] * n_small + [100] * n_large)
    for name, jpb, n_jobs, max_iters in (("wave", 4, n_small, 65536), ("block", 1, n_large, 2048)):
        jobs, gx, iters = p["form"][name]
        assert jobs == n_jobs
        if not n_jobs:
            assert gx == 0 and iters == 0
            continue
        groups = -(-n_jobs // jpb)
        assert gx * iters >= groups > gx * (iters - 1) and 1 <= gx <= groups and iters <= max_iters
        assert gx * frames < 2 ** 31
        assert gx == groups or gx * frames >= 8192 or iters == max_iters
