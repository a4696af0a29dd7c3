"""The bond graphs on the device (shapemol_amd.mol_graph, csrc/sm_mol_graph.h) against the numpy oracle
(tests/mol_graph_oracle.py) on the crafted cases of tests/mol_graph_cases.py, which tests/test_mol_graph_cpu.py shows to be
well-posed.  Every output is an integer and must be equal: there is no tolerance in this file."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import mol_eval_oracle as E  # noqa: E402
import mol_graph_cases as K  # noqa: E402
import mol_graph_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOTS = np.arange(10)
FRAME_KEYS = ("nr_bonds", "degree", "frag", "ring", "n_bonds", "n_frags", "largest_frag", "complete", "n_cycles", "ring_sizes", "hist_bl", "hist_cc",
              "hist_all", "class_counts", "n_complete", "ring_counts")
LIST_KEYS = ("bond_list", "bond_ring", "bond_offsets")
EDGES = np.array([1.0, 1.25, 1.5, 1.75])             # 1.5 is the length of most crafted bonds: the 'left' rule puts it into bin 2


@pytest.fixture(scope="module")
def rule():
    from shapemol_amd import StabilityRule
    return StabilityRule.from_json(E.RULE_JSON)


@pytest.fixture(scope="module")
def orule():
    return E.Rule.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(report, expected, single=False):
    """Every output of the report equals the oracle's array, dtype and shape included."""
    for k in FRAME_KEYS + LIST_KEYS:
        e = torch.from_numpy(np.asarray(expected[k][0] if single and k in FRAME_KEYS else expected[k]))
        t = getattr(report, k)
        t = t.cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(t)
        assert t.dtype == e.dtype and t.shape == e.shape, (k, t.dtype, e.dtype, t.shape, e.shape)
        assert torch.equal(t, e), (k, int((t != e).sum()))


def identical(a, b):
    for k in FRAME_KEYS + LIST_KEYS:
        x, y = getattr(a, k), getattr(b, k)
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else torch.equal(x, y), k


@pytest.fixture(scope="module")
def ragged(orule):
    """T1's batch in two frames (the second: the same walks mirrored and with other classes) and the oracle's result."""
    pos, cls, batch, off = K.pack(K.ragged_batch())
    rng = np.random.default_rng(1)
    pos2, cls2 = pos * np.array([-1, 1, 1], np.float32), rng.choice([K.C_, K.N_], len(cls), p=[0.7, 0.3])
    pos, cls = np.stack([pos, pos2]), np.stack([cls, cls2])
    return pos, cls, batch, off, O.graph(pos, cls, off, orule, SLOTS, bl=EDGES)


@pytest.fixture(scope="module")
def crafted(orule):
    """T2's structures as one batch of one frame, and the oracle's result."""
    s = K.structures()
    pos, cls, batch, off = K.pack([v[:2] for v in s.values()])
    return list(s), pos, cls, batch, off, O.graph(pos[None], cls[None], off, orule, SLOTS, bl=EDGES)


def test_sizes_and_forms(rule, ragged):
    """T1: molecules of 1, 2, 63, 64, 65, 255 and 256 atoms, both forms in one ragged batch, a molecule without bonds between
    two with bonds; 257 atoms are refused."""
    from shapemol_amd import bond_graph, bond_graph_trajectory
    pos, cls, batch, off, exp = ragged
    r = bond_graph_trajectory(dev(pos), dev(cls), dev(batch), rule, mode="basic", bond_bins=EDGES, details=True)
    assert r.forms == ["wave", "wave", "wave", "wave", "block", "wave", "block", "wave", "block", "wave"]
    same(r, exp)
    assert exp["n_bonds"][0, 2] == 0 and exp["n_bonds"][0, 1] > 0 and exp["n_bonds"][0, 3] > 0
    assert set(np.unique(exp["bond_list"][:, 2]).tolist()) == {1, 2, 3} and (exp["bond_ring"] > 0).any() and (exp["bond_ring"] == 0).any()
    assert torch.equal(r.bonds(3, frame=1), dev(exp["bond_list"][exp["bond_offsets"][13]:exp["bond_offsets"][14]]))
    assert int(r.bonds(3, frame=1, local=True)[:, :2].min()) >= 0 and int(r.bonds(3, frame=1, local=True)[:, :2].max()) < 64
    assert torch.equal(r.fragments(mol=4, frame=1), dev(exp["frag"][1, off[4]:off[5]]))
    with pytest.raises(ValueError, match="limit is 256"):
        bond_graph(torch.zeros(257, 3, device=DEV), torch.ones(257, dtype=torch.int64, device=DEV), np.zeros(257, np.int64), rule)


def test_structures(rule, crafted):
    """T2: paths (the longest label propagation and breadth-first search of each form), cycles, fused and spiro rings, a cube,
    two fragments with rings, scrambled atom indices, a collapsed cluster, all orders, a NaN coordinate."""
    from shapemol_amd import bond_graph
    names, pos, cls, batch, off, exp = crafted
    r = bond_graph(dev(pos), dev(cls), dev(batch), rule, mode="basic", bond_bins=EDGES)
    same(r, exp, single=True)
    m = names.index("cube")
    assert r.rings(m).tolist() == [4] * 12 and int(r.ring_sizes[m]) == 1 << 4
    m = names.index("fused66")
    b = r.bonds(m, local=True).tolist()
    assert r.rings(m).tolist()[[x[:2] for x in b].index([2, 3])] == 6
    m = names.index("cluster20")
    assert int(r.n_bonds[m]) == 190 and set(r.rings(m).tolist()) == {3} and int(r.n_cycles[m]) == 171
    m = names.index("nan_atom")
    assert (r.fragments(mol=m) - int(off[m])).tolist() == [0, 0, 2, 3, 3] and r.degree[off[m] + 2] == 0 and not bool(r.complete[m])
    m = names.index("orders123")
    assert r.bonds(m, local=True).tolist() == [[0, 1, 1], [1, 2, 2], [2, 3, 3]]
    for name, ring, n in (("path256", 0, 256), ("cycle256", 256, 256), ("cycle64", 64, 64), ("path64", 0, 64)):
        m = names.index(name)
        assert set(r.rings(m).tolist()) == {ring} and bool(r.complete[m]) and int(r.largest_frag[m]) == n
    assert int(r.ring_sizes[names.index("cycle64")]) == np.array(1 << 31, np.uint32).astype(np.int32)
    ratio = r.ring_ratio()
    assert [ratio[s] for s in range(3, 31)] + [ratio[">30"]] == (exp["ring_counts"][0, 3:] / len(names)).tolist()
    assert ratio[4] >= 1 / len(names) and ratio[">30"] == 2 / len(names)


def test_class_outside_the_vocabulary_sets_the_status_flag(rule, crafted):
    """The class range is checked on the device: the run reports it, the context serves the next call."""
    from shapemol_amd import bond_graph
    names, pos, cls, batch, off, exp = crafted
    for bad in (10, -1):
        v = cls.copy()
        v[5] = bad
        with pytest.raises(ValueError, match="1 atom.s. have a class outside the 10 classes"):
            bond_graph(dev(pos), dev(v), dev(batch), rule, mode="basic", bond_bins=EDGES)
    same(bond_graph(dev(pos), dev(cls), dev(batch), rule, mode="basic", bond_bins=EDGES), exp, single=True)


def test_consistency_with_the_geometry_scores(rule):
    """T3: on a synthetic chain of 16 molecules x 5 frames the per-atom order sums are evaluate_trajectory's nr_bonds, and the
    class counts of complete and incomplete molecules together are its class_counts."""
    import yaml
    import shapemol_amd
    from shapemol_amd import bond_graph_trajectory, evaluate_trajectory, synth
    root = os.path.dirname(HERE)
    cfg = yaml.safe_load(open(os.path.join(root, "config", "training", "dgcnn_signeddist_512_attention_residue_uniform_pos0_10_pos1.e-7_0.01_6_v001.yml")))["model"]
    model = shapemol_amd.ScorePosNet3D(cfg, 15)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synthetic_state_dict(cfg, seed=7).items()}, strict=True)
    model = model.to(DEV)
    bb = synth.synthetic_batch(16, seed=3)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    res = model.sample_diffusion(T(bb["init_pos"]), T(bb["init_v"]), T(bb["batch"]), T(bb["shape"]).view(16, -1), num_steps=5, center_pos_mode="none", seed=5)
    assert len(res["pos_traj"]) == 5
    geo = evaluate_trajectory(res["pos_traj"], res["v_traj"], bb["batch"], rule, device=DEV)
    r = bond_graph_trajectory(res["pos_traj"], res["v_traj"], bb["batch"], rule, device=DEV)
    assert torch.equal(r.nr_bonds, geo.nr_bonds)
    N = len(bb["batch"])
    sums = torch.zeros(5 * N, dtype=torch.int64, device=DEV)
    frame_of_bond = torch.repeat_interleave(torch.arange(5, device=DEV).repeat_interleave(16), torch.from_numpy(np.diff(r.bond_offsets)).to(DEV))
    for col in (0, 1):
        sums.index_add_(0, frame_of_bond * N + r.bond_list[:, col].long(), r.bond_list[:, 2].long())
    assert torch.equal(sums.view(5, N).int(), geo.nr_bonds)
    v = torch.stack([torch.as_tensor(t) for t in res["v_traj"]]).to(DEV)
    whole = torch.stack([torch.bincount(v[f], minlength=15) for f in range(5)])
    assert torch.equal(whole, geo.class_counts)
    mol_of = torch.from_numpy(bb["batch"]).to(DEV).long()
    done = torch.stack([torch.bincount(v[f][r.complete[f][mol_of]], minlength=15) for f in range(5)])
    assert torch.equal(done, r.class_counts) and bool((r.class_counts <= geo.class_counts).all())
    assert r.validity(geometry=geo).keys() == {"mol_stable", "atm_stable", "complete"}


def test_shared_frame_serves_both_features(rule, ragged, crafted):
    """T3b: the pair, the histogram adds and the flush are one piece of code (csrc/sm_mol_rule.h) with two callers.  On the
    ragged batch, both launch forms of both kernels: equal nr_bonds, and the graph's complete-only counters nowhere above the
    scores'.  The oracle finds no frame of that batch all-complete, so the complete molecules among the crafted structures make
    one: there the counters of both are equal."""
    from shapemol_amd import bond_graph, bond_graph_trajectory, evaluate_geometry, evaluate_trajectory
    counters = ("hist_cc", "hist_all", "class_counts")
    pos, cls, batch, off, exp = ragged
    g = bond_graph_trajectory(dev(pos), dev(cls), dev(batch), rule, mode="basic", bond_bins=EDGES, details=True)
    s = evaluate_trajectory(dev(pos), dev(cls), dev(batch), rule, mode="basic", details=True)
    assert g.forms == s.forms and set(g.forms) == {"wave", "block"}
    assert torch.equal(g.nr_bonds, s.nr_bonds)
    for k in counters:
        a, b = getattr(g, k), getattr(s, k)
        assert a.dtype == b.dtype and a.shape == b.shape and bool((a <= b).all()), k
    assert not exp["complete"].all(axis=1).any() and bool((g.hist_all < s.hist_all).any())
    names, cpos, ccls, _, coff, cexp = crafted
    whole = np.flatnonzero(cexp["complete"][0])                                # the oracle's word, molecule by molecule
    assert {"path64", "path256", "cycle256", "cube"} <= {names[m] for m in whole} and len(whole) < len(names)
    pos, cls, batch, off = K.pack([(cpos[coff[m]:coff[m + 1]], ccls[coff[m]:coff[m + 1]]) for m in whole])
    g = bond_graph(dev(pos), dev(cls), dev(batch), rule, mode="basic", bond_bins=EDGES, details=True)
    s = evaluate_geometry(dev(pos), dev(cls), dev(batch), rule, mode="basic", details=True)
    assert set(g.forms) == {"wave", "block"} and bool(g.complete.all()) and int(g.n_complete) == len(whole)
    assert torch.equal(g.nr_bonds, s.nr_bonds)
    for k in counters:
        assert torch.equal(getattr(g, k), getattr(s, k)) and int(getattr(g, k).sum()) > 0, k


def test_accumulations(rule, orule, crafted):
    """T4: bond-length histograms over all and over complete molecules, the complete-only pair histograms and class counts,
    the ring-size counters; a distance exactly on a bin edge; a frame without a complete molecule."""
    from shapemol_amd import bond_graph_trajectory
    names, pos, cls, batch, off, _ = crafted
    far = pos * np.float32(8)                                                  # nothing bonds; no molecule has one atom
    pos3, cls3 = np.stack([pos, far, pos * np.array([-1, 1, 1], np.float32)]), np.stack([cls, cls, cls])
    exp = O.graph(pos3, cls3, off, orule, SLOTS, bl=EDGES)
    r = bond_graph_trajectory(dev(pos3), dev(cls3), dev(batch), rule, mode="basic", bond_bins=EDGES)
    same(r, exp)
    cc = O.pair_index(1, 1, 10)
    # the 63 + 255 bonds of the two paths alone have d == 1.5 == edge 2: bin 2 by the 'left' rule (bin 3 by the other)
    assert exp["hist_bl"][0, 0, cc, 0, 2] >= 318 > exp["hist_bl"][0, 0, cc, 0, 3]
    assert (exp["hist_bl"][0, 0] >= exp["hist_bl"][0, 1]).all() and exp["hist_bl"][0, 0].sum() > exp["hist_bl"][0, 1].sum() > 0
    assert exp["n_complete"].tolist()[1] == 0 and exp["n_complete"][0] > 0
    for k in ("hist_cc", "hist_all", "class_counts", "ring_counts"):
        assert exp[k][1].sum() == 0 and exp[k][0].sum() > 0, k
    assert exp["hist_bl"][1].sum() == 0
    emp = {(6, 6, 1): np.full(5, 0.2), (7, 6, 1): np.full(5, 0.2), (6, 6, 2): np.full(5, 0.2), "CC_2A": np.full(101, 1 / 101)}
    with np.errstate(all="raise"):                                             # no division by zero
        empty = r.jsd(emp, frame=1)
        profile = r.bond_length_profile(frame=1)
    assert all(not p.any() for p in profile.values())
    full = r.jsd(emp, frame=0)
    assert empty == {"JSD_6-6|1": None, "JSD_7-6|1": None, "JSD_6-6|2": None, "JSD_CC_2A": None} and r.validity(frame=1) == {"complete": 0.0}
    from scipy.spatial import distance
    h = exp["hist_bl"][0, 1, cc, 0].astype(np.float64)
    assert full["JSD_6-6|1"] == distance.jensenshannon(np.full(5, 0.2), h / h.sum()) and full["JSD_7-6|1"] is not None
    assert r.validity()["complete"] == exp["complete"].mean()


def test_determinism_and_workspace(rule, ragged, crafted):
    """T5: the same call twice with the workspace 0xFF-filled in between gives the same bits; a larger call after a smaller one
    grows the workspace, and the smaller one after it is unchanged."""
    from shapemol_amd import bond_graph, bond_graph_trajectory, mol_graph
    names, pos, cls, batch, off, exp = crafted
    small = lambda: bond_graph(dev(pos[:off[3]]), dev(cls[:off[3]]), dev(batch[:off[3]]), rule, mode="basic", bond_bins=EDGES)  # noqa: E731
    first = small()
    mol_graph._debug_fill(torch.device(DEV), 0xFF)
    second = small()
    identical(first, second)
    rp, rc, rb, roff, rexp = ragged
    same(bond_graph_trajectory(dev(rp), dev(rc), dev(rb), rule, mode="basic", bond_bins=EDGES), rexp)
    mol_graph._debug_fill(torch.device(DEV), 0xFF)
    same(bond_graph_trajectory(dev(rp), dev(rc), dev(rb), rule, mode="basic", bond_bins=EDGES), rexp)
    identical(first, small())


def test_dtype_and_layout(rule, crafted):
    """T6: int32 and int64 classes; one frame as (N, 3) and as (1, N, 3)."""
    from shapemol_amd import bond_graph, bond_graph_samples
    names, pos, cls, batch, off, exp = crafted
    a = bond_graph(dev(pos), dev(cls), batch, rule, mode="basic", bond_bins=EDGES)
    b = bond_graph(dev(pos), dev(cls).to(torch.int32), batch, rule, mode="basic", bond_bins=EDGES)
    c = bond_graph(dev(pos)[None], dev(cls)[None], batch, rule, mode="basic", bond_bins=EDGES)
    d = bond_graph_samples(([pos[off[k]:off[k + 1]] for k in range(len(names))], [cls[off[k]:off[k + 1]] for k in range(len(names))]), rule, mode="basic",
                           bond_bins=EDGES)
    same(a, exp, single=True)
    for other in (b, c, d):
        identical(a, other)
    assert a.nr_bonds.shape == (len(cls),) and c.n_bonds.shape == (len(names),)
