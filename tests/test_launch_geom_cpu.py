"""csrc/sm_launch.h without a GPU: the launch geometry and step forms that shapemol_hip.hip's launchers and decisions share.

tests/launch_geom_probe.cpp includes the header alone and prints the step forms and every geometry over num_cu in {4, 64, 256, 304},
KP of k in {4, 8, 12, 16, 24, 32}, H in {32, 128}, both precision modes, max_mol_atoms in {0, 1, 2, 33, 97, 128, 129} (and 121, 122: the fold's boundary where eight one-job f16 waves own 16 atoms) and every N from
1 past the last form switch of the CU count (the CU count is an input, so every switch is reached at small N; at 256 CUs N runs past
the 6144 atoms where the f16 kernels start to loop), and again with one option off its default.  Held here: chain_forms.py's
formulas -- which the GPU tests hold the library's launch records to -- equal the header's values; a fold never exceeds the LDS
table of the geometry launched; the fused x2h + node launch has one job per wave and fits the node stage's column tiles; every
geometry covers its jobs without an idle workgroup.  The probe is built with the address and undefined-behaviour sanitizers (host
code only: the flag goes behind -Xarch_host) and must leave no report."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import chain_forms as CF
from test_gpu_parity import MODE_IDS
from util import ROOT

STREAM_TPR, CHAIN_COLS, LIN6_CHUNK = 2, 2, 8      # kStreamTPR, CHAIN_COLS, kLin6Chunk of the kernel headers
MAX_MOL = (0, 1, 2, 33, 97, 128, 129, 121, 122)   # kMaxMol of the probe
KS = (4, 8, 12, 16, 24, 32)
ONE, LOOP, SLICED, STRIDED = range(4)             # lg::Form


class Table:
    def __init__(self, text):
        lines = text.split("\n", 1)
        self.names = lines[0].split()
        body = lines[1].split("\n")
        self.variants = [ln[2:] for ln in body if ln.startswith("# ")]
        data = np.array(" ".join(body[len(self.variants):]).split(), dtype=np.int64)
        self.rows = data.reshape(-1, len(self.names))

    def __getitem__(self, name):
        return self.rows[:, self.names.index(name)]

    def variant(self, *names):
        return np.isin(self["variant"], [self.variants.index(n) for n in names])


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    hipcc = shutil.which("hipcc") or (os.path.exists("/opt/rocm/bin/hipcc") and "/opt/rocm/bin/hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("launch_geom_probe") / "launch_geom_probe")
    r = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "launch_geom_probe.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe] + [str(v) for v in (CF.FOLD_CAP, STREAM_TPR, CHAIN_COLS, CF.GRAPH_CAP, LIN6_CHUNK)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == "", r.stderr[-2000:]      # the sanitizers report nothing
    return Table(r.stdout)


def test_sweep_covers_the_cases(table):
    t = table
    assert set(np.unique(t["num_cu"])) == {4, 64, 256, 304} and set(np.unique(t["H"])) == {32, 128}
    assert set(np.unique(t["KP"])) == {CF.kp_of(k) for k in KS} and set(np.unique(t["mode"])) == set(range(len(MODE_IDS)))
    assert len(t.variants) == 12 and set(np.unique(t["variant"])) == set(range(12))
    d = t.variant("default")
    for cu in (4, 64, 256, 304):
        n = t["N"][d & (t["num_cu"] == cu)]
        assert n.min() == 1 and n.max() > 40 and len(np.unique(n)) == n.max()      # every N
    # ... past every switch: all forms of the f16 launch at the real CU count, both sides of the tail's and the fold's boundary
    real = d & (t["num_cu"] == 256) & (t["mode"] == 1)
    assert set(np.unique(t["e_form"][real])) == {ONE, LOOP} and t["N"][real].max() > 6144
    assert set(np.unique(t["e_form"][t.variant("edge_tiles")])) == {ONE, SLICED}
    ex = d & (t["mode"] == 0) & (t["KP"] <= 16)
    assert set(np.unique(t["out_fused"][ex])) == {0, 1} and t["s_apw"][ex].max() > CF.FOLD_CAP
    assert set(np.unique(t["xc_fused"][d & (t["mode"] == 1)])) == {0, 1}
    assert t["xc_fused"][t.variant("chain16_does_not_fit", "lin_fuse", "edge_waves")].max() == 0


def test_chain_forms_streaming_formulas_equal_the_header(table):
    t = table
    m = ~t.variant("stream_chunk", "stream_whole_rounds")       # chain_forms.py states the automatic chunk
    pts, inv = np.unique(np.stack([t["N"][m], t["KP"][m], t["num_cu"][m]], 1), axis=0, return_inverse=True)
    ref = np.array([[CF.stream_jobs(n, kp), CF.stream_chunk(n, kp, cu), CF.stream_grid(n, kp, cu)] for n, kp, cu in pts.tolist()])[inv.reshape(-1)]
    for i, col in enumerate(("s_jobs", "s_chunk", "s_grid")):
        assert np.array_equal(ref[:, i], t[col][m]), col


def test_chain_forms_fold_equals_the_header(table):
    """fold_atoms, at every point: the atoms the fold counts -- the streaming workgroup's, or the larger of the two f16 x2h launches'.
    fold_expected and graph_fused_expected with the true hint, at every N a molecule of max_mol_atoms fits in and every CU count
    (H = 128, the width chain_forms.py's fold_expected states)."""
    t = table
    d = t.variant("default")
    own = np.where(t["mode"] == 0, t["s_apw"], np.maximum(t["e_apw"], t["x_apw"]))
    pts, inv = np.unique(np.stack([t["mode"][d], t["N"][d], t["KP"][d], t["num_cu"][d], t["H"][d]], 1), axis=0, return_inverse=True)
    ref = [CF.fold_atoms(MODE_IDS[mode], n, kp, cu, h) for mode, n, kp, cu, h in pts.tolist()]
    none = np.array([a is None for a in ref])[inv.reshape(-1)]
    atoms = np.array([a or 0 for a in ref])[inv.reshape(-1)]
    assert np.array_equal(none, t["KP"][d] > 16)
    assert np.array_equal(atoms[~none], own[d][~none])
    assert not t["fold_bits"][d][none].any()
    d &= t["H"] == 128
    rows = np.stack([t["mode"][d], t["N"][d], t["KP"][d], t["num_cu"][d]], 1).tolist()
    k_of = {CF.kp_of(k): [kk for kk in KS if CF.kp_of(kk) == CF.kp_of(k)] for k in KS}
    for bit, mm in enumerate(MAX_MOL):
        got_fold, got_graph = (t["fold_bits"][d] >> bit) & 1, (t["graph_fused_bits"][d] >> bit) & 1
        if mm == 0:      # no hint: neither
            assert not got_fold.any() and not got_graph.any()
            continue
        fits = t["N"][d] >= mm
        assert np.array_equal(got_graph, np.full(len(got_graph), CF.graph_fused_expected(np.array([mm]))))
        memo = {}
        for i, (mode, n, kp, cu) in enumerate(rows):
            if not fits[i]:
                continue
            key = (mode, n, kp, cu)
            if key not in memo:
                counts = np.full(-(-n // mm), mm)
                counts[-1] = n - mm * (len(counts) - 1)
                want = {CF.fold_expected(MODE_IDS[mode], counts, k, cu) for k in k_of[kp]}
                assert len(want) == 1
                memo[key] = want.pop()
            assert bool(got_fold[i]) == memo[key], (key, mm)


def test_a_fold_fits_the_table_of_the_launch(table):
    t = table
    launched = np.where(t["mode"] == 0, t["s_apw"], np.where(t["xc_fused"] == 1, t["x_apw"], t["e_apw"]))
    for bit, mm in enumerate(MAX_MOL):
        on = ((t["fold_bits"] >> bit) & 1) == 1
        assert mm > 0 or not on.any()
        assert (t["KP"][on] <= 16).all() and (launched[on] > 0).all()
        assert (launched[on] + 2 * (mm - 1) <= CF.FOLD_CAP).all(), mm
    f16_one = t.variant("default") & (t["mode"] == 1) & (t["KP"] == 8) & (t["H"] == 128) & (np.maximum(t["e_apw"], t["x_apw"]) == 16) & (t["N"] >= 122)
    assert ((t["fold_bits"][f16_one] >> MAX_MOL.index(121)) & 1).all() and not ((t["fold_bits"][f16_one] >> MAX_MOL.index(122)) & 1).any()
    assert (t["fold_bits"] != 0).any() and (t["fold_bits"][t.variant("edge_waves")] == 0).all()


def test_the_fused_x2h_launch_has_one_job_per_wave(table):
    t = table
    on = t["xc_fused"] == 1
    assert (t["x_form"][on] == ONE).all() and (t["x_jobs"][on] <= t["x_grid"][on] * t["x_waves"][on]).all()
    apj = 16 // t["KP"][on]
    assert (t["x_waves"][on] * apj <= CHAIN_COLS * 16).all() and (t["x_apw"][on] == t["x_waves"][on] * apj).all()
    assert (t["x_waves"][on] >= t["H"][on] // 16).all() and (t["x_waves"][on] <= 12).all()
    big = (t["s_apw"] > 3 * CHAIN_COLS * 16) & ~t.variant("x2h_out_fuse_2")      # the tail: three passes of 32 atoms at the most
    assert big.any() and (t["out_fused"][big] == 0).all()


def covers(grid, chunk, jobs):
    return (grid * chunk >= jobs).all() and ((grid - 1) * chunk < jobs).all() and (grid >= 1).all()


def test_every_geometry_covers_its_jobs(table):
    t = table
    assert covers(t["s_grid"], t["s_chunk"], t["s_jobs"])
    whole = t["e_form"] != SLICED
    assert covers(t["e_grid"][whole], t["e_chunk"][whole], t["e_jobs"][whole])
    sl = ~whole      # slices of grid x waves jobs; the last one holds the rest
    assert (t["e_slice"][sl] == t["e_grid"][sl] * t["e_chunk"][sl]).all() and (t["e_chunk"][sl] == t["e_waves"][sl]).all()
    rest = t["e_jobs"][sl] - (t["e_jobs"][sl] - 1) // t["e_slice"][sl] * t["e_slice"][sl]
    assert covers(t["e_last_grid"][sl], t["e_chunk"][sl], rest) and (t["e_last_grid"][sl] <= t["e_grid"][sl]).all()
    one = t["e_form"] == ONE
    assert (t["e_last_grid"][one] == t["e_grid"][one]).all()
    xo = t["x_form"] == ONE
    assert covers(t["x_grid"][xo], t["x_waves"][xo], t["x_jobs"][xo])
    po = t["p_form"] == ONE
    assert covers(t["p_grid"][po], t["p_chunk"][po], t["p_jobs"][po])
    assert ((t["p_grid"][~po] - 1) * t["p_chunk"][~po] < t["p_jobs"][~po]).all() and (t["p_form"][~po] == STRIDED).all()
    assert (t["q_grid"] >= 1).all() and (t["q_grid"] <= t["q_jobs"]).all()
    auto = ~t.variant("stream_chunk")      # (a given chunk takes as many workgroups as it needs)
    for col in ("s_grid", "e_grid", "x_grid", "p_grid", "q_grid"):
        assert (t[col][auto] <= t["num_cu"][auto]).all(), col
    assert covers(t["l_agroups"], t["l_tpg"], t["l_n_ct"])
    assert covers(t["n_pairs"], np.full(len(t.rows), CHAIN_COLS), t["n_n_ct"])
    lw = np.where(t.variant("after_waves"), 8, 16)
    ogroups = -(-8 * (t["H"] // 16) // lw)
    assert (t["n_ljobs"] % ogroups == 0).all() and covers(t["n_ljobs"] // ogroups, t["n_tpg"], t["n_n_ct"])
    assert (t["n_lin_chunk"] >= 1).all() and (t["n_lin_chunk"] <= np.minimum(t["n_tpg"], LIN6_CHUNK)).all()
    assert (t["n_fjobs"] == 2 * t["n_pairs"]).all() and (t["n_bw"] == np.maximum(lw, t["H"] // 16)).all()
