"""The statistic stage of classifier-free guidance (shapemol_amd/csrc/sm_cfg.h: radix-select quantile, fixed-order float64
reductions, whole-batch and per-group forms) on crafted tensors through shapemol_debug_cfg_stats, against plain references: the
quantile equals torch.quantile (CPU float32) and the sort-and-lerp restatement with ==, reference_threshold equals
float32(max|cond|) * float32(p), rescale is inside the project's float64 gate, every group's statistic is the whole-batch
statistic of its slice bit for bit.  tests/cfg_stats_cases.py holds the cases, tests/test_cfg_stats_cpu.py shows on the CPU that
each case exercises the branch it is named after and that the two quantile references agree on it.
Run on the GPU box:  pytest tests/test_gpu_cfg_stats.py -m gpu"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import cfg_stats_cases as K  # noqa: E402
from util import T, golden, hash_noise, hip_model, maxabs, record, synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TYPES = ("reference_threshold", "dynamic_threshold", "rescale")
BIG = 600_000       # above this many elements a tensor is compared with the restatement only (the CPU file shows it equals torch.quantile on the same data)


def model(num_classes):
    """A model of its own (seed 11): the workspace these tests grow stays out of the contexts the chain tests share."""
    return hip_model(seed=11, num_classes=num_classes, cond_mask_prob=0.1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Inputs:
    """The four prediction tensors of one hook call on the device, and the combined tensors on the host."""

    def __init__(self, N, Cn, cond, uncond, w, batch=None):
        self.N, self.C = N, Cn
        self.cond, self.uncond = cond, uncond                     # {'pos': (3N,), 'v': (N C,)} float32 numpy
        self.dev = [T(a, DEV) for a in (cond["pos"].reshape(N, 3), uncond["pos"].reshape(N, 3), cond["v"].reshape(N, Cn), uncond["v"].reshape(N, Cn))]
        self.batch = T(np.zeros(N, dtype=np.int64) if batch is None else batch, DEV)
        self.B = int(self.batch[-1].item()) + 1
        if w is not None:
            self.x = {k: K.combine(cond[k], uncond[k], w) for k in ("pos", "v")}

    def run(self, m, **setting):
        return m.debug_cfg_stats(*self.dev, self.batch, self.B, **setting)

    def rows(self, lo, hi, mol0):
        """The slice of atoms [lo, hi) as inputs of its own."""
        sub = Inputs.__new__(Inputs)
        sub.N, sub.C = hi - lo, self.C
        sub.dev = [t[lo:hi].contiguous() for t in self.dev]
        sub.batch = (self.batch[lo:hi] - mol0).contiguous()
        sub.B = int(sub.batch[-1].item()) + 1
        return sub


def case_inputs(case, w):
    t = K.tensors(case.profile, case.N, case.C)
    cond = {k: t[k][0] for k in ("pos", "v")}
    if w == 1.0:
        uncond = {k: np.zeros_like(v) for k, v in cond.items()}
    else:
        uncond = {k: K.mixed_uncond(case.profile, case.N, case.C, k) for k in ("pos", "v")}
    return Inputs(case.N, case.C, cond, uncond, w), {k: t[k][1] for k in ("pos", "v")}


# ---------------------------------------------------------------------------------------------- quantile
@pytest.mark.parametrize("case", K.QUANT, ids=[K.case_id(c) for c in K.QUANT])
def test_quantile_is_exact(case):
    """dynamic_threshold on both tensors of the case: with w = 1, uncond = 0 (x = 2 cond exactly) at the generic p and at the p
    the profile computes for its own ranks (the last copy of a tie, the last key of a 22-bit prefix, the last negative), and with
    w = 0.7 and a random uncond at two p.  The device value equals torch.quantile on the CPU and the sort-and-lerp restatement
    with == (-0.0 == 0.0), no tolerance.  At N = 174 763 the context takes the atoms (a 1.8 GB workspace), so the positions
    cover their cap; that case's 2.6 M logits are compared with the restatement alone."""
    m = model(case.C)
    for w in (1.0, K.W_MIXED):
        inp, claims = case_inputs(case, w)
        ps = K.P_MIXED if w != 1.0 else sorted(set(K.p_list(claims["pos"])) | set(K.p_list(claims["v"])))
        ref = {k: (torch.from_numpy(inp.x[k]), np.sort(inp.x[k])) for k in ("pos", "v")}
        for p in ps:
            stat = inp.run(m, guide_stren=w, threshold_type="dynamic_threshold", p=p)
            for i, k in enumerate(("pos", "v")):
                xt, srt = ref[k]
                want = [K.quantile_sorted(srt, p)] + ([np.float32(torch.quantile(xt, p).item())] if len(srt) <= BIG else [])
                for q in want:
                    assert not np.isnan(stat[i]) and q == stat[i], (case, w, p, k, q, stat[i])
    record("cfg_stats_quantile_exact", case=K.case_id(case))


# ---------------------------------------------------------------------------------------------- reference_threshold
@pytest.mark.parametrize("case", K.THRESH, ids=[K.case_id(c) for c in K.THRESH])
def test_reference_threshold_is_exact(case):
    """s = float32(max|cond|) * float32(p) exactly: the largest magnitude in every workgroup (ties3), or once, negative, as the
    last element the last workgroup reads (maxneg), up to the capped workgroup count and its 256-partial final reduction."""
    m = model(case.C)
    for w in (1.0, K.W_MIXED):
        inp, _ = case_inputs(case, w)
        for p in (1.05, 0.3):
            stat = inp.run(m, guide_stren=w, threshold_type="reference_threshold", p=p)
            for i, k in enumerate(("pos", "v")):
                want = np.float32(np.abs(inp.cond[k]).max()) * np.float32(p)
                assert want == stat[i], (case, w, p, k, want, stat[i])
                if case.profile == "maxneg":
                    assert want == np.float32(7.5) * np.float32(p)


# ---------------------------------------------------------------------------------------------- rescale
@pytest.mark.parametrize("case", K.RESCALE, ids=[K.case_id(c) for c in K.RESCALE])
def test_rescale_is_inside_the_gate(case):
    """r = std(cond) / std(x) against float64 two-pass unbiased standard deviations: eH <= 4 e32 + 16 * 2^-24 relative to the
    float64 value, e32 the error of CPU float32 torch.std(cond) / torch.std(x).  Zero-mean, heavy-tailed and un-centred data
    (mean / spread 50 and 1e5), small and above the workgroup cap; prints eH, e32 and eH / bound."""
    m = model(case.C)
    worst = 0.0
    for w in (1.0, K.W_MIXED):
        inp, _ = case_inputs(case, w)
        stat = inp.run(m, guide_stren=w, threshold_type="rescale", p=0.7)
        for i, k in enumerate(("pos", "v")):
            r64, e32, bound = K.rescale_gate(inp.x[k], inp.cond[k])
            eH = abs(float(stat[i]) - r64) / r64
            print(f"cfg_stats_rescale {K.case_id(case)} {k} w={w}: r {stat[i]:.9g} eH {eH:.3e} e32 {e32:.3e} eH/bound {eH / bound:.4f}")
            record("cfg_stats_rescale", case=K.case_id(case), tensor=k, w=w, eH=eH, e32=e32, ratio=eH / bound)
            worst = max(worst, eH / bound)
            assert eH <= bound, (case, w, k, eH, e32, bound)
    print(f"cfg_stats_rescale_worst {K.case_id(case)} {worst:.4f}")


# ---------------------------------------------------------------------------------------------- groups
_group_inputs = {}


def group_inputs(name):
    if name not in _group_inputs:
        Cn, counts, _, _ = K.GROUP_LAYOUTS[name]
        N = int(sum(counts))
        cond, uncond = {}, {}
        for k, n in (("pos", 3 * N), ("v", Cn * N)):
            cond[k] = K.profile("wide", n, K.seed_of("groups", name, k))[0]
            uncond[k] = np.random.RandomState(K.seed_of("groups", name, k, "u")).standard_normal(n).astype(np.float32)
        batch = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
        _group_inputs[name] = Inputs(N, Cn, cond, uncond, None, batch)
    return _group_inputs[name]


@pytest.mark.parametrize("ttype", TYPES)
@pytest.mark.parametrize("name", list(K.GROUP_LAYOUTS))
def test_group_statistics_are_the_slices_statistics(name, ttype):
    """shapemol_set_cfg_groups on one chain-shaped batch vector -- a single-atom group, 2048 logits, a w_g = 0 group between
    guided ones, 2049 coordinates, a group above the workgroup cap beside small ones, ranges that start at odd elements; or 256
    groups of one molecule: every group's statistic equals the whole-batch hook's on that group's slice alone bit for bit (the
    independence rule), the quantile equals torch.quantile of the slice, a w_g = 0 group gets the identity, and a second call
    after another layout left its histograms and tables gives the same bits."""
    Cn, counts, group_mols, strens = K.GROUP_LAYOUTS[name]
    m, inp = model(Cn), group_inputs(name)
    mol_off, atom_off = K.group_offsets(counts, group_mols)
    groups = list(zip(strens, group_mols))
    other = [(0.8, n) for n in K.OTHER_LAYOUT[name]]
    for p in K.GROUP_P[ttype]:
        kw = dict(threshold_type=ttype, p=p)
        stat = inp.run(m, guide_stren=groups, **kw)
        assert stat.shape == (len(groups), 2)
        for g, w in enumerate(strens):
            lo, hi = int(atom_off[g]), int(atom_off[g + 1])
            if w == 0.0:
                assert np.array_equal(stat[g], np.full(2, 1.0 if ttype == "rescale" else np.inf, dtype=np.float32)), (g, stat[g])
                continue
            alone = inp.rows(lo, hi, int(mol_off[g])).run(m, guide_stren=w, **kw)
            assert np.array_equal(bits(alone), bits(stat[g])), (name, ttype, p, g, alone, stat[g])
            for i, (k, per) in enumerate((("pos", 3), ("v", Cn))):
                sl = slice(lo * per, hi * per)
                if ttype == "dynamic_threshold":
                    q = torch.quantile(torch.from_numpy(K.combine(inp.cond[k][sl], inp.uncond[k][sl], w)), p).item()
                    assert np.float32(q) == stat[g, i], (name, p, g, k, q, stat[g, i])
                elif ttype == "reference_threshold":
                    assert np.float32(np.abs(inp.cond[k][sl]).max()) * np.float32(p) == stat[g, i], (name, g, k)
                else:
                    r64, e32, bound = K.rescale_gate(K.combine(inp.cond[k][sl], inp.uncond[k][sl], w), inp.cond[k][sl])
                    assert abs(float(stat[g, i]) - r64) / r64 <= bound, (name, g, k, stat[g, i], r64, e32)
        inp.run(m, guide_stren=other, **kw)
        again = inp.run(m, guide_stren=groups, **kw)
        assert np.array_equal(bits(again), bits(stat)), (name, ttype, p)


# ---------------------------------------------------------------------------------------------- the hook itself
def _raw(m, inp, *, null=None, N=None, B=None):
    from shapemol_amd import _lib
    from shapemol_amd._native import ptr, stream_ptr
    lib, ctx = _lib.load(), m._context(torch.device(DEV))
    args = [ptr(t) for t in inp.dev] + [ptr(inp.batch)]
    if null is not None:
        args[null] = None
    with torch.cuda.device(DEV):
        rc = lib.shapemol_debug_cfg_stats(ctx, *args, inp.N if N is None else N, inp.B if B is None else B, stream_ptr(torch.device(DEV)))
    return rc, lib.shapemol_last_error()


def _captures(m):
    from shapemol_amd import _lib
    out = C.c_int64(0)
    assert _lib.load().shapemol_debug_read(m._context(torch.device(DEV)), b"captures", C.byref(out), 8) == 8
    return out.value


def test_hook_refuses_before_any_launch():
    """No setting installed, a null pointer, sizes out of range, a group set of another molecule count: refused with a message,
    no launch, no workspace growth, no capture dropped; the hook works afterwards."""
    from shapemol_amd import _lib
    m = model(15)
    case = K.Quant("natural", 683, 15, "")
    inp, _ = case_inputs(case, 1.0)
    want = inp.run(m, guide_stren=1.0, threshold_type="dynamic_threshold", p=0.5)
    lib, ctx = _lib.load(), m._context(torch.device(DEV))
    dims0 = m.debug_read("dims", (8,), np.int64)
    rc, msg = _raw(m, inp)
    assert rc != 0 and b"no classifier-free guidance setting" in msg
    assert lib.shapemol_set_cfg(ctx, 1.0, 2, 0.5, None, None, None) == 0
    try:
        for i in range(5):
            rc, msg = _raw(m, inp, null=i)
            assert rc != 0 and b"null argument" in msg, i
        for kw in (dict(N=0), dict(B=0), dict(N=(1 << 27) + 1), dict(B=inp.N + 1)):
            rc, msg = _raw(m, inp, **kw)
            assert rc != 0 and b"out of range" in msg, kw
        assert lib.shapemol_set_cfg_groups(ctx, 2, (C.c_int64 * 3)(0, 2, 5), (C.c_double * 2)(0.7, 1.5), 2, 0.5, None, None, None) == 0
        rc, msg = _raw(m, inp)
        assert rc != 0 and b"groups cover 5 molecules" in msg
        assert lib.shapemol_set_cfg_groups(ctx, 0, None, None, 0, 0.0, None, None, None) == 0
        assert np.array_equal(m.debug_read("dims", (8,), np.int64), dims0)
        assert _raw(m, inp)[0] == 0
        assert np.array_equal(bits(m.debug_read("cfg_stat", (2,), np.float32)), bits(want))
    finally:
        lib.shapemol_set_cfg_groups(ctx, 0, None, None, 0, 0.0, None, None, None)
        lib.shapemol_set_cfg(ctx, 0.0, 0, 0.0, None, None, None)


@pytest.mark.parametrize("tag", ["dynamic_threshold", "rescale"])
def test_hook_and_chain_do_not_disturb_each_other(tag):
    """On the golden chains' own model: the reference's B = 4, 50-step chain (tests/golden/chain_cfg_<tag>.npz) is bit-identical
    before and after hook calls in both forms, still meets its golden, needs no new capture, and the hook right after a chain
    gives the crafted tensors' exact statistic."""
    m = hip_model(cond_mask_prob=0.1)
    c = golden(f"chain_cfg_{tag}.npz")
    B, S, seed = int(c["B"]), int(c["S"]), int(c["seed"])
    bb = synth.synthetic_batch(B, seed=seed)
    eps, u = hash_noise(len(bb["batch"]), S, seed)
    args = (T(bb["init_pos"], DEV), T(bb["init_v"], DEV), T(bb["batch"], DEV), T(bb["shape"], DEV).view(B, -1))
    kw = dict(num_steps=S, center_pos_mode="none", noise=(T(eps, DEV), T(u, DEV)), threshold_type=tag, threshold_args={"p": float(c["p"])},
              guide_stren=float(c["guide_stren"]), bounds=torch.from_numpy(c["bounds"]).float())
    case = K.Quant("twoprefix", 20, 15, "")          # fewer atoms than the chain: no workspace growth, the captured step stays
    inp, claims = case_inputs(case, 1.0)
    p = claims["pos"][0].p if tag == "dynamic_threshold" else 0.7
    inp.run(m, guide_stren=[(1.0, 1)], threshold_type=tag, p=p)      # (the first group set of a context allocates its rows: that drops a capture)
    before = m.sample_diffusion(*args, **kw)
    caps = _captures(m)
    one = inp.run(m, guide_stren=1.0, threshold_type=tag, p=p)
    grp = inp.run(m, guide_stren=[(1.0, 1)], threshold_type=tag, p=p)
    assert np.array_equal(bits(one), bits(grp[0]))
    if tag == "dynamic_threshold":
        assert one[0] == np.float32(torch.quantile(torch.from_numpy(inp.x["pos"]), p).item())
    after = m.sample_diffusion(*args, **kw)
    assert _captures(m) == caps
    assert torch.equal(before["pos"], after["pos"]) and torch.equal(before["v"], after["v"])
    for k in ("pos_traj", "v0_traj", "vt_traj", "pos_uncond_traj", "v_uncond_traj"):
        assert torch.equal(torch.stack(before[k]), torch.stack(after[k])), k
    assert np.array_equal(after["v"].cpu().numpy(), c["v"]) and maxabs(after["pos"], c["pos"]) <= 1e-4
    assert np.array_equal(bits(inp.run(m, guide_stren=1.0, threshold_type=tag, p=p)), bits(one))
