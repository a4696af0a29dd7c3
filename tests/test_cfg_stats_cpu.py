"""What makes the gates of tests/test_gpu_cfg_stats.py meaningful, on the CPU: for every case of tests/cfg_stats_cases.py the
two references of the quantile (torch.quantile in float32, the sort-and-lerp restatement) agree bit for bit, the ranks lie where
the case claims (same key / another last digit / another 22-bit prefix / another sign, the tie multiplicity, the workgroup
count), a numpy model of the three radix passes with the min-above channel and the finalize -- the algorithm as the header
comment of shapemol_amd/csrc/sm_cfg.h documents it -- gives the reference's value through the branch the case is named after,
and the model of the fixed-order float64 sums passes the rescale gate."""
import os
import re

import numpy as np
import pytest
import torch

import cfg_oracle as O
import cfg_stats_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRANCH = {"same": "same", "digit": "next_bin", "prefix": "min_above", "sign": "min_above"}      # the arm of sm_cfg.h:368-369 a relation takes


def _src(*path):
    return open(os.path.join(ROOT, *path)).read()


def same_float(a, b):
    """== on float32 values (so that -0.0 == 0.0 holds, as the device tests compare), neither NaN."""
    a, b = np.float32(a), np.float32(b)
    return not np.isnan(a) and not np.isnan(b) and a == b


def test_the_restated_constants_are_the_sources():
    src = _src("shapemol_amd", "csrc", "sm_cfg.h")
    assert re.search(r"constexpr int kCfgBins = 2048;", src) and re.search(r"constexpr int kCfgMaxBlocks = 256;", src)
    assert re.search(r"constexpr int kCfgMaxGroups = 256;", src) and re.search(r"kCfgShift\[3\] = \{21, 10, 0\};", src)
    assert "long long nb = (n + 2047) / 2048;" in src and "const unsigned mask = PASS == 2 ? 1023u : 2047u;" in src
    assert "(u & 0x80000000u) ? ~u : (u | 0x80000000u)" in src
    host = _src("shapemol_amd", "csrc", "shapemol_hip.hip")
    assert "std::min<int64_t>(kCfgMaxBlocks, std::max<int64_t>(1, (n + 2047) / 2048))" in host
    from shapemol_amd import _lib
    assert _lib.CFG_MAX_GROUPS == K.MAX_GROUPS


def test_the_hook_is_declared_exported_and_shares_the_chain_code():
    """shapemol_debug_cfg_stats is in the header and in _lib.EXPORTS (ABI version 5 stays), and its body calls the chain's own
    prep helper, cfg_args and run_cfg_stats; shapemol_sample reaches the table launch through the same helper only."""
    from shapemol_amd import _lib
    hdr, host = _src("include", "shapemol_hip.h"), _src("shapemol_amd", "csrc", "shapemol_hip.hip")
    assert "int shapemol_debug_cfg_stats(" in hdr and "shapemol_debug_cfg_stats" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 5 and re.search(r"SHAPEMOL_ABI_VERSION\s+5", hdr)
    body = host[host.index("int shapemol_debug_cfg_stats("):]
    body = body[:body.index("\n}\n")]
    for name in ("run_cfg_prep(c, s, d_batch, N, B)", "cfg_args(c, N)", "run_cfg_stats(c, s, a)", "ensure_workspace(c, N, B)"):
        assert name in body, name
    assert "hipMalloc" not in body and "<<<" not in body and "SMK(" not in body
    assert body.index("chain_guide(c) != Guide::Cfg") < body.index("ensure_workspace") < body.index("run_cfg_prep")
    assert host.count("SMK(cfg_groups_table_kernel") == 1 and host.count("run_cfg_prep(c, s, d_batch, N, B)") == 2
    sample = host[host.index("int shapemol_sample("):host.index("int shapemol_log_sample_categorical(")]
    assert "run_cfg_prep(c, s, d_batch, N, B)" in sample and "run_cfg_stats(c, s, cfg_args(c, N))" in sample


def test_key_is_order_preserving():
    rs = np.random.RandomState(3)
    x = np.concatenate([rs.standard_normal(500) * np.exp(8 * rs.standard_normal(500)), [0.0, -0.0, 1e-40, -1e-40, 1e-45, -1e-45, 3e38, -3e38]]).astype(np.float32)
    k = K.key(x)
    assert np.array_equal(K.unkey(k).view(np.uint32), x.view(np.uint32))
    order = np.argsort(k, kind="stable")
    assert np.all(np.diff(x[order].astype(np.float64)) >= 0)
    assert K.key(np.float32(-0.0)) == 0x7fffffff and K.key(np.float32(0.0)) == 0x80000000
    assert K.key(np.float32(-1e-45)) == 0x7ffffffe and K.key(np.float32(1e-45)) == 0x80000001


def test_the_workgroup_counts_the_sizes_are_there_for():
    assert [K.blocks(n) for n in (1, 3, 2046, 2048, 2049, 2064, 524288, 524289, 524320, 2621445)] == [1, 1, 1, 1, 2, 2, 256, 256, 256, 256]
    got = {(N, C): (K.blocks(3 * N), K.blocks(N * C)) for N, C, _ in K.SIZES}
    assert got == {(1, 15): (1, 1), (682, 15): (1, 5), (683, 15): (2, 6), (128, 16): (1, 1), (129, 16): (1, 2),
                   (16384, 32): (24, 256), (16385, 32): (25, 256), (174763, 15): (256, 256)}
    assert 3 * 682 == 2046 and 3 * 683 == 2049 and 16 * 128 == 2048 and 32 * 16384 == 256 * 2048 and 3 * 174763 == 256 * 2048 + 1
    assert -(-32 * 16385 // 2048) == 257 and -(-3 * 174763 // 2048) == 257            # uncapped they would be 257
    assert K.quantile_rank(3, 0.5)[:2] == (1, 1) and K.quantile_rank(2, 0.5)[:2] == (0, 1)
    assert O.quantile_rank(524289, 0.4995) == K.quantile_rank(524289, 0.4995)


def case_all_equal(sorted_keys):
    return sorted_keys[0] == sorted_keys[-1]      # (the one profile whose claims stand at the generic p, ranks 0 and n - 1 included)


def _check_tensor(cond, uncond, w, ps, claims, single):
    """The references' agreement and the model for one tensor at every p of `ps`; returns {p: (relation, branch)}."""
    x = K.combine(cond, uncond, w)
    if w == 1.0:
        assert np.array_equal(x.view(np.uint32), (np.float32(2.0) * cond).view(np.uint32))
    xt = torch.from_numpy(x)
    srt = np.sort(x)            # (-0.0 and 0.0 in either order: equal under ==)
    keys = np.sort(K.key(x))
    n = len(x)
    if single:
        assert len(np.unique(keys >> 10)) == 1
    seen = {}
    by_p = {c.p: c for c in claims}
    for p in ps:
        ref = np.float32(torch.quantile(xt, p).item())
        assert same_float(ref, K.quantile_sorted(srt, p)), (p, ref, K.quantile_sorted(srt, p))
        assert same_float(ref, O.quantile(xt, p).item()), p
        k_lo, k_hi, _ = K.quantile_rank(n, p)
        rel = K.relation(keys, k_lo, k_hi)
        got, branch = K.radix_select(x, p)
        assert same_float(ref, got), (p, ref, got, branch)
        assert branch == BRANCH[rel], (p, rel, branch)
        if p in by_p:
            c = by_p[p]
            assert (k_hi == k_lo + 1 or case_all_equal(keys)) and rel == c.rel, (p, rel, c)
            assert int((keys == keys[k_lo]).sum()) == c.mult, (p, c)
            if c.rel != "same":      # k_lo is the last copy of its key
                assert keys[k_lo] != keys[k_lo + 1] and (k_lo + 1 - c.mult < 0 or keys[k_lo + 1 - c.mult] == keys[k_lo])
        seen[p] = (rel, branch)
    return seen


@pytest.mark.parametrize("case", K.QUANT, ids=[K.case_id(c) for c in K.QUANT])
def test_quantile_case_is_what_it_claims(case):
    t = K.tensors(case.profile, case.N, case.C)
    for which, n in (("pos", 3 * case.N), ("v", case.N * case.C)):
        cond, claims, single = t[which]
        assert cond.dtype == np.float32 and len(cond) == n and np.isfinite(cond).all()
        seen = _check_tensor(cond, np.zeros_like(cond), 1.0, K.p_list(claims), claims, single)
        _check_tensor(cond, K.mixed_uncond(case.profile, case.N, case.C, which), K.W_MIXED, K.P_MIXED, [], False)
        rels = {r for r, _ in seen.values()}
        want = {"ties3": {"same", "sign", "prefix"}, "allequal": {"same"}, "pairs": {"same", "digit", "prefix"}, "zeros": {"same", "sign", "prefix"},
                "sign": {"sign"}, "clustered": {"digit"}, "twoprefix": {"prefix"}}.get(case.profile, set())
        if n >= 15:
            assert want <= rels, (which, want, rels)
        if case.profile == "allequal":
            assert rels == {"same"}
        if case.profile == "clustered":
            assert "min_above" not in {b for _, b in seen.values()}


def test_the_named_profiles_hold_the_named_values():
    n = 3 * K.EDGE[0]
    two = lambda name: np.float32(2.0) * K.profile(name, n, 5)[0]      # noqa: E731
    assert set(np.unique(two("ties3")).tolist()) == {-1.5, 0.25, 3.0}
    assert np.unique(two("allequal")).tolist() == [np.float32(0.37)]
    vals, cnt = np.unique(two("pairs"), return_counts=True)
    assert len(vals) == n // 2 and set(cnt.tolist()) == {2}
    z = two("zeros")
    assert set(np.unique(z.view(np.uint32)).tolist()) == {int(np.float32(v).view(np.uint32)) for v in (0.0, -0.0)} | \
        {int((np.float32(2.0) * np.float32(v)).view(np.uint32)) for v in (1e-40, -1e-40)}
    assert 0 < abs(float(z.max())) < 1.2e-38 and (z.view(np.uint32) == 0x80000000).sum() == n // 4       # denormals, and -0.0 kept
    s = two("sign")
    assert (s < 0).sum() == n // 2 and (s > 0).sum() == n - n // 2
    w = two("wide")
    assert np.log2(np.abs(w).max() / np.abs(w).min()) > 30


@pytest.mark.parametrize("case", K.THRESH, ids=[K.case_id(c) for c in K.THRESH])
def test_threshold_case_is_what_it_claims(case):
    t = K.tensors(case.profile, case.N, case.C)
    for which in ("pos", "v"):
        cond = t[which][0]
        n, nb = len(cond), K.blocks(len(cond))
        a = np.abs(cond)
        if case.profile == "maxneg":
            e = int(np.argmax(a))
            assert cond[e] == -7.5 and (a == a.max()).sum() == 1 and a[a < 7.5].max() <= 3.0
            assert (e // 256) % nb == nb - 1 and all(((j // 256) % nb) != nb - 1 for j in range(e + 1, n))
        else:
            assert (a == a.max()).sum() > n // 6 and cond[np.argmax(a)] > 0


@pytest.mark.parametrize("case", K.RESCALE, ids=[K.case_id(c) for c in K.RESCALE])
def test_rescale_model_is_inside_the_gate(case):
    """The one-pass float64 sums in the kernels' fixed order, restated (K.strided_sums), against the two-pass float64 value
    under the device test's gate eH <= 4 e32 + 16 * 2^-24: the formula sum x^2 - (sum x)^2 / n loses nothing that matters at
    mean / spread = 1e5 and 524 320 elements."""
    t = K.tensors(case.profile, case.N, case.C)
    for which in ("pos", "v"):
        cond = t[which][0]
        for w, un in ((1.0, np.zeros_like(cond)), (K.W_MIXED, K.mixed_uncond(case.profile, case.N, case.C, which))):
            x = K.combine(cond, un, w)
            r64, e32, bound = K.rescale_gate(x, cond)
            eH = abs(float(K.rescale_model(x, cond)) - r64) / r64
            print(f"rescale_model {K.case_id(case)} {which} w={w}: eH {eH:.3e} e32 {e32:.3e} eH/bound {eH / bound:.3f}")
            assert eH <= bound, (which, w, eH, e32)
    if case.profile.startswith("offset"):
        m, s = float(np.mean(cond.astype(np.float64))), float(np.std(cond.astype(np.float64)))
        assert m / s > (4e4 if case.profile == "offset1000" else 40)


@pytest.mark.parametrize("name", list(K.GROUP_LAYOUTS))
def test_group_layout_is_what_it_claims(name):
    C, counts, group_mols, strens = K.GROUP_LAYOUTS[name]
    assert sum(group_mols) == len(counts) and len(strens) == len(group_mols)
    _, atom_off = K.group_offsets(counts, group_mols)
    atoms = np.diff(atom_off)
    assert sum(K.OTHER_LAYOUT[name]) == len(counts) and tuple(K.OTHER_LAYOUT[name]) != tuple(group_mols)
    if name.startswith("many"):
        assert len(group_mols) == K.MAX_GROUPS and set(group_mols) == {1} and atoms.min() == 1 and 0.0 in strens
        assert any(o % 2 for o in (3 * atom_off[1:-1]).tolist()) and any(o % 2 for o in (C * atom_off[1:-1]).tolist())
        return
    assert atoms[0] == 1 and atoms[1] == 128 and atoms[3] == 683 and 3 * atoms[3] == 2049
    if C == 16:
        assert C * atoms[1] == 2048
    assert strens[2] == 0.0 and strens[1] != 0.0 and strens[3] != 0.0
    assert C * atoms[4] > K.MAX_BLOCKS * K.BLOCK_ELEMS and K.blocks(int(C * atoms[4])) == 256 and K.blocks(int(3 * atoms[4])) < 256
    assert [int(3 * o) % 2 for o in atom_off[1:4]] == [1, 1, 0] and (3 * atom_off[4]) % 2 == 1
    if C == 15:
        assert sum(int(C * o) % 2 for o in atom_off[1:5]) == 3
    # the launch bound of the per-group kernels covers the groups' workgroups (cfg_group_blocks: n / 2048 + G)
    for per in (3, C):
        assert sum(K.blocks(int(per * a)) for a, w in zip(atoms, strens) if w != 0.0) <= per * atom_off[-1] // 2048 + len(group_mols)
