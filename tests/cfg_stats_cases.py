"""The cases of tests/test_gpu_cfg_stats.py and tests/test_cfg_stats_cpu.py: crafted prediction tensors for the statistic stage of
classifier-free guidance (shapemol_amd/csrc/sm_cfg.h = S), each built so that one branch of the radix select, of the fixed-order
float64 reduction or of the workgroup tables decides the answer, together with numpy restatements of what S documents: the
order-preserving key (S:93-97), the workgroup count (S:31-32), the three passes with the min-above channel and the finalize
(S:17-23), and the strided float64 partial sums (S:15-16).

Placing values: the device statistic is taken of x = (1 + w) cond - w uncond.  With w = 1 and uncond = 0, x = 2 cond exactly, so
a profile states `cond` and the combined tensor has the same key structure one exponent up.  Every profile also runs with w = 0.7
and a random uncond (W_MIXED), the combine restated in float32 as two rounded operations (`combine`).

What a rank claims (RankClaim): where the two neighbouring order statistics k_lo, k_hi of a p lie relative to each other
  same    one key (a tie spans both ranks: S:368 is false)
  digit   the same 22-bit prefix, another last digit (next_bin < 1024, S:369)
  prefix  another 22-bit prefix, the same sign (the min-above channel, S:369 `~H[3 * kCfgBins]`, S:333-340)
  sign    k_lo negative, k_hi not (adjacent or not, the keys differ in the top bit, so in every prefix; min-above channel)
and the multiplicity of k_lo's key.  tests/test_cfg_stats_cpu.py asserts every claim from the data."""
import math
import zlib
from collections import namedtuple

import numpy as np

BLOCK_ELEMS, MAX_BLOCKS, BINS, MAX_GROUPS = 2048, 256, 2048, 256      # S:31, kCfgMaxBlocks, kCfgBins, kCfgMaxGroups
P_GENERIC = (0.0, 1.0, 0.5, 0.4995, 0.995, 0.123456)
P_MIXED = (0.4995, 0.995)      # the p of the w = 0.7 runs
W_MIXED = 0.7

RankClaim = namedtuple("RankClaim", "p rel mult")
Quant = namedtuple("Quant", "profile N C reason")
Thresh = namedtuple("Thresh", "profile N C reason")
Rescale = namedtuple("Rescale", "profile N C reason")


# ---------------------------------------------------------------------------------------------- restatements of S
def key(x):
    """cfg_key (S:93-96) of a float32 array: uint32 keys with key(a) < key(b) <=> a < b, -0.0 below +0.0."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def blocks(n):
    """Workgroups of a tensor (or of one group's slice) of n elements: S:31-32, cfg_args."""
    return min(MAX_BLOCKS, max(1, -(-n // BLOCK_ELEMS)))


def quantile_rank(n, p):
    """torch.quantile's rank: float32(p) * float32(n - 1) in float32, its floor and ceil, the float32 weight."""
    r = np.float32(np.float32(p) * np.float32(n - 1))
    lo, hi = int(r), int(math.ceil(float(r)))
    return lo, hi, np.float32(r - np.float32(lo))


def p_for_rank(n, k):
    """A p whose rank lies strictly between k and k + 1: k_lo = k, k_hi = k + 1."""
    p = (k + 0.5) / (n - 1)
    assert quantile_rank(n, p)[:2] == (k, k + 1), (n, k)
    return p


def _fma32(a, b, c):
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))       # (the float64 product of two float32 is exact)


def lerp32(a, b, w):
    """torch.lerp in float32: one fused multiply-add in the branch |weight| < 0.5, the other form otherwise."""
    a, b, w = np.float32(a), np.float32(b), np.float32(w)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.float32(b - a)
        return _fma32(w, d, a) if abs(w) < 0.5 else _fma32(-d, np.float32(1.0) - w, b)


def quantile_sorted(srt, p):
    """The independent sort-and-lerp restatement of torch.quantile(x, p) on the sorted float32 values."""
    lo, hi, w = quantile_rank(len(srt), p)
    return lerp32(srt[lo], srt[hi], w)


def combine(cond, uncond, w):
    """(1 + w) cond - w uncond in float32: the scalars rounded once, two rounded products, one rounded difference, no FMA."""
    w1, wf = np.float32(1.0 + w), np.float32(w)
    return (w1 * cond.astype(np.float32)).astype(np.float32) - (wf * uncond.astype(np.float32)).astype(np.float32)


def _find_digit(h, krem):
    """cfg_find_digit (S:269-299): the bin that holds rank krem, the rank left inside it, its count."""
    cum = np.cumsum(h.astype(np.int64))
    d = int(np.searchsorted(cum, krem, side="right"))
    return d, int(krem - (cum[d - 1] if d else 0)), int(h[d])


def radix_select(x, p):
    """The three passes (11, 11, 10 bits), the min-above channel and the finalize of S:301-378 on the combined float32 values x.
    Returns (statistic, branch): branch is 'same' | 'next_bin' | 'min_above', the arm of S:368-369 that chose key_hi."""
    k = key(x)
    k_lo, k_hi, weight = quantile_rank(len(k), p)
    h0 = np.bincount(k >> 21, minlength=BINS)
    d0, krem, _ = _find_digit(h0, k_lo)
    sel = k[(k >> 21) == d0]
    h1 = np.bincount((sel >> 10) & 2047, minlength=BINS)
    d1, krem, _ = _find_digit(h1, krem)
    prefix = (d0 << 11) | d1
    top = k >> 10
    h2 = np.bincount(k[top == prefix] & 1023, minlength=BINS)
    above = k[top > prefix]
    min_above_inv = int((~above).max()) if len(above) else 0       # atomicMax of ~key (S:333, S:340)
    d2, krem, cnt = _find_digit(h2, krem)
    key_lo = (prefix << 10) | d2
    key_hi, branch = key_lo, "same"
    if k_hi != k_lo and krem + 1 >= cnt:
        nxt = np.nonzero(h2[d2 + 1:1024])[0]
        if len(nxt):
            key_hi, branch = (prefix << 10) | (d2 + 1 + int(nxt[0])), "next_bin"
        else:
            key_hi, branch = (~np.uint32(min_above_inv)) & np.uint32(0xffffffff), "min_above"
    lo, hi = unkey(np.uint32(key_lo)), unkey(np.uint32(key_hi))
    return lerp32(lo, hi, weight), branch


def strided_sums(vals):
    """The fixed-order float64 sum of cfg_partial_kernel and cfg_finalize_kernel (S:241-267, S:379-393) of float64 `vals`:
    thread t of workgroup b adds elements b * 256 + t + i * nblk * 256 in order of i, a 256-lane halving tree per workgroup,
    then one partial per lane of the final workgroup and the same tree."""
    n, nb = len(vals), blocks(len(vals))
    step = nb * 256
    pad = np.zeros(-(-n // step) * step, dtype=np.float64)
    pad[:n] = vals
    acc = np.zeros(step, dtype=np.float64)
    for row in pad.reshape(-1, step):
        acc = acc + row

    def tree(a):
        a = a.copy()
        h = 128
        while h:
            a[..., :h] = a[..., :h] + a[..., h:2 * h]
            h >>= 1
        return a[..., 0]
    part = np.zeros(256, dtype=np.float64)
    part[:nb] = tree(acc.reshape(nb, 256))
    return float(tree(part))


def rescale_model(x, cond):
    """r = float32(std(cond)) / float32(std(x)) from the one-pass float64 sums of S:398-403."""
    out = []
    for v in (cond, x):
        d = v.astype(np.float64)
        n = float(len(d))
        s, ss = strided_sums(d), strided_sums(d * d)
        var = (ss - s * s / n) / (n - 1.0)
        out.append(np.float32(math.sqrt(max(var, 0.0))))
    return np.float32(out[0] / out[1])


def rescale_gate(x, cond):
    """(r64, e32, bound): the float64 two-pass unbiased ratio, the relative error of CPU float32 torch.std(cond) / torch.std(x)
    against it, and the project's gate 4 e32 + 16 * 2^-24."""
    import torch
    r64 = float(np.std(cond.astype(np.float64), ddof=1) / np.std(x.astype(np.float64), ddof=1))
    r32 = float((torch.std(torch.from_numpy(cond)) / torch.std(torch.from_numpy(x))).item())
    e32 = abs(r32 - r64) / r64
    return r64, e32, 4.0 * e32 + 16.0 * 2.0 ** -24


def relation(srt_keys, k_lo, k_hi):
    a, b = int(srt_keys[k_lo]), int(srt_keys[k_hi])
    if a == b:
        return "same"
    if (a >> 31) != (b >> 31):
        return "sign"
    return "digit" if (a >> 10) == (b >> 10) else "prefix"


# ---------------------------------------------------------------------------------------------- profiles
def seed_of(*parts):
    return zlib.crc32("-".join(str(p) for p in parts).encode()) & 0x7fffffff


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _bits(b):
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


def profile(name, n, seed):
    """(cond float32 (n,), [RankClaim], single_prefix): the conditional values of one tensor -- the combined tensor of the exact
    runs is 2 * cond -- the ranks the profile is there for, and whether all keys share one 22-bit prefix."""
    rs = np.random.RandomState(seed)
    claims, single = [], False
    if name == "natural":
        cond = rs.standard_normal(n)
    elif name == "wide":
        cond = rs.standard_normal(n) * np.exp(4.0 * rs.standard_normal(n))
    elif name == "offset50":
        cond = 50.0 + rs.standard_normal(n)
    elif name == "offset1000":
        cond = 1000.0 + 0.01 * rs.standard_normal(n)
    elif name == "allequal":
        cond = np.full(n, 0.185)
        claims = [RankClaim(p, "same", n) for p in P_GENERIC]
    elif name == "ties3":
        idx = rs.randint(0, 3, n)
        idx[:3] = [0, 1, 2][:n]
        cond = np.array([-0.75, 0.125, 1.5])[idx]
        c0, c1 = int((idx == 0).sum()), int((idx == 1).sum())
        claims = [RankClaim(p_for_rank(n, c0 - 1), "sign", c0), RankClaim(p_for_rank(n, c0 + c1 - 1), "prefix", c1)]
    elif name == "pairs":
        assert n % 2 == 0 and n >= 1400
        m = n // 2
        cond = _bits(np.uint32(0x3f800000) + 3 * np.repeat(np.arange(m, dtype=np.uint32), 2))      # 1 + 3 j ulp, each twice
        inside = next(j for j in range(m // 3, m) if (3 * j) % 1024 < 1020)       # j and j + 1 in one 22-bit prefix
        across = next(j for j in range(m // 3, m) if (3 * j) % 1024 >= 1021)      # j + 1 in the next one
        claims = [RankClaim(p_for_rank(n, 2 * inside), "same", 2), RankClaim(p_for_rank(n, 2 * inside + 1), "digit", 2),
                  RankClaim(p_for_rank(n, 2 * across + 1), "prefix", 2)]
    elif name == "zeros":
        assert n >= 8
        q = n // 4
        cond = np.concatenate([np.full(q, -1e-40), np.full(q, -0.0), np.full(q, 0.0), np.full(n - 3 * q, 1e-40)])
        claims = [RankClaim(p_for_rank(n, q - 1), "prefix", q), RankClaim(p_for_rank(n, 2 * q - 1), "sign", q),
                  RankClaim(p_for_rank(n, 3 * q - 1), "prefix", q), RankClaim(p_for_rank(n, q), "same", q),
                  RankClaim(p_for_rank(n, 2 * q), "same", q)]
    elif name == "sign":
        assert n >= 4
        mag = np.abs(rs.standard_normal(n)) + 0.01
        cond = np.where(np.arange(n) < n // 2, -mag, mag)
        claims = [RankClaim(p_for_rank(n, n // 2 - 1), "sign", 1)]
    elif name == "clustered":
        assert n >= 8
        digits = rs.randint(0, 1024, n).astype(np.uint32)
        cond = _bits(np.uint32(0x3f800000) + digits)
        srt = np.sort(digits)
        mid = int(srt[n // 2]) if srt[n // 2] != srt[-1] else int(srt[0])
        last = int(np.searchsorted(srt, mid, side="right")) - 1
        claims = [RankClaim(p_for_rank(n, last), "digit", int((srt == mid).sum()))]
        single = True
    elif name == "twoprefix":
        assert n >= 16
        nb, na = n // 4, n // 4
        below = -np.abs(rs.standard_normal(nb)) - 1.0
        a = _bits(np.uint32(0x3f800000) + np.concatenate([rs.randint(0, 1000, na), [1023]]).astype(np.uint32))       # 1.0 ..: one prefix, a unique largest key
        b = np.concatenate([[8.0], 8.5 + 10.0 * np.abs(rs.standard_normal(n - nb - na - 2))])                        # a unique smallest key, others above
        cond = np.concatenate([below, a.astype(np.float64), b])
        claims = [RankClaim(p_for_rank(n, nb + na), "prefix", 1)]
    else:
        raise KeyError(name)
    cond = _f32(cond)
    return cond[rs.permutation(n)], claims, single


def tail_of_last_workgroup(n):
    """The last element the last workgroup of a tensor of n elements reads (S:246: e = local * 256 + t + i * nblk * 256)."""
    nb = blocks(n)
    e = np.arange(n)
    return int(e[(e // 256) % nb == nb - 1][-1])


def maxneg(n, seed):
    """reference_threshold: normal values clipped to [-3, 3] and one -7.5, the largest magnitude, at the tail of the last workgroup."""
    cond = np.clip(np.random.RandomState(seed).standard_normal(n), -3.0, 3.0)
    cond[tail_of_last_workgroup(n)] = -7.5
    return _f32(cond)


def tensors(name, N, C, tag=""):
    """Both prediction tensors of a case, each with its own draw of the profile: {'pos': (cond, claims, single), 'v': ...}."""
    out = {}
    for which, n in (("pos", 3 * N), ("v", N * C)):
        seed = seed_of(name, N, C, which, tag)
        out[which] = (maxneg(n, seed), [], False) if name == "maxneg" else profile(name, n, seed)
    return out


def mixed_uncond(name, N, C, which, tag=""):
    """The random uncond of the w = 0.7 runs: another draw of the offset profiles (the combination keeps its offset mean), a
    standard normal otherwise."""
    n = (3 if which == "pos" else C) * N
    seed = seed_of(name, N, C, which, tag, "uncond")
    if name.startswith("offset"):
        return profile(name, n, seed)[0]
    return _f32(np.random.RandomState(seed).standard_normal(n))


# ---------------------------------------------------------------------------------------------- cases
# Sizes: positions have 3 N elements, logits N C.  EDGE: a profile's own ranks at a few thousand elements (even counts for
# `pairs`): positions 2052 (two workgroups), logits 10260 (six).
EDGE = (684, 15)
SIZES = [
    (1, 15, "one atom: 3 and 15 elements, one workgroup with 253 | 241 idle lanes, ranks 0..2"),
    (682, 15, "positions 2046: the last element count with one workgroup"),
    (683, 15, "positions 2049: a second workgroup with one element"),
    (128, 16, "logits exactly 2048: one full workgroup"),
    (129, 16, "logits 2064: a second workgroup of 16 elements"),
    (16384, 32, "logits 524 288: exactly kCfgMaxBlocks = 256 workgroups of 2048"),
    (16385, 32, "logits 524 320: above the cap, the stride nblk * 256 wraps a ninth time for 32 elements"),
    (174763, 15, "positions 524 289: one element above the cap (logits 2.6 M: 40 rounds of the capped stride)"),
]
QUANT = ([Quant(p, *EDGE, "the profile's own ranks") for p in ("ties3", "allequal", "pairs", "zeros", "sign", "wide", "clustered", "twoprefix", "natural")]
         + [Quant(p, N, C, why) for N, C, why in SIZES for p in ("wide", "ties3")])
THRESH = ([Thresh("ties3", *EDGE, "the largest magnitude many times, in every workgroup")]
          + [Thresh("maxneg", N, C, "a single negative largest magnitude at the tail of the last workgroup; " + why)
             for N, C, why in [(684, 15, "two | six workgroups")] + SIZES[5:]])
RESCALE_SIZES = [(683, 15, "small: 2 | 6 workgroups"), (16385, 32, "logits above the cap: 256 partials in the final reduction")]
RESCALE = [Rescale(p, N, C, why) for p in ("natural", "wide", "offset50", "offset1000") for N, C, why in RESCALE_SIZES]


def case_id(c):
    return f"{c.profile}-n{c.N}-c{c.C}"


def p_list(claims):
    """The generic p and the case's own, each once."""
    out = list(P_GENERIC)
    for c in claims:
        if c.p not in out:
            out.append(c.p)
    return out


# ---------------------------------------------------------------------------------------------- groups
def _layout(C, cap_atoms):
    """(atoms per molecule, molecules per group, strengths): a single-atom group, 128 atoms (2048 logits at C = 16), a w_g = 0
    group between guided ones, 683 atoms (2049 coordinates), a group above the cap, a small last one.  Atom offsets 1, 129, 134,
    817: the coordinate ranges start at elements 3, 387, 402, 2451 and (C = 15) the logit ranges at 15, 1935, 2010, 12255."""
    counts = [1, 60, 68, 2, 3, 683, cap_atoms, 7, 9]
    return counts, (1, 2, 2, 1, 1, 2), (0.7, 1.5, 0.0, 0.9, 1.1, 0.3)


def _many(C):
    """kCfgMaxGroups groups of one molecule each, 1..40 atoms."""
    counts = (1 + np.random.RandomState(seed_of("many", C)).randint(0, 40, MAX_GROUPS)).tolist()
    strens = tuple(0.0 if g % 37 == 5 else 0.3 + 0.01 * g for g in range(MAX_GROUPS))
    return counts, (1,) * MAX_GROUPS, strens


GROUP_LAYOUTS = {
    "edges-c16": (16, *_layout(16, 32769)),        # 32769 atoms: 524 304 logits, one workgroup round above the cap
    "edges-c15": (15, *_layout(15, 34953)),        # 34953 atoms: 524 295 logits
    "many-c15": (15, *_many(15)),
}
# the layout a second call runs over the histograms of: the same atoms, other group boundaries
OTHER_LAYOUT = {"edges-c16": (2, 1, 3, 2, 1), "edges-c15": (2, 1, 3, 2, 1), "many-c15": (3,) * 85 + (1,)}
GROUP_P = {"reference_threshold": (1.05,), "dynamic_threshold": (0.4995, 0.995, 0.0), "rescale": (0.6,)}


def group_offsets(counts, group_mols):
    """(molecule offsets, atom offsets) of the groups."""
    mol_off = np.concatenate([[0], np.cumsum(group_mols)]).astype(np.int64)
    return mol_off, np.concatenate([[0], np.cumsum(counts)])[mol_off].astype(np.int64)
