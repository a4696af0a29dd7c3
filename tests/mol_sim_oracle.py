"""numpy float64 restatement of the Gaussian similarity and the overlay (csrc/sm_mol_sim.h), the stored
results of the reference (tests/golden/mol_sim.npz, written by tests/golden/make_golden_mol_sim.py) and the molecules the
tests of both machines share.  Element by element the expressions are the kernel's; sums are numpy's (pairwise), where the
kernel adds in its own fixed order: that difference is what the summation bound covers."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "mol_sim.npz")
GAUSS_JSON = os.path.join(HERE, "golden", "mol_sim_gaussint.json")

WAVE_ATOMS, MAX_ATOMS, MAX_TERMS, MAX_STARTS, MAX_ITER, MAX_PAIRS = 64, 256, 16, 5, 10000, 1 << 22
PI15 = float.fromhex("0x1.645f7c63f2c6bp+2")             # np.pi ** 1.5
STEP_MAX, ARMIJO, HALVINGS, SWEEPS = 0.5, 1e-4, 30, 12
GTOL, ITER_CAP = 1e-6, 200                               # the package's defaults
EPS = 2.0 ** -52
# The overlay tolerance on a Tanimoto score: 10 x the oracle's own largest disagreement between a case and its rigidly moved
# copy over overlay_cases(), measured by tests/test_mol_sim_cpu.py::test_overlay_tolerance (profiles/mol_sim/README.md).
# The measured value is 11 * 2^-53: scores near 1 are spaced 2^-53 apart, and the test that re-measures it allows one such step.
OVERLAY_MEASURED = 11 * 2.0 ** -53                       # 1.2212453270876722e-15
OVERLAY_TOL = 10 * OVERLAY_MEASURED
# The winning start is compared wherever the oracle's best and second-best start differ by more than 100 x the overlay tolerance.
START_GAP = 100 * OVERLAY_TOL
STATIONARITY_MARGIN = 2.0                                # the oracle's gradient at the device's pose: <= margin * gtol * scale


def load_golden():
    return dict(np.load(GOLDEN, allow_pickle=False))


def gaussint_terms():
    """(A_k, B_k) of the library's convention from the stored GaussInt tables: A = a, B = -b."""
    with open(GAUSS_JSON) as f:
        d = json.load(f)
    return np.array(d["a"], np.float64).reshape(-1), -np.array(d["b"], np.float64).reshape(-1)


def r2_of(x, y):
    d = x[:, None, :] - y[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], d


def shape_coefficients(ax, px, ay, py, float32=False):
    """A (nx, ny), B (nx, ny) of the shape mode; ``float32``: formed as get_ROCS forms them, from float32 tensors."""
    if float32:
        ax, px, ay, py = (np.asarray(v, np.float32) for v in (ax, px, ay, py))
        s = ax[:, None] + ay[None, :]
        num = (np.float32(PI15) * (px[:, None] * py[None, :])).astype(np.float32)
        A = num.astype(np.float64) / (s ** np.float32(1.5)).astype(np.float64)
        return A, ((ax[:, None] * ay[None, :]) / s).astype(np.float64)
    s = ax[:, None] + ay[None, :]
    return (PI15 * (px[:, None] * py[None, :])) / (s * np.sqrt(s)), (ax[:, None] * ay[None, :]) / s


def shape_integral(x, y, ax, px, ay, py, float32=False):
    """(S_xy, sum |term|, number of terms)."""
    A, B = shape_coefficients(ax, px, ay, py, float32)
    r2, _ = r2_of(x, y)
    term = A * np.exp(-(B * r2))
    return term.sum(), np.abs(term).sum(), term.size


def esp_integral(x, y, wx, wy, cA, cB):
    r2, _ = r2_of(x, y)
    t = cA[:, None, None] * np.exp(-(cB[:, None, None] * r2[None]))
    ww = wx[:, None] * wy[None, :]
    return (t.sum(0) * ww).sum(), (np.abs(t) * np.abs(ww)[None]).sum(), t.size


def bound(n_terms, sum_abs):
    """The float64 summation bound plus a few ulp per exp."""
    return (n_terms + 16) * EPS * sum_abs


def metric(name, saa, sbb, sab):
    """(score, zero-denominator flag) by the stated IEEE expressions."""
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt(saa * sbb) if name == "carbo" else (saa + sbb) - sab
        return (np.where(den == 0, np.nan, sab / np.where(den == 0, 1.0, den)), den == 0)


def tanimoto_bound(saa, sbb, sab, baa, bbb, bab):
    """First-order bound on the Tanimoto score's error from the three integrals' bounds, plus 4 ulp for its own operations."""
    den = (saa + sbb) - sab
    return (bab * (saa + sbb) + (baa + bbb) * abs(sab)) / (den * den) * 1.01 + 4 * EPS


# ---- the overlay ----------------------------------------------------------------------------------------------------------------
def frame(m):
    """csrc/sm_mol_sim.h msim_frame: m = xx, yy, zz, xy, xz, yz of a symmetric matrix -> (3, 3) right-handed eigenvector frame."""
    A = np.array([[m[0], m[3], m[4]], [m[3], m[1], m[5]], [m[4], m[5], m[2]]], np.float64)
    E = np.eye(3)
    for _ in range(SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[p, q]
            if apq == 0.0:
                continue
            with np.errstate(over="ignore"):
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                tt = (-1.0 if theta < 0.0 else 1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
            c = 1.0 / np.sqrt(tt * tt + 1.0)
            s = tt * c
            for M, cols in ((A, True), (A, False), (E, True)):
                if cols:
                    x, y = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = c * x - s * y, s * x + c * y
                else:
                    x, y = M[p, :].copy(), M[q, :].copy()
                    M[p, :], M[q, :] = c * x - s * y, s * x + c * y
            A[p, q] = A[q, p] = 0.0
    d = [A[0, 0], A[1, 1], A[2, 2]]
    order = sorted(range(3), key=lambda k: (d[k], k))
    c0, c1 = E[:, order[0]], E[:, order[1]]
    return np.stack([c0, c1, np.cross(c0, c1)], 1), np.array([d[k] for k in order])


def inertia(p0):
    r2 = (p0 * p0).sum(1)
    return np.array([(r2 - p0[:, 0] ** 2).sum(), (r2 - p0[:, 1] ** 2).sum(), (r2 - p0[:, 2] ** 2).sum(),
                     -(p0[:, 0] * p0[:, 1]).sum(), -(p0[:, 0] * p0[:, 2]).sum(), -(p0[:, 1] * p0[:, 2]).sum()])


def moments(pos):
    """Ascending principal moments of the unit-weight inertia tensor."""
    return frame(inertia(pos - pos.mean(0)))[1]


def well_posed(pos, ratio=1.2):
    m = moments(pos)
    return bool(m[0] > 0 and m[1] >= ratio * m[0] and m[2] >= ratio * m[1])


START_SIGNS = ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))


def rotate(w, R):
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    ka, kb = (np.sin(th) / th, (1.0 - np.cos(th)) / th2) if th > 1e-8 else (1.0, 0.5)
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return ((np.eye(3) + ka * W) + kb * (W @ W)) @ R


def value_gradient(R, u, a0, b0, A, B):
    """S_ab at y = R a0 + u and its derivative by (u, rotation about u)."""
    lever = a0 @ R.T
    r2, d = r2_of(lever + u, b0)
    term = A * np.exp(-(B * r2))
    force = (((-2.0 * B) * term)[..., None] * d).sum(1)
    return term.sum(), np.concatenate([force.sum(0), np.cross(lever, force).sum(0)])


def optimise(R, u, a0, b0, A, B, stop, max_iter):
    """BFGS as the kernel runs it.  -> S_ab, R, u, iterations, converged, moved"""
    f, g = value_gradient(R, u, a0, b0, A, B)
    H = np.eye(6)
    scaled, identity, moved, it, converged = False, True, False, 0, False
    while True:
        if np.isnan(f) or np.isnan(g).any():                 # a NaN pose is never converged
            break
        if np.abs(g).max() <= stop:
            converged = True
            break
        if it >= max_iter:
            break
        it += 1
        d = H @ g
        gd = g @ d
        if not gd > 0.0:
            H, d, gd, scaled, identity = np.eye(6), g.copy(), g @ g, False, True
        dmax = np.abs(d).max()
        if dmax > STEP_MAX:
            d, gd = d * (STEP_MAX / dmax), gd * (STEP_MAX / dmax)
        step, accepted = 1.0, False
        for _ in range(HALVINGS + 1):
            s = step * d
            un, Rn = u + s[:3], rotate(s[3:], R)
            fn, gn = value_gradient(Rn, un, a0, b0, A, B)
            if fn >= f + ARMIJO * step * gd:
                accepted = True
                break
            step *= 0.5
        if not accepted:
            if identity:
                break
            H, scaled, identity = np.eye(6), False, True
            continue
        y = g - gn
        sy, yy, ss = s @ y, y @ y, s @ s
        if sy > 1e-10 * np.sqrt(ss * yy):
            if not scaled:
                H, scaled = np.eye(6) * (sy / yy), True
            Hy = H @ y
            rho = 1.0 / sy
            H = (H - rho * (np.outer(s, Hy) + np.outer(Hy, s))) + ((rho * rho) * (y @ Hy) + rho) * np.outer(s, s)
            identity = False
        f, g, R, u, moved = fn, gn, Rn, un, True
    return f, R, u, it, converged, moved


def apply(R, t, x):
    """The kernel's x' = ((R0 x + R1 y) + R2 z) + t, row by row, without fused operations."""
    return np.stack([((R[k, 0] * x[:, 0] + R[k, 1] * x[:, 1]) + R[k, 2] * x[:, 2]) + t[k] for k in range(3)], 1)


def align(a, b, alpha_a, p_a, alpha_b, p_b, include_given=False, max_iter=ITER_CAP, gtol=GTOL):
    """The overlay of one pair.  -> dict(tanimoto, start, rot, trans, iterations, converged, aligned, s_aa, s_bb, s_ab,
    start_scores: the Tanimoto of every start's end pose)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    saa = shape_integral(a, a, alpha_a, p_a, alpha_a, p_a)[0]
    sbb = shape_integral(b, b, alpha_b, p_b, alpha_b, p_b)[0]
    A, B = shape_coefficients(alpha_a, p_a, alpha_b, p_b)
    ca, cb = a.sum(0) / len(a), b.sum(0) / len(b)
    a0, b0 = a - ca, b - cb
    Va, Vb = frame(inertia(a0))[0], frame(inertia(b0))[0]
    stop = gtol * (0.5 * (saa + sbb))
    res = []
    for k in range(4 + bool(include_given)):
        R, u = (Vb @ np.diag(START_SIGNS[k]) @ Va.T, np.zeros(3)) if k < 4 else (np.eye(3), ca - cb)
        f, R, u, it, conv, moved = optimise(R, u, a0, b0, A, B, stop, max_iter)
        if k == 4 and not moved:
            R, t = np.eye(3), np.zeros(3)
        else:
            t = (u + cb) - R @ ca
        res.append((f, R, t, it, conv, moved))
    fs = np.array([r[0] for r in res])
    best = 0
    for k in range(1, len(res)):
        if fs[k] > fs[best] or (np.isnan(fs[best]) and not np.isnan(fs[k])):
            best = k
    f, R, t, it, conv, _ = res[best]
    aligned = apply(R, t, a)
    sab = shape_integral(aligned, b, alpha_a, p_a, alpha_b, p_b)[0]
    if include_given:
        sg = shape_integral(a, b, alpha_a, p_a, alpha_b, p_b)[0]
        if sg > sab or (np.isnan(sab) and not np.isnan(sg)):
            # the flag of the pose returned: start 4's own when it never left the pose as given, else not converged
            best, R, t, it, conv, aligned, sab = 4, np.eye(3), np.zeros(3), 0, res[4][4] and not res[4][5], a.copy(), sg
    return dict(tanimoto=float(metric("tanimoto", saa, sbb, sab)[0]), start=best, rot=R, trans=t, iterations=it, converged=bool(conv), aligned=aligned,
                s_aa=saa, s_bb=sbb, s_ab=sab, start_scores=np.array([float(metric("tanimoto", saa, sbb, x)[0]) for x in fs]))


def pose_gradient(aligned, b, alpha_a, p_a, alpha_b, p_b):
    """Largest component of the derivative of S_ab by a rigid motion of `aligned` (translation, rotation about its centroid),
    and the scale (S_aa + S_bb) / 2 of the stopping rule."""
    A, B = shape_coefficients(alpha_a, p_a, alpha_b, p_b)
    c = aligned.mean(0)
    _, g = value_gradient(np.eye(3), c, aligned - c, b, A, B)
    saa = shape_integral(aligned, aligned, alpha_a, p_a, alpha_a, p_a)[0]
    sbb = shape_integral(b, b, alpha_b, p_b, alpha_b, p_b)[0]
    return float(np.abs(g).max()), 0.5 * (saa + sbb)


# ---- molecules of the tests -------------------------------------------------------------------------------------------------------
def walk(rng, n, lo=1.1, hi=1.6):
    """A random walk with steps of lo..hi Angstrom."""
    u = rng.standard_normal((n, 3))
    u *= (rng.uniform(lo, hi, n) / np.linalg.norm(u, axis=1))[:, None]
    return np.cumsum(u, 0)


def walk_well_posed(rng, n):
    """The first walk of the generator whose adjacent principal moments differ by a factor of 1.2 (n >= 3)."""
    while True:
        p = walk(rng, n)
        if n < 3 or well_posed(p):
            return p


def random_rotation(rng, max_angle=np.pi):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    return rotate(axis * rng.uniform(0.3, max_angle), np.eye(3))


def moved(rng, pos, shift=5.0):
    R = random_rotation(rng)
    return pos @ R.T + rng.uniform(-shift, shift, 3), R


def overlay_cases():
    """The overlay cases both test files use: name -> (a, b) with b the condition.  'copy*': a is a rigidly moved copy of b
    (a permuted one for 'copy-perm*'); 'pair*': two different molecules; sizes cover 1, 2, 3, 63, 64, 65, 255, 256 atoms and
    both launch forms."""
    rng = np.random.default_rng(20261021)
    cases = {}
    for n in (1, 2, 3, 17, 63, 64, 65, 255, 256):
        b = walk_well_posed(rng, n)
        cases[f"copy{n}"] = (moved(rng, b)[0], b)
    for n in (24, 65):
        b = walk_well_posed(rng, n)
        cases[f"copy-perm{n}"] = (moved(rng, b)[0][rng.permutation(n)], b)
    for na, nb in ((3, 5), (12, 9), (22, 27), (30, 24), (63, 40), (64, 64), (40, 65), (65, 63), (100, 256)):
        cases[f"pair{na}x{nb}"] = (walk_well_posed(rng, na) + rng.uniform(-3, 3, 3), walk_well_posed(rng, nb))
    return cases


def rocs_parameters(n, alpha=0.81, prefactor=0.8):
    return np.full(n, alpha, np.float64), np.full(n, prefactor, np.float64)
