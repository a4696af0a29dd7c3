"""Shape and electrostatic similarity of molecules on the device, and the rigid overlay that scores a sample against its
shape condition.

The reference scores a sample by writing two ``.mol`` files, running the closed ShaEP executable for a rigid overlay, reading
an SDF back and scoring the aligned pose with ``get_ROCS`` (utils/evaluation/similarity.py ``calculate_shaep_shape_sim``,
shaep_utils.py); its electrostatic companion is espsim's ``GetIntegralsViaGaussians``.  Here the scoring functions are kernels
(csrc/sm_mol_sim.h): ``shape_tanimoto`` / ``get_rocs`` / ``esp_similarity`` are the reference's
functions at a fixed pose, batched over pairs of molecules, and agree with them to the float64 summation bound.
``align_shapes`` is the overlay.  ShaEP is not available, so THE OVERLAY RULE IS THIS PACKAGE'S OWN: principal-frame starts
and a BFGS ascent of the same Gaussian shape overlap that ``get_ROCS`` scores.  Agreement with ShaEP's poses has not been
measured and is not claimed.

Molecule sets: one ``(n, 3)`` array (one molecule) or a list of them; per-atom parameters likewise.  Pairs: 1-to-1 for sets of
equal length, N-to-1 or 1-to-N when one set has a single molecule, ``pairs="all"`` or an explicit ``(P, 2)`` index array.
The coefficient tables of ``esp_similarity`` are data the caller passes; the package ships none.

Limits (``ValueError`` before any kernel runs): 1..256 atoms per molecule, at most 16 Gaussian terms, finite parameters,
widths > 0, pair indices inside their sets.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._native import DeviceContexts, hip_device, host, ptr, stream_ptr

FORMS = ("wave", "block")
METRICS = {"tanimoto": 0, "carbo": 1}
Sizes = collections.namedtuple("Sizes", "wave_atoms max_atoms max_terms max_starts max_iter max_pairs")
GIVEN_START = 4


def sizes():
    """The library's limits (shapemol_sim_sizes; the constants of csrc/sm_mol_sim.h)."""
    out = (C.c_int64 * 6)()
    _lib.load().shapemol_sim_sizes(out, 6)
    return Sizes(*out)


_contexts = DeviceContexts("shapemol_sim_create", "shapemol_sim_destroy")


def _debug_fill(device, byte):
    """Tests only: fill the context's device workspaces."""
    _lib.check(_lib.load().shapemol_sim_debug_fill(_contexts.of(device), int(byte), stream_ptr(device)), "shapemol_sim_debug_fill")


class _Set:
    """A packed set of molecules: ``pos`` (N, 3) float64 (a tensor, moved to the device by the call), ``off`` (M + 1) int64,
    per-atom ``u`` and ``v`` float64 host arrays."""

    def __init__(self, name, centers, u, v):
        mols = list(centers) if isinstance(centers, (list, tuple)) else [centers]
        if not mols:
            raise ValueError(f"molecule similarity: set {name} is empty")
        mols = [m if isinstance(m, torch.Tensor) else torch.as_tensor(host(m)) for m in mols]
        for k, m in enumerate(mols):
            if m.dim() != 2 or m.shape[1] != 3:
                raise ValueError(f"molecule similarity: molecule {k} of set {name} must be (n, 3), got {tuple(m.shape)}")
        ns = [int(m.shape[0]) for m in mols]
        self.n = np.array(ns, np.int64)
        self.off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        self.pos = torch.cat([m.to(torch.float64) for m in mols]) if len(mols) > 1 else mols[0].to(torch.float64)
        self.u, self.v = self._param(name, u, ns), self._param(name, v, ns)

    @staticmethod
    def _param(name, value, ns):
        if value is None:
            return None
        N = sum(ns)
        if isinstance(value, (list, tuple)) and len(value) == len(ns) and all(np.ndim(host(x)) == 1 for x in value):
            value = np.concatenate([host(x, np.float64) for x in value]) if len(value) else np.zeros(0)
        value = host(value, np.float64).reshape(-1)
        if value.size == 1 and N != 1:
            value = np.full(N, float(value[0]))
        if value.size != N:
            raise ValueError(f"molecule similarity: set {name} has {N} atoms and {value.size} per-atom parameters")
        return np.ascontiguousarray(value, np.float64)


def _pairs(pairs, Ma, Mb):
    if pairs is None:
        if Ma == Mb:
            pairs = np.stack([np.arange(Ma), np.arange(Mb)], 1)
        elif Mb == 1:
            pairs = np.stack([np.arange(Ma), np.zeros(Ma, np.int64)], 1)
        elif Ma == 1:
            pairs = np.stack([np.zeros(Mb, np.int64), np.arange(Mb)], 1)
        else:
            raise ValueError(f"molecule similarity: sets of {Ma} and {Mb} molecules need an explicit pair list (or pairs='all')")
    elif isinstance(pairs, str):
        if pairs != "all":
            raise ValueError(f"molecule similarity: unknown pair rule {pairs!r}")
        pairs = np.stack(np.meshgrid(np.arange(Ma), np.arange(Mb), indexing="ij"), -1).reshape(-1, 2)
    pairs = host(pairs)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in "iu":
        raise ValueError("molecule similarity: pairs must be a (P, 2) integer array")
    return np.ascontiguousarray(pairs, np.int64)


def _check(mode, a, b, pairs, terms):
    cA, cB = terms if terms is not None else (None, None)
    forms = np.zeros(len(pairs), np.int32)
    lib = _lib.load()
    if lib.shapemol_sim_check(mode, len(a.n), ptr(a.off), ptr(a.u), ptr(a.v), len(b.n), ptr(b.off), ptr(b.u), ptr(b.v), len(pairs), ptr(pairs),
                              0 if cA is None else len(cA), ptr(cA), ptr(cB), ptr(forms)):
        raise ValueError(lib.shapemol_last_error().decode())
    return forms


def _device(device, *sets):
    if device is None:
        on = [s.pos.device for s in sets if s.pos.is_cuda]
        device = on[0] if on else "cuda" if torch.cuda.is_available() else "cpu"
    device = hip_device(device, "molecule similarity runs on a HIP device")
    for s in sets:
        s.pos = s.pos.to(device).contiguous()
    return device


class SimilarityResult:
    """Device tensors of one fixed-pose call over P pairs: ``score (P,)`` float64 (NaN where ``zero_denominator``),
    ``integrals (P, 3)`` = S_aa, S_bb, S_ab, ``zero_denominator (P,)`` bool; ``pairs`` (host) and ``forms``, the launch form
    of every pair, ``"wave"`` or ``"block"``."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _score(mode, metric, a, b, pairs, terms, details, device):
    if metric not in METRICS:
        raise ValueError("Unknown metric.")
    pairs = _pairs(pairs, len(a.n), len(b.n))
    forms = _check(mode, a, b, pairs, terms)
    device = _device(device, a, b)
    cA, cB = terms if terms is not None else (None, None)
    P = len(pairs)
    out = torch.empty((P, 4), dtype=torch.float64, device=device)
    flags = torch.empty((P,), dtype=torch.int32, device=device)
    lib = _lib.load()
    with torch.cuda.device(device):
        _lib.check(lib.shapemol_sim_score(_contexts.of(device), mode, METRICS[metric], len(a.n), ptr(a.off), ptr(a.pos), ptr(a.u), ptr(a.v),
                                          len(b.n), ptr(b.off), ptr(b.pos), ptr(b.u), ptr(b.v), P, ptr(pairs), 0 if cA is None else len(cA),
                                          ptr(cA), ptr(cB), ptr(out), ptr(flags), stream_ptr(device)), "shapemol_sim_score")
    if not details:
        return out[:, 3]
    return SimilarityResult(score=out[:, 3], integrals=out[:, :3], zero_denominator=flags != 0, pairs=pairs, forms=[FORMS[k] for k in forms])


def shape_tanimoto(centers_1, centers_2, alphas_1, alphas_2, prefactors_1, prefactors_2, *, pairs=None, details=False, device=None):
    """``shaep_utils.shape_tanimoto`` of the reference, batched: the Tanimoto score of the second-order Gaussian shape overlap
    with per-atom widths ``alphas`` and prefactors ``prefactors`` (a scalar serves every atom).  Returns the scores ``(P,)``
    float64 on the device, or with ``details`` a :class:`SimilarityResult`."""
    a, b = _Set("1", centers_1, alphas_1, prefactors_1), _Set("2", centers_2, alphas_2, prefactors_2)
    return _score(0, "tanimoto", a, b, pairs, None, details, device)


def get_rocs(centers_1, centers_2, prefactor=0.8, alpha=0.81, *, pairs=None, details=False, device=None):
    """``shaep_utils.get_ROCS`` of the reference, batched: :func:`shape_tanimoto` with one width and one prefactor.  The
    coefficients are formed in float64; the reference forms them in float32, which moves its score by a few 1e-8."""
    return shape_tanimoto(centers_1, centers_2, alpha, alpha, prefactor, prefactor, pairs=pairs, details=details, device=device)


def _terms(coefficients):
    a, b = coefficients
    a, b = host(a, np.float64).reshape(-1), host(b, np.float64).reshape(-1)
    if a.size != b.size:
        raise ValueError(f"molecule similarity: {a.size} amplitudes and {b.size} exponents")
    return np.ascontiguousarray(a), np.ascontiguousarray(-b)          # GaussInt: a * exp(b * r2), b < 0; the library: A * exp(-(B * r2))


def esp_similarity(centers_1, centers_2, charges_1, charges_2, coefficients, metric="carbo", *, pairs=None, details=False, device=None):
    """espsim's ``GetIntegralsViaGaussians`` + ``SimilarityMetric``, batched: the overlap of the molecules' electrostatic
    potentials from per-atom ``charges``, each atom pair contributing ``sum_k a_k * exp(b_k * r^2)``.  ``coefficients = (a, b)``
    are ``GaussInt``'s two tables in its own convention (``b`` negative), flattened; at most 16 terms.  ``metric``: ``"carbo"``
    or ``"tanimoto"``.  Where the reference raises on a zero denominator the score is NaN and ``zero_denominator`` is set."""
    a, b = _Set("1", centers_1, charges_1, None), _Set("2", centers_2, charges_2, None)
    if a.u is None or b.u is None:
        raise ValueError("molecule similarity: the electrostatic similarity needs per-atom charges")
    return _score(1, metric, a, b, pairs, _terms(coefficients), details, device)


class OverlayResult:
    """One overlay call over P pairs, device tensors: ``tanimoto (P,)`` float64, ``integrals (P, 3)`` = S_aa, S_bb, S_ab of the
    returned pose, ``start (P,)`` int32 the winning start (0..3 principal-frame starts, 4 the pose as given), ``rotation
    (P, 3, 3)`` and ``translation (P, 3)`` float64 acting on the first molecule's coordinates as given (``x @ R.T + t``),
    ``iterations (P,)`` int32, ``converged (P,)`` bool, ``zero_denominator (P,)`` bool; ``aligned``: a list with the moved
    coordinates of every pair's first molecule (views of one device tensor), or ``None``; ``pairs`` and ``forms`` (host)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def align_shapes(centers_1, centers_2, prefactor=0.8, alpha=0.81, *, alphas_1=None, alphas_2=None, prefactors_1=None, prefactors_2=None, pairs=None,
                 include_given=False, max_iter=200, gtol=1e-6, return_positions=True, device=None):
    """Overlay the molecules of ``centers_1`` on those of ``centers_2``: per pair, the rigid motion of the first molecule that
    maximises the Gaussian shape overlap :func:`get_rocs` scores (per-atom ``alphas_*`` / ``prefactors_*`` override the
    scalars).  This package's own rule, not ShaEP's: starts from the four proper rotations that map the first molecule's
    principal frame onto the second's (and, with ``include_given``, from the pose as given), BFGS with the analytic gradient
    until the largest gradient component is at most ``gtol * (S_aa + S_bb) / 2`` or ``max_iter`` iterations.  Returns an
    :class:`OverlayResult`."""
    if not 0 <= int(max_iter) <= sizes().max_iter or not (np.isfinite(gtol) and gtol >= 0):
        raise ValueError(f"molecule similarity: an iteration cap in 0..{sizes().max_iter} and a finite stopping threshold >= 0, got {max_iter} and {gtol}")
    pick = lambda per_atom, scalar: scalar if per_atom is None else per_atom  # noqa: E731
    a = _Set("1", centers_1, pick(alphas_1, alpha), pick(prefactors_1, prefactor))
    b = _Set("2", centers_2, pick(alphas_2, alpha), pick(prefactors_2, prefactor))
    pairs = _pairs(pairs, len(a.n), len(b.n))
    forms = _check(0, a, b, pairs, None)
    device = _device(device, a, b)
    P = len(pairs)
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=device)  # noqa: E731
    out, rot, trans, info = new((P, 4), torch.float64), new((P, 3, 3), torch.float64), new((P, 3), torch.float64), new((P, 4), torch.int32)
    counts = a.n[pairs[:, 0]]
    aligned = new((int(counts.sum()), 3), torch.float64) if return_positions else None
    lib = _lib.load()
    with torch.cuda.device(device):
        _lib.check(lib.shapemol_sim_align(_contexts.of(device), len(a.n), ptr(a.off), ptr(a.pos), ptr(a.u), ptr(a.v), len(b.n), ptr(b.off), ptr(b.pos),
                                          ptr(b.u), ptr(b.v), P, ptr(pairs), int(bool(include_given)), int(max_iter), float(gtol), ptr(out), ptr(rot),
                                          ptr(trans), ptr(info), ptr(aligned), stream_ptr(device)), "shapemol_sim_align")
    return OverlayResult(tanimoto=out[:, 3], integrals=out[:, :3], start=info[:, 0], rotation=rot, translation=trans, iterations=info[:, 1],
                         converged=info[:, 2] != 0, zero_denominator=info[:, 3] != 0, pairs=pairs, forms=[FORMS[k] for k in forms],
                         aligned=list(torch.split(aligned, counts.tolist())) if return_positions else None)


def _sample_positions(result):
    """The sampling driver's result, a tuple or a list as ``evaluate_samples`` takes it (``pred_pos`` first: a list with one
    ``(n, 3)`` array per molecule), or a list of position arrays.  The two are told apart by the first entry: a list whose own
    entries are two-dimensional (or an empty list) is ``pred_pos``; a sample written as a nested list has rows of numbers."""
    if isinstance(result, (list, tuple)) and len(result) >= 2 and isinstance(result[0], (list, tuple)) and (
            not len(result[0]) or result[0][0] is None or (result[0][0].dim() if isinstance(result[0][0], torch.Tensor) else np.ndim(result[0][0])) == 2):
        result = result[0]
    if not isinstance(result, (list, tuple)):
        raise ValueError("similarity to the condition: one position array per sample")
    return [None if p is None else host(p, np.float64) for p in result]


def _scorable(p, max_atoms):
    return p is not None and p.ndim == 2 and p.shape[1:] == (3,) and 1 <= len(p) <= max_atoms and bool(np.isfinite(p).all())


def similarity_to_condition(result_or_positions, condition_positions, prefactor=0.8, alpha=0.81, *, include_given=False, max_iter=200, gtol=1e-6,
                            device=None):
    """What ``calculate_shaep_shape_sim`` returns and ``evaluate_diffusion_sim.py`` summarises, without leaving the process:
    every sample overlaid on its condition molecule by :func:`align_shapes` and scored by :func:`get_rocs`.

    One group: ``result_or_positions`` is ``sample_diffusion_ligand``'s result as ``evaluate_samples`` takes it (a tuple or a
    list, ``pred_pos`` first) or a list of ``(n, 3)`` arrays, ``condition_positions`` one ``(m, 3)`` array.  Several groups: a list of such results and a list of conditions of
    the same length.  A sample that cannot be scored (no atoms, more than 256, a coordinate that is not finite, a NaN score)
    gets the score -1 and no positions, as the reference's ``except`` branch gives.  Returns a dict: ``aligned_positions``
    and ``scores`` (per group when there are several), and the three figures of the script over the scores ``>= 0``:
    ``avg_ref_shaep_rocssims`` and ``std_ref_shaep_rocssims`` (mean and deviation of the groups' means) and
    ``avg_ref_max_shaep_rocssims`` (mean of the groups' maxima); NaN for a group without a scored sample."""
    many = isinstance(condition_positions, (list, tuple))
    groups = list(result_or_positions) if many else [result_or_positions]
    conds = [host(c, np.float64) for c in (condition_positions if many else [condition_positions])]
    if len(groups) != len(conds) or not conds:
        raise ValueError(f"similarity to the condition: {len(groups)} groups of samples and {len(conds)} conditions")
    max_atoms = sizes().max_atoms
    for k, c in enumerate(conds):
        if not _scorable(c, max_atoms):
            raise ValueError(f"similarity to the condition: condition {k} must be (m, 3), finite, with 1..{max_atoms} atoms")
    samples = [_sample_positions(g) for g in groups]
    index = [(g, s) for g, grp in enumerate(samples) for s, p in enumerate(grp) if _scorable(p, max_atoms)]
    scores = [[-1.0] * len(grp) for grp in samples]
    aligned = [[None] * len(grp) for grp in samples]
    if index:
        r = align_shapes([samples[g][s] for g, s in index], conds, prefactor, alpha, pairs=np.array([[k, g] for k, (g, _) in enumerate(index)]),
                         include_given=include_given, max_iter=max_iter, gtol=gtol, device=device)
        value = r.tanimoto.cpu().numpy()
        moved = torch.cat(r.aligned).cpu().numpy()
        off = np.concatenate([[0], np.cumsum([len(samples[g][s]) for g, s in index])])
        for k, (g, s) in enumerate(index):
            if np.isfinite(value[k]):
                scores[g][s], aligned[g][s] = float(value[k]), moved[off[k]:off[k + 1]]
    with np.errstate(invalid="ignore"):
        kept = [np.array([x for x in grp if x >= 0], np.float64) for grp in scores]
        means = [k.mean() if len(k) else np.nan for k in kept]
        maxima = [k.max() if len(k) else np.nan for k in kept]
    return dict(aligned_positions=aligned if many else aligned[0], scores=scores if many else scores[0],
                avg_ref_shaep_rocssims=float(np.mean(means)), std_ref_shaep_rocssims=float(np.std(means)),
                avg_ref_max_shaep_rocssims=float(np.mean(maxima)))
