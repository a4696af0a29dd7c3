"""Geometry scores of sampled molecules on the device: stability and pair-distance profiles.

What the reference's evaluation script does first with its samples (scripts/evaluate_diffusion_sim.py:134-148, :228-229):
``analyze.check_stability`` per molecule, ``eval_bond_length.pair_distance_from_pos_v`` + ``get_pair_length_profile`` +
``eval_pair_length_profile`` over all of them, and the atom-type counts.  Here one kernel (csrc/sm_mol_eval.h, DESIGN.md
section 22) does it for every frame of a packed batch -- a final frame, or all recorded frames of a chain -- and the results
stay on the device.  Every output is an integer and equals the reference's loops on the same float64 positions exactly.

The rule is data: ``StabilityRule`` holds the bond-length tables, margins and valences, read from a JSON file
(INTEGRATION.md shows how to dump the reference's); the package ships no table.  Bin edges and cut-offs are arguments.

Limits (``ValueError`` before any kernel runs): 1..1024 atoms per molecule and no empty molecule, classes inside the
vocabulary, at most 16 elements in the rule, 32 atom classes and 255 bin edges per histogram.
"""
import collections
import ctypes as C
import json

import numpy as np
import torch

from . import _lib
from ._native import DeviceContexts, hip_device, host, ptr, stream_ptr
from .mol_surface import VOCAB_ELEMENTS

FORMS = ("wave", "block")
Sizes = collections.namedtuple("Sizes", "wave_atoms max_atoms max_elements max_classes max_edges threads")
_RULE_FIELDS = ("elements", "bonds1", "bonds2", "bonds3", "margins", "allowed_bonds")


def sizes():
    """The library's limits and block shape (shapemol_eval_sizes; the constants of csrc/sm_mol_rule.h and sm_mol_eval.h)."""
    out = (C.c_int64 * 6)()
    _lib.load().shapemol_eval_sizes(out, 6)
    return Sizes(*out)


class StabilityRule:
    """The tables of the reference's ``analyze`` module as float64 arrays: ``elements`` (E,) atomic numbers, ``bonds1``,
    ``bonds2``, ``bonds3`` (E, E) bond lengths in pm (``-1``: no such bond; it stays a number, so the threshold is
    ``-1 + margin``, as in the reference), ``margins`` (3,), ``allowed_bonds`` (E,) one valence per element."""

    def __init__(self, elements, bonds1, bonds2, bonds3, margins, allowed_bonds):
        self.elements = np.array(elements, np.float64).reshape(-1)
        E = len(self.elements)
        if E < 1 or len(set(self.elements.tolist())) != E:
            raise ValueError("stability rule: elements must be distinct atomic numbers, at least one")
        self.bonds1, self.bonds2, self.bonds3 = (np.array(b, np.float64) for b in (bonds1, bonds2, bonds3))
        for name in ("bonds1", "bonds2", "bonds3"):
            if getattr(self, name).shape != (E, E):
                raise ValueError(f"stability rule: {name} must be a {E} x {E} table")
        self.margins = np.array(margins, np.float64).reshape(-1)
        self.allowed_bonds = np.array(allowed_bonds, np.float64).reshape(-1)
        if self.margins.shape != (3,) or self.allowed_bonds.shape != (E,):
            raise ValueError("stability rule: three margins and one valence per element")

    def thresholds(self):
        """(3, E, E) float64: ``bondsK + marginK``, what ``100 * d`` is compared with."""
        return np.ascontiguousarray(np.stack([self.bonds1 + self.margins[0], self.bonds2 + self.margins[1], self.bonds3 + self.margins[2]]))

    def slot_of(self, atomic_numbers):
        """The rule's row of every atomic number; ``ValueError`` names the ones it lacks."""
        z = np.asarray(atomic_numbers).reshape(-1)
        rows = {float(e): k for k, e in enumerate(self.elements)}
        missing = sorted({int(a) for a in z.tolist() if float(a) not in rows})
        if missing:
            raise ValueError(f"stability rule: no entry for atomic number(s) {missing}")
        return np.array([rows[float(a)] for a in z.tolist()], np.int32)

    def to_dict(self):
        return {k: getattr(self, k).tolist() for k in _RULE_FIELDS}

    def to_json(self, path):
        with open(path, "w") as f:
            json.dump(self.to_dict(), f)

    @classmethod
    def from_json(cls, path):
        with open(path) as f:
            d = json.load(f)
        return cls(*(d[k] for k in _RULE_FIELDS))


def class_table(rule, mode="add_aromatic", num_classes=None):
    """The rule's row of every atom class of the vocabulary ``mode``.  ``num_classes`` (default: the vocabulary's size) may
    exceed the ``add_aromatic`` table: the classes past it are carbon, as in ``transforms.get_atomic_number_from_index``."""
    if mode not in VOCAB_ELEMENTS:
        raise ValueError(f"unknown atom vocabulary {mode!r}")
    z = list(VOCAB_ELEMENTS[mode])
    n = len(z) if num_classes is None else int(num_classes)
    if n < len(z) or (n > len(z) and mode != "add_aromatic"):
        raise ValueError(f"{mode!r} has {len(z)} atom classes, not {n}")
    return rule.slot_of(z + [6] * (n - len(z)))


def _bins(bins, default_stop):
    """``None`` | edges | (edges, cut-off) -> (float64 edges, cut-off); the cut-off defaults to the last edge."""
    if bins is None:
        bins = np.linspace(0, default_stop, 100)
    cut = None
    if isinstance(bins, tuple) and len(bins) == 2 and np.ndim(bins[0]) == 1:
        bins, cut = bins
    edges = np.ascontiguousarray(np.asarray(bins, np.float64).reshape(-1))
    if edges.size < 1:
        raise ValueError("molecule evaluation: a histogram needs at least one bin edge")
    return edges, float(edges[-1] if cut is None else cut)


_contexts = DeviceContexts("shapemol_eval_create", "shapemol_eval_destroy")


def _debug_fill(device, byte):
    """Tests only: fill the context's device workspace."""
    _lib.check(_lib.load().shapemol_eval_debug_fill(_contexts.of(device), int(byte), stream_ptr(device)), "shapemol_eval_debug_fill")


class _Report:
    """The fields of one call; ``single``: the call had one frame and its tensors have no frame axis."""

    def __init__(self, single, **kw):
        self.single = single
        self.__dict__.update(kw)

    def _frames(self, t, frame):
        t = t[None] if self.single else t
        return t if frame is None else t[frame][None] if isinstance(frame, int) else t[frame]


class GeometryReport(_Report):
    """Device tensors of one call over F frames, N atoms and B molecules per frame: ``nr_bonds (F, N)`` int32,
    ``n_stable_atoms (F, B)`` int32, ``mol_stable (F, B)`` bool, ``hist_cc (F, n_cc + 1)``, ``hist_all (F, n_all + 1)`` and
    ``class_counts (F, C)`` int64; ``n_atoms (B,)`` (host) the molecules' sizes; ``cc_bins`` / ``all_bins`` the edges used;
    ``forms`` (with ``details=True``) the launch form of every molecule, ``"wave"`` or ``"block"``.  ``evaluate_geometry``
    drops the frame axis."""

    def validity(self, frame=None):
        """``mol_stable`` and ``atm_stable`` as the script computes them: stable molecules over molecules, stable atoms over
        atoms -- over all frames, or over ``frame`` (an index or a slice)."""
        ms, ns = self._frames(self.mol_stable, frame), self._frames(self.n_stable_atoms, frame)
        return {"mol_stable": int(ms.sum()) / ms.numel(), "atm_stable": int(ns.sum()) / (ns.shape[0] * int(self.n_atoms.sum()))}

    def pair_length_profile(self, frame=None):
        """``get_pair_length_profile`` of the reference: the two histograms, summed over the frames, as distributions."""
        out = {}
        for key, h in (("CC_2A", self.hist_cc), ("All_12A", self.hist_all)):
            counts = self._frames(h, frame).sum(0).cpu().numpy()
            out[key] = np.array(counts) / np.sum(counts)
        return out

    def jsd(self, empirical, frame=None):
        """``eval_pair_length_profile`` against the caller's distributions ``{'CC_2A': ..., 'All_12A': ...}``: Jensen-Shannon
        distances by ``scipy.spatial.distance.jensenshannon`` in float64 on the host."""
        from scipy.spatial import distance
        profile = self.pair_length_profile(frame)
        return {f"JSD_{k}": distance.jensenshannon(gt, profile[k]) if k in profile else None for k, gt in empirical.items()}


def _as_stack(x):
    if isinstance(x, (list, tuple)):
        return torch.stack([torch.as_tensor(t) for t in x]) if any(isinstance(t, torch.Tensor) for t in x) else np.stack([np.asarray(t) for t in x])
    return x


_Call = collections.namedtuple("_Call", "pos classes thr device F N B counts off slots cc_edges all_edges forms batch_args rule_args new")


def _prepare(what, check, more_edges, class_range, device_msg, pos, classes, batch, rule, slots, cc_bins, all_bins, device):
    """The front half of a call of the geometry scores and of the bond graphs (mol_graph.py), refusals prefixed with ``what``:
    ``pos (F, N, 3)``, ``classes (F, N)`` indices into ``slots`` (class -> rule row) and ``batch (N,)`` sorted molecule ids
    are checked, the library's ``check`` function (given the histograms' edges, ``more_edges`` after the two common ones) plans
    the call and names the launch forms, and the inputs go to the device.  ``class_range``: refuse classes outside ``slots``
    here, with one reduction, and not after the run."""
    E, Cn = len(rule.elements), len(slots)
    cc_edges, cc_cut = _bins(cc_bins, 2)
    all_edges, all_cut = _bins(all_bins, 12)
    tensors = isinstance(pos, torch.Tensor) and isinstance(classes, torch.Tensor)
    if not tensors:
        pos, classes = torch.as_tensor(host(pos)), torch.as_tensor(host(classes))
    if pos.dim() != 3 or pos.shape[-1] != 3 or classes.shape != pos.shape[:2]:
        raise ValueError(f"{what}: positions (F, N, 3) and classes (F, N), got {tuple(pos.shape)} and {tuple(classes.shape)}")
    F, N = int(pos.shape[0]), int(pos.shape[1])
    b = host(batch).astype(np.int64).reshape(-1)
    if len(b) != N or N < 1:
        raise ValueError(f"{what}: {N} atoms per frame and a batch vector of {len(b)}")
    if b[0] != 0 or (np.diff(b) < 0).any():
        raise ValueError(f"{what}: the batch vector must be sorted and start at 0 (a packed batch)")
    B = int(b[-1]) + 1
    counts = np.bincount(b, minlength=B)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    slots = np.ascontiguousarray(slots, np.int32)
    forms = np.zeros(B, np.int32)
    lib = _lib.load()
    more = [x for e in more_edges for x in (ptr(e), len(e))]
    if getattr(lib, check)(F, B, ptr(off), E, Cn, ptr(slots), ptr(cc_edges), len(cc_edges), cc_cut, ptr(all_edges), len(all_edges), all_cut, *more,
                           ptr(forms)):
        raise ValueError(lib.shapemol_last_error().decode())
    if classes.dtype not in (torch.int32, torch.int64):
        if classes.is_floating_point() or classes.dtype == torch.bool:
            raise TypeError(f"{what}: atom classes must be integers, got {classes.dtype}")
        classes = classes.to(torch.int64)
    if class_range:
        lo, hi = (int(t) for t in torch.aminmax(classes))
        if lo < 0 or hi >= Cn:
            raise ValueError(f"{what}: atom classes {lo}..{hi} lie outside the {Cn} classes")
    if device is None:
        device = pos.device if pos.is_cuda else "cuda" if torch.cuda.is_available() else "cpu"
    device = hip_device(device, device_msg)
    pos = pos.to(device=device, dtype=torch.float32).contiguous()
    classes = classes.to(device).contiguous()
    carbon, thr = np.flatnonzero(rule.elements == 6.0), rule.thresholds()
    # what both run functions take first: the batch up to the thresholds, then the rule from the carbon slot to the histograms
    batch_args = (F, B, ptr(off), ptr(pos), ptr(classes), int(classes.dtype == torch.int64), E, ptr(thr))
    rule_args = (int(carbon[0]) if len(carbon) else -1, Cn, ptr(slots), ptr(cc_edges), len(cc_edges), cc_cut, ptr(all_edges), len(all_edges), all_cut)
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=device)  # noqa: E731
    return _Call(pos, classes, thr, device, F, N, B, counts, off, slots, cc_edges, all_edges, forms, batch_args, rule_args, new)


def _finish(report, c, single, details, out, **kw):
    """The report of a call: without the frame axis for a ``single`` frame, with the launch forms for ``details``."""
    if single:
        out = {k: t[0] for k, t in out.items()}
    if details:
        out["forms"] = [FORMS[k] for k in c.forms]
    return report(single, n_atoms=c.counts, cc_bins=c.cc_edges, all_bins=c.all_edges, **kw, **out)


def _run(pos, classes, batch, rule, slots, single, hs, cc_bins, all_bins, details, device):
    """``pos (F, N, 3)``, ``classes (F, N)`` indices into ``slots`` (class -> rule row), ``batch (N,)`` sorted molecule ids."""
    c = _prepare("molecule evaluation", "shapemol_eval_check", (), True, "molecules are evaluated on a HIP device", pos, classes, batch, rule, slots,
                 cc_bins, all_bins, device)
    F, N, B, new = c.F, c.N, c.B, c.new
    allowed = np.ascontiguousarray(rule.allowed_bonds)
    out = dict(nr_bonds=new((F, N), torch.int32), n_stable_atoms=new((F, B), torch.int32), mol_stable=new((F, B), torch.bool),
               hist_cc=new((F, len(c.cc_edges) + 1), torch.int64), hist_all=new((F, len(c.all_edges) + 1), torch.int64),
               class_counts=new((F, len(c.slots)), torch.int64))
    with torch.cuda.device(c.device):
        _lib.check(_lib.load().shapemol_eval_run(_contexts.of(c.device), *c.batch_args, ptr(allowed), *c.rule_args, int(bool(hs)),
                                                 *(ptr(t) for t in out.values()), stream_ptr(c.device)), "shapemol_eval_run")
    return _finish(GeometryReport, c, single, details, out)


def evaluate_trajectory(pos_traj, v_traj, batch, rule, mode="add_aromatic", hs=False, cc_bins=None, all_bins=None, details=False, *,
                        num_classes=None, device=None):
    """Scores of every frame of a chain: ``pos_traj (F, N, 3)`` and ``v_traj (F, N)`` (atom classes of the vocabulary ``mode``)
    as stacked tensors or as lists of per-step tensors, ``batch (N,)`` the packed batch's molecule ids, shared by all frames
    (``sample_diffusion``'s layout).  Tensors on a HIP device are read in place (positions float32, classes int32 or int64);
    anything else is uploaded to ``device``.  ``hs=True`` asks for valence == bonds, as the reference's flag.  ``cc_bins`` /
    ``all_bins``: bin edges, or ``(edges, cut-off)``; default ``np.linspace(0, 2, 100)`` / ``np.linspace(0, 12, 100)`` with the
    last edge as the cut-off.  Returns a :class:`GeometryReport`."""
    slots = class_table(rule, mode, num_classes)
    return _run(_as_stack(pos_traj), _as_stack(v_traj), batch, rule, slots, False, hs, cc_bins, all_bins, details, device)


def evaluate_geometry(pos, v, batch, rule, mode="add_aromatic", hs=False, cc_bins=None, all_bins=None, details=False, *, num_classes=None,
                      device=None):
    """One frame: ``pos (N, 3)``, ``v (N,)``, ``batch (N,)``; see :func:`evaluate_trajectory`.  The report's tensors have no
    frame axis."""
    slots = class_table(rule, mode, num_classes)
    pos, v = (x if isinstance(x, torch.Tensor) else torch.as_tensor(host(x)) for x in (pos, v))
    if pos.dim() != 2 or v.dim() != 1:
        raise ValueError(f"molecule evaluation: positions (N, 3) and classes (N,), got {tuple(pos.shape)} and {tuple(v.shape)}")
    return _run(pos[None], v[None], batch, rule, slots, True, hs, cc_bins, all_bins, details, device)


def _pack_samples(what, result):
    """Per-molecule lists ``(pred_pos, pred_v, ...)`` as one packed frame: float32 positions, int64 classes, the batch vector."""
    pred_pos, pred_v = result[0], result[1]
    if len(pred_pos) != len(pred_v) or not len(pred_pos):
        raise ValueError(f"{what}: one position array and one class array per molecule, at least one")
    ns = [len(host(v).reshape(-1)) for v in pred_v]
    if 0 in ns:
        raise ValueError(f"{what}: molecule {ns.index(0)} has no atoms")
    pos = np.concatenate([host(p, np.float64).reshape(-1, 3) for p in pred_pos]).astype(np.float32)
    v = np.concatenate([host(v).reshape(-1) for v in pred_v]).astype(np.int64)
    if len(pos) != len(v):
        raise ValueError(f"{what}: positions and classes of a molecule differ in length")
    return pos, v, np.repeat(np.arange(len(ns)), ns)


def evaluate_samples(result, rule, mode="add_aromatic", hs=False, cc_bins=None, all_bins=None, details=False, *, num_classes=None, device=None):
    """The final molecules of ``sample_diffusion_ligand``: ``result`` is its tuple (``pred_pos``, ``pred_v`` first: lists with
    one ``(n, 3)`` and one ``(n,)`` array per molecule) or just that pair.  The float64 host positions are the chain's float32
    ones, so the upload as float32 loses nothing.  One frame; see :func:`evaluate_geometry`."""
    pos, v, batch = _pack_samples("molecule evaluation", result)
    return evaluate_geometry(pos, v, batch, rule, mode, hs, cc_bins, all_bins, details, num_classes=num_classes, device=device)


def check_stability(positions, atom_type, rule, hs=False, return_nr_bonds=False, *, device=None):
    """``analyze.check_stability`` of the reference for one molecule: ``positions (n, 3)``, ``atom_type (n,)`` atomic numbers.
    Returns ``(molecule_stable, nr_stable_bonds, n)`` and, with ``return_nr_bonds``, the bonds per atom as a numpy array."""
    z = host(atom_type).reshape(-1)
    classes = rule.slot_of(z).astype(np.int64)
    pos = positions if isinstance(positions, torch.Tensor) else torch.as_tensor(host(positions))
    if pos.dim() != 2 or pos.shape[1] != 3 or len(classes) != pos.shape[0]:
        raise ValueError(f"check_stability: positions (n, 3) and n atom types, got {tuple(pos.shape)} and {len(classes)}")
    v = torch.as_tensor(classes).to(pos.device)
    r = _run(pos[None], v[None], np.zeros(len(classes), np.int64), rule, np.arange(len(rule.elements), dtype=np.int32), True, hs, None, None, False,
             device)
    res = (bool(r.mol_stable[0]), int(r.n_stable_atoms[0]), len(classes))
    return res + (r.nr_bonds.cpu().numpy().astype(np.int64),) if return_nr_bonds else res
