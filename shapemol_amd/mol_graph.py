"""Bond graphs of sampled molecules on the device: bonds with orders, fragments, completeness, rings, bond lengths.

What the reference's evaluation script (scripts/evaluate_diffusion_sim.py) does once it knows which atoms are bonded:
``fraction_complete``, the bond-length profile and its Jensen-Shannon distances, the pair profile and atom types of the
complete molecules, the ring sizes.  The reference decides bonds with OpenBabel; **the bond rule here is this package's own**:
a pair is a bond when ``analyze.get_bond_order`` -- the distance tables the caller supplies in :class:`StabilityRule`, the rule
``evaluate_geometry`` counts valences with -- gives an order above 0.  It is not OpenBabel's perception, and agreement with the
reference's reconstructed molecules has not been measured and is not claimed.  ``ring_sizes`` is no SSSR: bit ``s`` says that
some bond's shortest cycle has ``s`` bonds.

One kernel body in two passes (csrc/sm_mol_graph.h) does it for every frame of a packed batch; the
results stay on the device.  Every output is an integer, the same in every run, and equals the numpy oracle exactly.

Limits (``ValueError`` before any kernel runs): 1..256 atoms per molecule and no empty molecule, at most 16 elements in the
rule, 32 atom classes and 255 bin edges per histogram; fewer than 2^31 bonds in a call.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._native import DeviceContexts, host, ptr, stream_ptr
from .evaluation import FORMS  # noqa: F401  (the launch forms' names, a name of this module as well)
from .evaluation import _as_stack, _bins, _finish, _pack_samples, _prepare, _Report, class_table

Sizes = collections.namedtuple("Sizes", "wave_atoms max_atoms max_elements max_classes max_edges threads ring_bits")
MOL_FIELDS = ("n_bonds", "n_frags", "largest_frag", "complete", "n_cycles", "ring_sizes")
# element symbols by atomic number, for the mol block
_SYMBOLS = ("* H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo Tc "
            "Ru Rh Pd Ag Cd In Sn Sb Te I Xe").split()


def sizes():
    """The library's limits and block shape (shapemol_graph_sizes; the constants of csrc/sm_mol_rule.h and sm_mol_graph.h)."""
    out = (C.c_int64 * 7)()
    _lib.load().shapemol_graph_sizes(out, 7)
    return Sizes(*out)


_contexts = DeviceContexts("shapemol_graph_create", "shapemol_graph_destroy")


def _debug_fill(device, byte):
    """Tests only: fill the context's device workspaces."""
    _lib.check(_lib.load().shapemol_graph_debug_fill(_contexts.of(device), int(byte), stream_ptr(device)), "shapemol_graph_debug_fill")


def _jsd(p, q):
    from scipy.spatial import distance
    return distance.jensenshannon(p, q)


def bond_key(bond_type):
    """``(z_a, z_b, order)`` -> the reference's name of a bond type, ``'6-8|2'``."""
    a, b, o = bond_type
    return f"{int(a)}-{int(b)}|{int(o)}"


class GraphReport(_Report):
    """Device tensors of one call over F frames, N atoms and B molecules per frame.  Per atom ``(F, N)`` int32: ``nr_bonds``
    (the orders summed: ``evaluate_geometry``'s ``nr_bonds``), ``degree``, ``frag`` (the smallest atom index, within the frame,
    of the atom's fragment), ``ring`` (the smallest ring through one of its bonds, 0: none).  Per molecule ``(F, B)``:
    ``n_bonds``, ``n_frags``, ``largest_frag``, ``n_cycles``, ``ring_sizes`` int32 and ``complete`` bool.  The bond list:
    ``bond_list (total, 3)`` int32 = atom i, atom j > i (indices within the frame), order, sorted by frame, molecule, i, j;
    ``bond_ring (total,)`` the bonds in the shortest cycle through each, 0 for a bridge; ``bond_offsets (F * B + 1,)`` int64.
    Per frame, int64: ``hist_bl (F, 2, P, 3, n_bl + 1)`` bond lengths of all | complete molecules for the ``P`` element pairs
    ``pairs`` (atomic numbers, in the rule's order) and orders 1..3; ``hist_cc``, ``hist_all``, ``class_counts`` of the
    complete molecules; ``n_complete (F,)``; ``ring_counts (F, 32)`` molecules whose ``ring_sizes`` has each bit.  Host:
    ``n_atoms (B,)``, ``mol_off (B + 1,)``, the bin edges ``bl_bins``, ``cc_bins``, ``all_bins``.  ``bond_graph`` drops the
    frame axis of the per-atom, per-molecule and per-frame tensors."""

    def _span(self, mol, frame):
        f = 0 if frame is None else int(frame)
        B = len(self.n_atoms)
        if not 0 <= mol < B or not 0 <= f < self.n_frames:
            raise IndexError(f"bond graph: molecule {mol} of frame {f}; there are {B} molecules and {self.n_frames} frames")
        lo, hi = (int(x) for x in self.bond_offsets[f * B + mol:f * B + mol + 2])
        return lo, hi

    def bonds(self, mol, frame=None, local=False):
        """The bonds of one molecule (of frame 0 unless given) as a ``(k, 3)`` device tensor of (i, j, order); with ``local``
        the atom indices count from the molecule's first atom."""
        lo, hi = self._span(mol, frame)
        b = self.bond_list[lo:hi]
        if local:
            b = b.clone()
            b[:, :2] -= int(self.mol_off[mol])
        return b

    def rings(self, mol, frame=None):
        """The ring of every bond of ``bonds(mol, frame)``."""
        lo, hi = self._span(mol, frame)
        return self.bond_ring[lo:hi]

    def fragments(self, mol=None, frame=None):
        """The fragment labels: of every atom (all frames, or ``frame``), or of the atoms of molecule ``mol``."""
        t = self.frag if self.single or frame is None else self.frag[frame]
        return t if mol is None else t[..., int(self.mol_off[mol]):int(self.mol_off[mol + 1])]

    def validity(self, frame=None, geometry=None):
        """``complete``: complete molecules over molecules (the script's ``fraction_complete`` under this package's bond rule) --
        over all frames, or over ``frame``; with ``geometry`` (the :class:`GeometryReport` of the same call) its two fractions
        beside it."""
        c = self._frames(self.complete, frame)
        out = {} if geometry is None else dict(geometry.validity(frame))
        out["complete"] = int(c.sum()) / c.numel()
        return out

    def pair_length_profile(self, frame=None):
        """The pair-distance profile of the complete molecules (the script's ``success_pair_dist``); all zeros when none is."""
        out = {}
        for key, h in (("CC_2A", self.hist_cc), ("All_12A", self.hist_all)):
            counts = self._frames(h, frame).sum(0).cpu().numpy().astype(np.float64)
            out[key] = counts / counts.sum() if counts.sum() else counts
        return out

    def bond_length_profile(self, complete_only=True, frame=None):
        """``get_bond_length_profile``: ``{(z_a, z_b, order): distribution over the n_bl + 1 bins}`` for every element pair of
        the rule and order 1..3, summed over the frames; a type without bonds gives zeros, not a division by zero."""
        h = self._frames(self.hist_bl, frame)[:, 1 if complete_only else 0].sum(0).cpu().numpy().astype(np.float64)
        out = {}
        for p, (za, zb) in enumerate(self.pairs):
            for o in (1, 2, 3):
                counts = h[p, o - 1]
                out[(za, zb, o)] = counts / counts.sum() if counts.sum() else counts
        return out

    def jsd(self, empirical, complete_only=True, frame=None):
        """Jensen-Shannon distances (``scipy.spatial.distance.jensenshannon``, float64, on the host, as ``GeometryReport.jsd``)
        against the caller's distributions: keys ``(z_a, z_b, order)`` name bond types (``eval_bond_length_profile``; the
        result's key is the reference's ``'JSD_6-8|2'``), keys ``'CC_2A'`` / ``'All_12A'`` the pair profiles of the complete
        molecules.  ``None`` where this report has nothing to compare: no such type, or no bond or pair of it."""
        bl, pl = self.bond_length_profile(complete_only, frame), self.pair_length_profile(frame)
        out = {}
        for k, gt in empirical.items():
            if isinstance(k, str):
                name, prof = f"JSD_{k}", pl.get(k)
            else:
                k = tuple(int(x) for x in k)
                name, prof = f"JSD_{bond_key(k)}", bl.get(k if k[0] <= k[1] or k in bl else (k[1], k[0], k[2]))
            out[name] = _jsd(np.asarray(gt, np.float64), prof) if prof is not None and prof.sum() else None
        return out

    def ring_ratio(self, frame=None):
        """``{s: molecules with a ring of s bonds / molecules}`` for s = 3..30 and ``'>30'``: the script's ring-size ratios
        under this package's definition (some bond's shortest cycle has s bonds; not an SSSR)."""
        c = self._frames(self.ring_counts, frame).sum(0).cpu().numpy()
        mols = self._frames(self.complete, frame).numel()
        out = {s: int(c[s]) / mols for s in range(3, 31)}
        out[">30"] = int(c[31]) / mols
        return out


def _run(pos, classes, batch, rule, slots, single, cc_bins, all_bins, bond_bins, details, device):
    """``pos (F, N, 3)``, ``classes (F, N)`` indices into ``slots`` (class -> rule row), ``batch (N,)`` sorted molecule ids."""
    bl_edges, _ = _bins(np.linspace(0.8, 2.4, 161) if bond_bins is None else bond_bins, 0)
    # a class outside the table is left to the device: the run's status flag, reported as a ValueError below
    c = _prepare("bond graph", "shapemol_graph_check", (bl_edges,), False, "bond graphs are built on a HIP device", pos, classes, batch, rule, slots,
                 cc_bins, all_bins, device)
    F, N, B, E, new, lib = c.F, c.N, c.B, len(rule.elements), c.new, _lib.load()
    out = dict(nr_bonds=new((F, N), torch.int32), degree=new((F, N), torch.int32), frag=new((F, N), torch.int32), ring=new((F, N), torch.int32),
               mol=new((F, B, 6), torch.int32), hist_bl=new((F, 2, E * (E + 1) // 2, 3, len(bl_edges) + 1), torch.int64),
               hist_cc=new((F, len(c.cc_edges) + 1), torch.int64), hist_all=new((F, len(c.all_edges) + 1), torch.int64),
               class_counts=new((F, len(c.slots)), torch.int64), frame_counts=new((F, 33), torch.int64))
    total = C.c_int64(0)
    with torch.cuda.device(c.device):
        ctx, s = _contexts.of(c.device), stream_ptr(c.device)
        if lib.shapemol_graph_run(ctx, *c.batch_args, *c.rule_args, ptr(bl_edges), len(bl_edges), *(ptr(t) for t in out.values()), C.byref(total), s):
            msg = lib.shapemol_last_error().decode()
            if msg.startswith("bond graph:"):
                raise ValueError(msg)
            raise _lib.ShapeMolLibraryError(f"shapemol_graph_run failed: {msg}")
        n = int(total.value)
        offsets, bond_list, bond_ring = np.zeros(F * B + 1, np.int64), new((n, 3), torch.int32), new((n,), torch.int32)
        _lib.check(lib.shapemol_graph_bonds(ctx, 0, ptr(offsets), F * B + 1, s), "shapemol_graph_bonds")
        if n:
            _lib.check(lib.shapemol_graph_bonds(ctx, 1, ptr(bond_list), 3 * n, s), "shapemol_graph_bonds")
            _lib.check(lib.shapemol_graph_bonds(ctx, 2, ptr(bond_ring), n, s), "shapemol_graph_bonds")
    mol, fc = out.pop("mol"), out.pop("frame_counts")
    for k, name in enumerate(MOL_FIELDS):
        out[name] = mol[..., k].contiguous() if name != "complete" else mol[..., k] != 0
    out["n_complete"], out["ring_counts"] = fc[:, 0].contiguous(), fc[:, 1:].contiguous()
    z = [int(e) for e in rule.elements]
    return _finish(GraphReport, c, single, details, out, n_frames=F, mol_off=c.off, bond_offsets=offsets, bond_list=bond_list, bond_ring=bond_ring,
                   pairs=[(z[a], z[b]) for a in range(E) for b in range(a, E)], bl_bins=bl_edges)


def bond_graph_trajectory(pos_traj, v_traj, batch, rule, mode="add_aromatic", hs=False, cc_bins=None, all_bins=None, bond_bins=None, details=False, *,
                          num_classes=None, device=None):
    """The bond graphs of every frame of a chain; the arguments of ``evaluate_trajectory`` (``hs`` is accepted for the shared
    convention and changes nothing: bonds do not depend on valences), plus ``bond_bins``: the bond-length bin edges in
    Angstrom, default ``np.linspace(0.8, 2.4, 161)``.  ``hist_bl`` takes ``F * 2 * E (E + 1) / 2 * 3 * (len(bond_bins) + 1)``
    int64 of device memory; pass coarser edges for long trajectories.  Returns a :class:`GraphReport`."""
    slots = class_table(rule, mode, num_classes)
    return _run(_as_stack(pos_traj), _as_stack(v_traj), batch, rule, slots, False, cc_bins, all_bins, bond_bins, details, device)


def bond_graph(pos, v, batch, rule, mode="add_aromatic", hs=False, cc_bins=None, all_bins=None, bond_bins=None, details=False, *, num_classes=None,
               device=None):
    """One frame: ``pos (N, 3)`` or ``(1, N, 3)``, ``v (N,)`` or ``(1, N)``, ``batch (N,)``; see :func:`bond_graph_trajectory`.
    The report's per-atom, per-molecule and per-frame tensors have no frame axis."""
    slots = class_table(rule, mode, num_classes)
    pos, v = (x if isinstance(x, torch.Tensor) else torch.as_tensor(host(x)) for x in (pos, v))
    if pos.dim() == 3 and pos.shape[0] == 1 and v.dim() == 2 and v.shape[0] == 1:
        pos, v = pos[0], v[0]
    if pos.dim() != 2 or v.dim() != 1:
        raise ValueError(f"bond graph: positions (N, 3) and classes (N,), got {tuple(pos.shape)} and {tuple(v.shape)}")
    return _run(pos[None], v[None], batch, rule, slots, True, cc_bins, all_bins, bond_bins, details, device)


def bond_graph_samples(result, rule, mode="add_aromatic", hs=False, cc_bins=None, all_bins=None, bond_bins=None, details=False, *, num_classes=None,
                       device=None):
    """The final molecules of ``sample_diffusion_ligand``, as ``evaluate_samples`` takes them: ``result`` is its tuple
    (``pred_pos``, ``pred_v`` first) or just that pair.  One frame; see :func:`bond_graph`."""
    pos, v, batch = _pack_samples("bond graph", result)
    return bond_graph(pos, v, batch, rule, mode, hs, cc_bins, all_bins, bond_bins, details, num_classes=num_classes, device=device)


def atom_type_jsd(counts, empirical, atomic_numbers=None):
    """``eval_atom_type.eval_atom_type_distribution``: the Jensen-Shannon distance between ``empirical`` (``{atomic number:
    probability}``, the caller's table) and the predicted distribution over the same keys, each count over ALL counted atoms.
    ``counts``: ``{atomic number: count}``, or class counts (an array or tensor, summed over leading axes) with
    ``atomic_numbers`` naming every class's element (classes of one element are added)."""
    if isinstance(counts, dict):
        by_z = {int(k): int(v) for k, v in counts.items()}
    else:
        c = host(counts).astype(np.int64)
        c = c.reshape(-1, c.shape[-1]).sum(0)
        if atomic_numbers is None or len(atomic_numbers) != len(c):
            raise ValueError("atom_type_jsd: class counts need the atomic number of every class")
        by_z = collections.Counter()
        for z, k in zip(atomic_numbers, c.tolist()):
            by_z[int(z)] += k
    total = sum(by_z.values())
    if total <= 0:
        return None
    pred = np.array([by_z.get(int(k), 0) / total for k in empirical], np.float64)
    return _jsd(np.array(list(empirical.values()), np.float64), pred)


def to_molblock(pos, atomic_numbers, bonds, name="shapemol_amd"):
    """A V2000 mol block of one molecule: ``pos (n, 3)``, ``atomic_numbers (n,)``, ``bonds (k, 3)`` rows of (i, j, order) with
    atom indices counted from the molecule's first atom (``GraphReport.bonds(mol, local=True)``).  Pure Python; a reader such
    as RDKit's ``MolFromMolBlock`` takes it from there."""
    pos, z = host(pos, np.float64).reshape(-1, 3), [int(a) for a in host(atomic_numbers).reshape(-1)]
    bonds = host(bonds).astype(np.int64).reshape(-1, 3)
    n = len(z)
    if len(pos) != n or n < 1:
        raise ValueError(f"to_molblock: {len(pos)} positions and {n} atomic numbers")
    if n > 999 or len(bonds) > 999:
        raise ValueError("to_molblock: a V2000 block holds at most 999 atoms and 999 bonds")
    if any(not 0 < a < len(_SYMBOLS) for a in z):
        raise ValueError("to_molblock: atomic numbers 1..54")
    lines = [name, "     shapemol_amd          3D", "", f"{n:3d}{len(bonds):3d}  0  0  0  0  0  0  0  0999 V2000"]
    for (x, y, w), a in zip(pos.tolist(), z):
        lines.append(f"{x:10.4f}{y:10.4f}{w:10.4f} {_SYMBOLS[a]:<3s} 0  0  0  0  0  0  0  0  0  0  0  0")
    for i, j, o in bonds.tolist():
        if not (0 <= i < n and 0 <= j < n and i != j and 1 <= o <= 3):
            raise ValueError(f"to_molblock: bond ({i}, {j}, {o}) does not fit a molecule of {n} atoms")
        lines.append(f"{i + 1:3d}{j + 1:3d}{o:3d}  0")
    lines.append("M  END")
    return "\n".join(lines) + "\n"
