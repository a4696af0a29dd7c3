"""Float64 numpy oracle of the bond graphs: what shapemol_amd.mol_graph computes on the device, written
independently of it.  The pair loop is analyze.check_stability's with the pairs kept (tests/mol_eval_oracle.py: distances and
bond_orders, themselves held to the reference's stored results); the fragments come from a union-find, the rings from one
breadth-first search per bond on the graph without that bond, the bins from np.searchsorted(..., side='left')."""
import collections

import numpy as np

import mol_eval_oracle as E

WAVE_ATOMS, MAX_ATOMS, RING_BITS = E.WAVE_ATOMS, 256, 32
BOND_BINS = np.linspace(0.8, 2.4, 161)


def find(parent, i):
    while parent[i] != i:
        parent[i] = parent[parent[i]]
        i = parent[i]
    return i


def fragments(n, pairs):
    """Label per atom: the smallest index of its connected component."""
    parent = list(range(n))
    for i, j in pairs:
        a, b = find(parent, i), find(parent, j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(parent, i) for i in range(n)], np.int64)


def ring_of(nbrs, i, j):
    """1 + the distance from i to j without the bond (i, j); 0 when there is no other way."""
    dist = {i: 0}
    queue = collections.deque([i])
    while queue:
        u = queue.popleft()
        for v in nbrs[u]:
            if (u == i and v == j) or v in dist:
                continue
            dist[v] = dist[u] + 1
            if v == j:
                return dist[v] + 1
            queue.append(v)
    return 0


def ring_bit(r):
    return min(r, RING_BITS - 1)


def pair_index(a, b, n_el):
    a, b = min(a, b), max(a, b)
    return a * n_el - a * (a - 1) // 2 + (b - a)


def molecule(pos, slots, thr):
    """One molecule -> (orders (n, n), d (n, n), bonds [(i, j, order)], rings [per bond], frag (n,))."""
    d = E.distances(pos)
    o = E.bond_orders(d, slots, thr)
    n = len(slots)
    bonds = [(i, j, int(o[i, j])) for i in range(n) for j in range(i + 1, n) if o[i, j] > 0]
    nbrs = [np.flatnonzero(o[i] > 0).tolist() for i in range(n)]
    rings = [ring_of(nbrs, i, j) for i, j, _ in bonds]
    return o, d, bonds, rings, fragments(n, [(i, j) for i, j, _ in bonds])


def margin(pos, slots, thr):
    """The smallest relative distance of a pair's 100 * d from any of its three thresholds (NaN pairs and thresholds <= 0,
    which no distance can approach from below, left out)."""
    d = E.distances(pos)
    iu = np.triu_indices(len(slots), 1)
    p = 100 * d[iu]
    t = thr[:, slots[iu[0]], slots[iu[1]]]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(p[None] - t) / t
    rel = rel[(t > 0) & ~np.isnan(p)[None]]
    return float(rel.min()) if rel.size else np.inf


def graph(pos, classes, off, rule, class_slots, cc=(E.CC_BINS, 2.0), al=(E.ALL_BINS, 12.0), bl=BOND_BINS):
    """pos (F, N, 3), classes (F, N), off (B + 1) -> dict of the device outputs as numpy arrays."""
    pos, classes, off = np.asarray(pos), np.asarray(classes), np.asarray(off)
    F, N = classes.shape
    B, C, n_el = len(off) - 1, len(class_slots), len(rule.elements)
    thr, class_slots = rule.thresholds(), np.asarray(class_slots)
    carbon = np.flatnonzero(rule.elements == 6.0)
    P = n_el * (n_el + 1) // 2
    out = dict(nr_bonds=np.zeros((F, N), np.int32), degree=np.zeros((F, N), np.int32), frag=np.zeros((F, N), np.int32), ring=np.zeros((F, N), np.int32),
               n_bonds=np.zeros((F, B), np.int32), n_frags=np.zeros((F, B), np.int32), largest_frag=np.zeros((F, B), np.int32),
               complete=np.zeros((F, B), bool), n_cycles=np.zeros((F, B), np.int32), ring_sizes=np.zeros((F, B), np.int32),
               hist_bl=np.zeros((F, 2, P, 3, len(bl) + 1), np.int64), hist_cc=np.zeros((F, len(cc[0]) + 1), np.int64),
               hist_all=np.zeros((F, len(al[0]) + 1), np.int64), class_counts=np.zeros((F, C), np.int64), n_complete=np.zeros(F, np.int64),
               ring_counts=np.zeros((F, RING_BITS), np.int64))
    bond_list, bond_ring, offsets = [], [], [0]
    for f in range(F):
        for b in range(B):
            s = slice(off[b], off[b + 1])
            n = s.stop - s.start
            slots = class_slots[classes[f, s]]
            o, d, bonds, rings, frag = molecule(pos[f, s], slots, thr)
            out["nr_bonds"][f, s] = o.sum(1)
            out["degree"][f, s] = (o > 0).sum(1)
            out["frag"][f, s] = frag + off[b]
            ra = np.zeros(n, np.int64)
            bits = 0
            for (i, j, _), r in zip(bonds, rings):
                if r:
                    ra[i] = r if not ra[i] else min(ra[i], r)
                    ra[j] = r if not ra[j] else min(ra[j], r)
                    bits |= 1 << ring_bit(r)
            out["ring"][f, s] = ra
            sizes = np.bincount(frag, minlength=n)
            n_frags = int((sizes > 0).sum())
            complete = n_frags == 1
            out["n_bonds"][f, b], out["n_frags"][f, b], out["largest_frag"][f, b] = len(bonds), n_frags, sizes.max()
            out["complete"][f, b], out["n_cycles"][f, b] = complete, len(bonds) - n + n_frags
            out["ring_sizes"][f, b] = np.array(bits, np.uint32).astype(np.int32)
            for k in range(RING_BITS):
                out["ring_counts"][f, k] += bits >> k & 1
            for i, j, order in bonds:
                cell = (pair_index(slots[i], slots[j], n_el), order - 1, int(np.searchsorted(bl, d[i, j], side="left")))
                out["hist_bl"][(f, 0) + cell] += 1
                if complete:
                    out["hist_bl"][(f, 1) + cell] += 1
            if complete:
                out["n_complete"][f] += 1
                out["class_counts"][f] += np.bincount(classes[f, s], minlength=C)
                iu = np.triu_indices(n, 1)
                du = d[iu]
                if len(carbon):
                    both = (slots[iu[0]] == carbon[0]) & (slots[iu[1]] == carbon[0])
                    out["hist_cc"][f] += E.histogram(du[both], *cc)
                out["hist_all"][f] += E.histogram(du, *al)
            bond_list += [(i + off[b], j + off[b], order) for i, j, order in bonds]
            bond_ring += rings
            offsets.append(len(bond_list))
    out["bond_list"] = np.array(bond_list, np.int32).reshape(-1, 3)
    out["bond_ring"] = np.array(bond_ring, np.int32)
    out["bond_offsets"] = np.array(offsets, np.int64)
    return out
