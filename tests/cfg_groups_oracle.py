"""Test-local restatement of classifier-free guidance with one threshold statistic and one box per group of molecules: the
functions of tests/cfg_oracle.py applied to each group's slice of the atoms (a group is a contiguous run of atoms)."""
import torch

import cfg_oracle as O


def threshold_cfg_groups(x, cond, atom_off, threshold_type, threshold_args, boxes=None, strens=None, dtype=torch.float32):
    """threshold_CFG per group: group g is rows atom_off[g] .. atom_off[g + 1] - 1, boxes[g] its (3,2) box or None.  A group whose
    strength is 0 keeps its conditional prediction (the reference's else branch)."""
    outs = []
    for g in range(len(atom_off) - 1):
        sl = slice(int(atom_off[g]), int(atom_off[g + 1]))
        if strens is not None and strens[g] == 0:
            outs.append(cond[sl].to(dtype))
            continue
        outs.append(O.threshold_cfg(x[sl], cond[sl], threshold_type, threshold_args, None if boxes is None else boxes[g], dtype))
    return torch.cat(outs)


def combine_groups(cond, uncond, atom_off, strens, dtype=torch.float32):
    return torch.cat([O.combine(cond[int(a):int(b)], uncond[int(a):int(b)], w, dtype)
                      for a, b, w in zip(atom_off[:-1], atom_off[1:], strens)])


def statistic_groups(x, cond, atom_off, threshold_type, p):
    return [O.statistic(x[int(a):int(b)], cond[int(a):int(b)], threshold_type, p) for a, b in zip(atom_off[:-1], atom_off[1:])]
