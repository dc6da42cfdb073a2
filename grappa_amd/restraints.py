"""Restraints for the fused FIRE minimiser (`grappa_amd.relax`, csrc/relax.hip; the objective is stated in include/grappa_hip.h at
grappa_relax_fire_restr_f32) and for the stepwise dynamics (`grappa_amd.dynamics`, csrc/md_restr.h; grappa_md_steps_*_restr_f32):
frozen atoms, harmonic tethers to the start coordinates (in the dynamics: to `restraint_reference`, by default the start) and periodic
dihedral restraints k (1 - cos(phi - target)) with one target per conformation -- what "optimise the hydrogens only", "relax, but stay
near the input", a relaxed torsion scan, a restrained equilibration and the windows of an umbrella run along a torsion need.  In the
dynamics a frozen atom is an atom of mass 0: `simulate` folds `frozen` into the masses.
  Restraints      the restraints of ONE molecule, atom indices in the order of the molecule's atoms
  RestraintBatch  the molecules of a batch concatenated, with `dih_molptr`, for `HipBackend.relax_fire(restraints=...)`
  set_dihedral    host numpy: rotate one side of a bond rigidly so that a dihedral takes a value (the starts of a torsion scan)
Units: Angstrom, kcal/mol, radians.  Distance and angle restraints, flat-bottomed wells, time-dependent targets, restraints on the
stepwise minimiser and on the fused dynamics are out of scope."""
from typing import Optional, Sequence

import numpy as np
import torch

MAX_DIHEDRALS = 16             # GRAPPA_RELAX_MAX_DIHEDRALS


class Restraints:
    """frozen (n,) bool or None; position_k (n,) kcal/mol/A^2 or None (0: no tether; the tether is to the START coordinates);
    dihedrals (R, 4) atom indices with dihedral_k (R,) kcal/mol (a scalar serves all) and dihedral_targets (R,) or (R, C) in radians
    ((R,): the same target in every conformation).  ValueError for everything the kernel would refuse (status 5)."""

    def __init__(self, frozen=None, position_k=None, dihedrals=None, dihedral_k=None, dihedral_targets=None):
        self.frozen = None if frozen is None else np.asarray(frozen).reshape(-1).astype(bool)
        self.position_k = None
        if position_k is not None:
            pk = np.asarray(position_k, dtype=np.float64).reshape(-1)
            if not (np.isfinite(pk).all() and (pk >= 0).all()):
                raise ValueError("position_k must be finite and non-negative")
            self.position_k = pk.astype(np.float32)
        if self.frozen is not None and self.position_k is not None and self.frozen.shape != self.position_k.shape:
            raise ValueError(f"frozen ({self.frozen.shape[0]},) and position_k ({self.position_k.shape[0]},) must name the same atoms")
        if dihedrals is None:
            if dihedral_k is not None or dihedral_targets is not None:
                raise ValueError("dihedral_k and dihedral_targets need dihedrals")
            dihedrals, dihedral_k, dihedral_targets = np.zeros((0, 4)), np.zeros(0), np.zeros(0)
        elif dihedral_k is None or dihedral_targets is None:
            raise ValueError("dihedrals need dihedral_k and dihedral_targets")
        d = np.asarray(dihedrals)
        if d.size and not np.issubdtype(d.dtype, np.integer):
            raise ValueError(f"dihedrals must be integer atom indices, got {d.dtype}")
        if d.ndim != 2 and d.size % 4:
            raise ValueError(f"dihedrals must be (R, 4), got {d.shape}")
        d = d.astype(np.int64).reshape(-1, 4)
        R = d.shape[0]
        if R > MAX_DIHEDRALS:
            raise ValueError(f"{R} restrained dihedrals: a molecule takes at most {MAX_DIHEDRALS}")
        if (d < 0).any():
            raise ValueError("a dihedral names a negative atom index")
        if any(len(set(row)) != 4 for row in d.tolist()):
            raise ValueError("the four atoms of a dihedral must be distinct")
        k = np.asarray(dihedral_k, dtype=np.float64)
        k = np.full(R, float(k)) if k.ndim == 0 else k.reshape(-1)
        if k.shape[0] != R:
            raise ValueError(f"one dihedral_k per dihedral ({R}), got {k.shape[0]}")
        if not (np.isfinite(k).all() and (k >= 0).all()):
            raise ValueError("dihedral_k must be finite and non-negative")
        t = np.asarray(dihedral_targets, dtype=np.float64)
        if t.ndim == 0:
            t = np.full(R, float(t))
        if t.ndim not in (1, 2) or t.shape[0] != R:
            raise ValueError(f"dihedral_targets must be ({R},) or ({R}, C), got {t.shape}")
        if not np.isfinite(t).all():
            raise ValueError("dihedral_targets must be finite")
        self.dihedrals, self.dihedral_k, self.dihedral_targets = d.astype(np.int32), k.astype(np.float32), t.astype(np.float32)

    @property
    def n_dihedrals(self) -> int:
        return int(self.dihedrals.shape[0])

    @property
    def n_atoms(self) -> Optional[int]:
        """the atoms the per-atom arrays name (None: neither frozen nor position_k is given)"""
        for a in (self.frozen, self.position_k):
            if a is not None:
                return int(a.shape[0])
        return None

    @property
    def empty(self) -> bool:
        return self.frozen is None and self.position_k is None and self.n_dihedrals == 0

    def targets(self, C: int) -> np.ndarray:
        """(R, C) float32"""
        t = self.dihedral_targets
        if t.ndim == 1:
            return np.repeat(t[:, None], C, axis=1)
        if t.shape[1] != C:
            raise ValueError(f"dihedral_targets holds {t.shape[1]} conformations, the call has {C}")
        return t


class RestraintBatch:
    """the restraints of a batch's molecules for C conformations, in the batch's order (None: an unrestrained molecule): `dih_molptr`
    (B+1,) int32, `dih_atoms` (R, 4) int32, `dih_k` (R,) float32, `dih_target` (R, C) float32 and -- None when no molecule has any,
    (N,) once `atom_counts` is known -- `frozen` int32 and `pos_k` float32.  atom_counts: atoms per molecule; required when a molecule
    has frozen atoms or tethers and another gives no per-atom array, and checked against every index when given."""

    def __init__(self, items: Sequence[Optional[Restraints]], C: int, atom_counts=None):
        items = list(items)
        for r in items:
            if r is not None and not isinstance(r, Restraints):
                raise TypeError(f"expected Restraints or None per molecule, got {type(r).__name__}")
        if isinstance(C, bool) or not isinstance(C, (int, np.integer)) or C < 0:
            raise ValueError(f"C must be a non-negative integer, got {C!r}")
        self.items, self.C, self.B = items, int(C), len(items)
        counts = None if atom_counts is None else [int(n) for n in atom_counts]
        if counts is not None and len(counts) != self.B:
            raise ValueError(f"atom_counts names {len(counts)} molecules, the batch has {self.B}")
        some = [r for r in items if r is not None]
        self.dih_molptr = torch.from_numpy(np.concatenate([[0], np.cumsum([0 if r is None else r.n_dihedrals for r in items])]).astype(np.int32))
        self.dih_atoms = torch.from_numpy(np.concatenate([r.dihedrals for r in some] + [np.zeros((0, 4), np.int32)]))
        self.dih_k = torch.from_numpy(np.concatenate([r.dihedral_k for r in some] + [np.zeros(0, np.float32)]))
        self.dih_target = torch.from_numpy(np.ascontiguousarray(np.concatenate([r.targets(self.C) for r in some] + [np.zeros((0, self.C), np.float32)])))
        self.R = int(self.dih_atoms.shape[0])
        per_atom = any(r.frozen is not None or r.position_k is not None for r in some)
        self.frozen = self.pos_k = None
        self.atom_counts = counts
        if counts is None:
            if per_atom and any(r is None or r.n_atoms is None for r in items):
                raise ValueError("atom_counts is required: a molecule has frozen atoms or tethers, another gives no per-atom array")
            counts = [r.n_atoms for r in items] if per_atom else None
        if counts is not None:
            for b, r in enumerate(items):
                if r is None:
                    continue
                if r.n_atoms is not None and r.n_atoms != counts[b]:
                    raise ValueError(f"molecule {b}: the restraints name {r.n_atoms} atoms, the molecule has {counts[b]}")
                if r.n_dihedrals and int(r.dihedrals.max()) >= counts[b]:
                    raise ValueError(f"molecule {b}: a dihedral names atom {int(r.dihedrals.max())}, the molecule has {counts[b]} atoms")
            self.atom_counts = counts
        if per_atom:
            fz = [np.zeros(n, np.int32) if r is None or r.frozen is None else r.frozen.astype(np.int32) for r, n in zip(items, counts)]
            pk = [np.zeros(n, np.float32) if r is None or r.position_k is None else r.position_k for r, n in zip(items, counts)]
            if any(r is not None and r.frozen is not None for r in items):
                self.frozen = torch.from_numpy(np.concatenate(fz + [np.zeros(0, np.int32)]))
            if any(r is not None and r.position_k is not None for r in items):
                self.pos_k = torch.from_numpy(np.concatenate(pk + [np.zeros(0, np.float32)]))

    @property
    def empty(self) -> bool:
        return self.R == 0 and self.frozen is None and self.pos_k is None

    def to(self, device) -> "RestraintBatch":
        out = RestraintBatch.__new__(RestraintBatch)
        out.items, out.C, out.B, out.R, out.atom_counts = self.items, self.C, self.B, self.R, self.atom_counts
        out.dih_molptr, out.dih_atoms, out.dih_k, out.dih_target = (t.to(device) for t in (self.dih_molptr, self.dih_atoms, self.dih_k, self.dih_target))
        out.frozen = None if self.frozen is None else self.frozen.to(device)
        out.pos_k = None if self.pos_k is None else self.pos_k.to(device)
        return out


def dihedral_angle(xyz, i, j, k, l) -> float:
    """the library's dihedral (include/grappa_hip.h; the reference's sign convention) of four rows of xyz (n, 3), float64"""
    x = np.asarray(xyz, dtype=np.float64)
    a, b, c = x[j] - x[i], x[j] - x[k], x[l] - x[k]
    n1, n2 = np.cross(a, b), np.cross(b, c)
    return float(np.arctan2(np.dot(np.cross(n1, n2), b) / np.linalg.norm(b), np.dot(n1, n2)))


def rotating_side(n_atoms: int, bonds, j: int, k: int):
    """the atoms on k's side of the bond j-k in the bond graph (k itself included): (n,) bool, or None if j-k lies in a ring (k's side
    reaches j without the bond)"""
    nbrs = [[] for _ in range(n_atoms)]
    for a, b in np.asarray(bonds, dtype=np.int64).reshape(-1, 2).tolist():
        nbrs[a].append(b)
        nbrs[b].append(a)
    side = np.zeros(n_atoms, dtype=bool)
    side[k] = True
    stack = [k]
    while stack:
        a = stack.pop()
        for b in nbrs[a]:
            if a == k and b == j:
                continue
            if b == j:
                return None
            if not side[b]:
                side[b] = True
                stack.append(b)
    return side


def set_dihedral(xyz, bonds, dihedral, target: float) -> np.ndarray:
    """xyz (n, 3) with the l-side of the bond j-k of dihedral = (i, j, k, l) rotated rigidly about that bond so that the dihedral equals
    `target` (radians), in float64.  bonds (T, 2): atom indices.  Bond lengths, and every angle and dihedral that does not span the
    rotation, are unchanged; the i-side does not move.  If j-k lies in a ring nothing is rotated: a copy of the input."""
    x = np.array(xyz, dtype=np.float64)
    i, j, k, l = (int(a) for a in dihedral)
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError(f"xyz must be (n_atoms, 3), got {x.shape}")
    if len({i, j, k, l}) != 4 or min(i, j, k, l) < 0 or max(i, j, k, l) >= x.shape[0]:
        raise ValueError(f"the dihedral {(i, j, k, l)} must name four distinct atoms of the molecule's {x.shape[0]}")
    if not np.isfinite(target):
        raise ValueError("the target must be finite")
    side = rotating_side(x.shape[0], bonds, j, k)
    if side is None or side[i] or not side[l]:
        return x
    # with this sign convention a rotation of the l-side by +delta about the axis k -> j raises phi by delta
    axis = (x[j] - x[k]) / np.linalg.norm(x[j] - x[k])
    for _ in range(2):          # (the second pass removes the rounding of the first)
        delta = target - dihedral_angle(x, i, j, k, l)
        r = x[side] - x[k]
        c, s = np.cos(delta), np.sin(delta)
        x[side] = x[k] + r * c + np.cross(axis, r) * s + np.outer(r @ axis, axis) * (1.0 - c)
    return x
