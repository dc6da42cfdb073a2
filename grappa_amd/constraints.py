"""X-H bond constraints for the Langevin dynamics, fused and stepwise (`grappa_amd.dynamics`, csrc/dynamics_cons.hip and
csrc/dynamics_steps.hip; the loop is stated in include/grappa_hip.h at grappa_md_langevin_cons_f32).  Constraints come as star clusters: one centre atom and up to `MAX_LEAVES`
leaves, each held at one length from the centre (X-H, XH2, XH3, XH4); an atom belongs to at most one cluster.
  Constraints           the clusters of ONE molecule: `clusters` (K, 5) int32 -- the centre, then the leaves, -1 = no leaf, as atom
                        indices within the molecule -- and `lengths` (K, 4) float32 in Angstrom (0 where there is no leaf)
  hydrogen_constraints  every bond between a hydrogen and a heavy atom of a `Parameters`, at its predicted equilibrium length
  ConstraintBatch       the molecules of a batch concatenated, with `cluster_molptr`, for `HipBackend.md_langevin(constraints=...)` and `md_steps_cons`
Rigid water (SETTLE) and constraints other than these stars are out of scope."""
from typing import Optional, Sequence

import numpy as np
import torch

MAX_LEAVES = 4                 # GRAPPA_MD_CONS_MAX_LEAVES
TOLERANCE_DEFAULT = 2.0 ** -19
TOLERANCE_RANGE = (2.0 ** -20, 2.0 ** -7)


class Constraints:
    """the star clusters of one molecule (see the module text)"""

    def __init__(self, clusters, lengths):
        cl = np.asarray(clusters, dtype=np.int64).reshape(-1, MAX_LEAVES + 1)
        d = np.asarray(lengths, dtype=np.float64).reshape(-1, MAX_LEAVES)
        if cl.shape[0] != d.shape[0]:
            raise ValueError(f"clusters (K, {MAX_LEAVES + 1}) and lengths (K, {MAX_LEAVES}) must agree in K, got {cl.shape[0]} and {d.shape[0]}")
        used = cl[:, 1:] >= 0
        if (cl[:, 0] < 0).any() or (cl[:, 1:] < -1).any():
            raise ValueError("a cluster's centre must be an atom index and a leaf an atom index or -1")
        if not (used.sum(1) >= 1).all():
            raise ValueError("every cluster needs at least one leaf")
        atoms = np.concatenate([cl[:, 0], cl[:, 1:][used]])
        if len(np.unique(atoms)) != len(atoms):
            raise ValueError("an atom may belong to one cluster only, once")
        if not (np.isfinite(d[used]).all() and (d[used] > 0).all()):
            raise ValueError("constraint lengths must be finite and positive")
        self.clusters = cl.astype(np.int32)
        self.lengths = np.where(used, d, 0.0).astype(np.float32)

    @property
    def n_clusters(self) -> int:
        return int(self.clusters.shape[0])

    @property
    def n_constraints(self) -> int:
        return int((self.clusters[:, 1:] >= 0).sum())

    def pairs(self):
        """-> (centre (n,), leaf (n,), length (n,)): one entry per constrained bond"""
        k, j = np.nonzero(self.clusters[:, 1:] >= 0)
        return self.clusters[k, 0].astype(np.int64), self.clusters[k, 1 + j].astype(np.int64), self.lengths[k, j].astype(np.float64)

    def n_constraints_moving(self, masses) -> int:
        """the constraints with a moving end (mass > 0): those that remove a degree of freedom"""
        m = np.asarray(masses, dtype=np.float64).reshape(-1)
        c, l, _ = self.pairs()
        if len(c) and max(int(c.max()), int(l.max())) >= m.shape[0]:
            raise ValueError(f"the constraints name atom {max(int(c.max()), int(l.max()))}, the molecule has {m.shape[0]} atoms")
        return int(((m[c] > 0) | (m[l] > 0)).sum())

    @classmethod
    def from_bonds(cls, bonds, is_hydrogen, lengths) -> "Constraints":
        """bonds (T, 2) atom indices, is_hydrogen (n_atoms,) bool, lengths (T,) in Angstrom.  A bond is constrained if exactly one of
        its ends is a hydrogen; that hydrogen must have no other bond (ValueError).  H-H bonds are left free.  A centre with more than
        `MAX_LEAVES` hydrogens raises ValueError.  Clusters are ordered by their centre, leaves by their index."""
        bonds = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
        is_h = np.asarray(is_hydrogen, dtype=bool).reshape(-1)
        lengths = np.asarray(lengths, dtype=np.float64).reshape(-1)
        if lengths.shape[0] != bonds.shape[0]:
            raise ValueError(f"one length per bond ({bonds.shape[0]}), got {lengths.shape[0]}")
        if bonds.size and (bonds.min() < 0 or bonds.max() >= is_h.shape[0]):
            raise ValueError(f"a bond names an atom outside the molecule's {is_h.shape[0]} atoms")
        degree = np.bincount(bonds.reshape(-1), minlength=is_h.shape[0])
        stars = {}
        for (a, b), d in zip(bonds.tolist(), lengths.tolist()):
            if is_h[a] == is_h[b]:
                continue
            h, x = (a, b) if is_h[a] else (b, a)
            if degree[h] != 1:
                raise ValueError(f"hydrogen {h} is bonded to {int(degree[h])} atoms: only a hydrogen with one bond can be constrained")
            stars.setdefault(x, []).append((h, d))
        cl = np.full((len(stars), MAX_LEAVES + 1), -1, dtype=np.int64)
        dd = np.zeros((len(stars), MAX_LEAVES))
        for k, x in enumerate(sorted(stars)):
            leaves = sorted(stars[x])
            if len(leaves) > MAX_LEAVES:
                raise ValueError(f"atom {x} carries {len(leaves)} hydrogens: a cluster holds at most {MAX_LEAVES}")
            cl[k, 0] = x
            for j, (h, d) in enumerate(leaves):
                cl[k, 1 + j], dd[k, j] = h, d
        return cls(cl, dd)


def hydrogen_constraints(parameters, atomic_numbers) -> Constraints:
    """every X-H bond of `parameters` (a `Parameters`; atomic_numbers in the order of `parameters.atoms`) held at its predicted
    equilibrium length"""
    z = np.asarray(atomic_numbers).reshape(-1)
    ids = np.asarray(parameters.atoms).reshape(-1)
    if z.shape[0] != ids.shape[0]:
        raise ValueError(f"one atomic number per atom ({ids.shape[0]}), got {z.shape[0]}")
    pos = {int(a): k for k, a in enumerate(ids.tolist())}
    bonds = np.array([[pos[int(a)], pos[int(b)]] for a, b in np.asarray(parameters.bonds).reshape(-1, 2).tolist()], dtype=np.int64).reshape(-1, 2)
    return Constraints.from_bonds(bonds, z == 1, np.asarray(parameters.bond_eq, dtype=np.float64).reshape(-1))


class ConstraintBatch:
    """the constraints of a batch's molecules, in the batch's order (None: a molecule without constraints): `cluster_molptr` (B+1,)
    int32, `cluster_atoms` (K, 5) int32, `cluster_d` (K, 4) float32 and the relative tolerance on a length"""

    def __init__(self, items: Sequence[Optional[Constraints]], tolerance: float = TOLERANCE_DEFAULT):
        items = list(items)
        for c in items:
            if c is not None and not isinstance(c, Constraints):
                raise TypeError(f"expected Constraints or None per molecule, got {type(c).__name__}")
        if isinstance(tolerance, bool) or not isinstance(tolerance, (int, float, np.integer, np.floating)) \
                or not (TOLERANCE_RANGE[0] <= float(tolerance) <= TOLERANCE_RANGE[1]):
            raise ValueError(f"tolerance must lie in [2^-20, 2^-7], got {tolerance!r}")
        self.items = items
        self.tolerance = float(tolerance)
        self.B = len(items)
        counts = [0 if c is None else c.n_clusters for c in items]
        self.cluster_molptr = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
        some = [c for c in items if c is not None]
        self.cluster_atoms = torch.from_numpy(np.concatenate([c.clusters for c in some] + [np.zeros((0, MAX_LEAVES + 1), np.int32)]))
        self.cluster_d = torch.from_numpy(np.concatenate([c.lengths for c in some] + [np.zeros((0, MAX_LEAVES), np.float32)]))
        self.K = int(self.cluster_atoms.shape[0])

    def to(self, device) -> "ConstraintBatch":
        out = ConstraintBatch.__new__(ConstraintBatch)
        out.items, out.tolerance, out.B, out.K = self.items, self.tolerance, self.B, self.K
        out.cluster_molptr, out.cluster_atoms, out.cluster_d = (t.to(device) for t in (self.cluster_molptr, self.cluster_atoms, self.cluster_d))
        return out

    def check_masses(self, masses, atom_counts) -> None:
        """ValueError for a cluster that its frozen atoms over-determine: a moving centre cannot hold `MAX_LEAVES` fixed lengths to
        frozen leaves (three fix it; the velocity projection's system is then singular)"""
        m = np.asarray(masses, dtype=np.float64).reshape(-1)
        ptr = np.concatenate([[0], np.cumsum([int(n) for n in atom_counts])]).astype(np.int64)
        if len(ptr) != self.B + 1 or ptr[-1] != m.shape[0]:
            raise ValueError(f"expected the atom counts of {self.B} molecules adding up to {m.shape[0]} masses")
        for b, c in enumerate(self.items):
            if c is None or c.n_clusters == 0:
                continue
            mm = m[ptr[b]:ptr[b + 1]]
            if int(c.clusters.max()) >= mm.shape[0]:
                raise ValueError(f"the constraints of molecule {b} name atom {int(c.clusters.max())}, the molecule has {mm.shape[0]} atoms")
            leaves = c.clusters[:, 1:]
            frozen = ((leaves >= 0) & (mm[np.clip(leaves, 0, None)] <= 0)).sum(1)
            bad = np.nonzero((mm[c.clusters[:, 0]] > 0) & (frozen >= MAX_LEAVES))[0]
            if len(bad):
                raise ValueError(f"molecule {b}: the moving atom {int(c.clusters[bad[0], 0])} is constrained to {MAX_LEAVES} frozen atoms, "
                                 f"which over-determine it (freeze it too, or drop a constraint)")

    def n_constraints_host(self, masses, atom_counts) -> np.ndarray:
        """(B,) int64: per molecule, the constraints with a moving end.  masses (N,) on the host, atom_counts: atoms per molecule"""
        m = np.asarray(masses, dtype=np.float64).reshape(-1)
        counts = [int(n) for n in atom_counts]
        if len(counts) != self.B or sum(counts) != m.shape[0]:
            raise ValueError(f"expected the atom counts of {self.B} molecules adding up to {m.shape[0]} masses")
        ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return np.array([0 if c is None else c.n_constraints_moving(m[ptr[b]:ptr[b + 1]]) for b, c in enumerate(self.items)], dtype=np.int64)
