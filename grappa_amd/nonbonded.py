"""Nonbonded (Lennard-Jones + Coulomb) energies and gradients on the device: the half of a molecular-mechanics force field that
Grappa does not predict.  With it `E_QM - E_nonbonded` -- the `energy_ref` / `gradient_ref` of a training record -- can be made here
(`MolData.from_arrays`, `MolData.with_nonbonded`), where the reference asks OpenMM (data/MolData.py:105-151, :476-494).

Semantics: OpenMM's `NonbondedForce` with `NoCutoff`, in this project's units (Angstrom, kcal/mol, elementary charges):

    E = sum_{i<j, (i,j) no exception} 4 eps_ij ((s_ij/r)^12 - (s_ij/r)^6) + K q_i q_j / r
      + sum_{exceptions p=(i,j)}      4 eps_p  ((s_p /r)^12 - (s_p /r)^6) + K qq_p / r
    s_ij = (sigma_i + sigma_j)/2, eps_ij = sqrt(eps_i eps_j), K = constants.COULOMB_CONSTANT;   gradient = +dE/dxyz (not the force)

An exception replaces the pair's interaction; with epsilon 0 and charge product 0 it is an exclusion, which is never evaluated (two
excluded atoms may sit on one point).  A non-excluded pair at zero distance gives inf / NaN, as in OpenMM.  Atoms of different
molecules of a batch never interact.

With `cutoff=` (a `Cutoff`, or a plain distance) the semantics are those of OpenMM's `CutoffNonPeriodic`: a pair that is no exception
contributes only below the cutoff rc, its Lennard-Jones energy times the switch S (1 up to `switch_distance` rs, then
1 - 10 u^3 + 15 u^4 - 6 u^5 with u = (r - rs)/(rc - rs)), its Coulomb energy as the reaction field K q_i q_j (1/r + k_rf r^2 - c_rf) with
k_rf = (eps - 1)/((2 eps + 1) rc^3), c_rf = 3 eps/((2 eps + 1) rc), which vanishes at rc.  Exceptions are not cut: an exception is
evaluated at any distance with the plain formulas.  The kernel skips whole tiles of 64 x 64 atoms whose bounding boxes lie farther apart
than rc (include/grappa_hip.h grappa_nb_cut states the rule); the bits do not depend on it.

The arithmetic runs in csrc/nonbonded.hip through `HipBackend.nonbonded`; there is no CPU evaluator.  Out of scope: gradients with
respect to charges, sigma or epsilon; periodic boxes, PME, a long-range Lennard-Jones correction.
"""
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

_KEYS = ("charge", "sigma", "epsilon", "exception_idx", "exception_chargeprod", "exception_sigma", "exception_epsilon")


@dataclass(frozen=True)
class Cutoff:
    """a nonbonded cutoff (grappa_nb_cut): distance rc in Angstrom (finite, > 0); switch_distance None or 0 (no switch) or inside
    (0, distance); rf_dielectric finite and >= 1 (1: no reaction field, a shifted Coulomb).  prune=False evaluates every tile: the same
    bits, slower -- it is there to measure what the skipped tiles are worth."""
    distance: float
    switch_distance: Optional[float] = None
    rf_dielectric: float = 78.3
    prune: bool = True

    def __post_init__(self):
        num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))      # noqa: E731
        if not num(self.distance) or not (math.isfinite(self.distance) and self.distance > 0):
            raise ValueError(f"cutoff: distance must be a finite number > 0, got {self.distance!r}")
        rs = self.switch_distance
        if rs is not None and (not num(rs) or not (rs == 0 or 0 < rs < self.distance)):
            raise ValueError(f"cutoff: switch_distance must be None, 0 or inside (0, {self.distance}), got {rs!r}")
        if not num(self.rf_dielectric) or not (math.isfinite(self.rf_dielectric) and self.rf_dielectric >= 1):
            raise ValueError(f"cutoff: rf_dielectric must be a finite number >= 1, got {self.rf_dielectric!r}")
        if not isinstance(self.prune, (bool, np.bool_)):
            raise ValueError(f"cutoff: prune must be True or False, got {self.prune!r}")

    def as_opts(self) -> dict:
        """the four fields of grappa_nb_cut by name"""
        return {"cutoff": float(self.distance), "switch_distance": float(self.switch_distance or 0.0), "rf_dielectric": float(self.rf_dielectric),
                "prune": int(bool(self.prune))}


def as_cutoff(cutoff: Union[None, float, "Cutoff"]) -> Optional["Cutoff"]:
    """None, a `Cutoff`, or a plain distance (-> Cutoff(distance)), checked"""
    if cutoff is None or isinstance(cutoff, Cutoff):
        return cutoff
    return Cutoff(cutoff)


def _f64(x, shape=None):
    a = np.asarray(x, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


@dataclass
class NonbondedParameters:
    """per-atom charge (e), sigma (A), epsilon (kcal/mol) of one molecule and its exceptions (atom index pairs with their own
    charge product, sigma, epsilon), as OpenMM's NonbondedForce holds them"""
    charge: np.ndarray
    sigma: np.ndarray
    epsilon: np.ndarray
    exception_idx: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), dtype=np.int64))
    exception_chargeprod: np.ndarray = field(default_factory=lambda: np.zeros(0))
    exception_sigma: np.ndarray = field(default_factory=lambda: np.zeros(0))
    exception_epsilon: np.ndarray = field(default_factory=lambda: np.zeros(0))

    def __post_init__(self):
        self.charge, self.sigma, self.epsilon = _f64(self.charge), _f64(self.sigma), _f64(self.epsilon)
        self.exception_idx = np.asarray(self.exception_idx, dtype=np.int64)
        if self.exception_idx.size == 0:
            self.exception_idx = self.exception_idx.reshape(0, 2)
        self.exception_chargeprod, self.exception_sigma, self.exception_epsilon = (
            _f64(self.exception_chargeprod), _f64(self.exception_sigma), _f64(self.exception_epsilon))

    @property
    def n_atoms(self) -> int:
        return int(self.charge.shape[0])

    def validate(self) -> "NonbondedParameters":
        n = self.charge.shape[0] if self.charge.ndim == 1 else -1
        if n < 0 or self.sigma.shape != (n,) or self.epsilon.shape != (n,):
            raise ValueError(f"charge, sigma, epsilon must share the shape (n,), got {self.charge.shape}, {self.sigma.shape}, {self.epsilon.shape}")
        idx = self.exception_idx
        if idx.ndim != 2 or idx.shape[1] != 2:
            raise ValueError(f"exception_idx must be (P, 2), got {idx.shape}")
        P = idx.shape[0]
        for k in ("exception_chargeprod", "exception_sigma", "exception_epsilon"):
            if getattr(self, k).shape != (P,):
                raise ValueError(f"{k} must be ({P},), got {getattr(self, k).shape}")
        if P and (idx.min() < 0 or idx.max() >= n):
            raise ValueError(f"exception_idx: atom index outside [0, {n})")
        if (idx[:, 0] == idx[:, 1]).any():
            raise ValueError("exception_idx: an atom cannot be excepted from itself")
        key = idx.min(axis=1) * max(n, 1) + idx.max(axis=1)
        if np.unique(key).shape[0] != P:
            raise ValueError("exception_idx: a pair appears twice (in either order)")
        if (self.sigma < 0).any() or (self.epsilon < 0).any() or (self.exception_sigma < 0).any() or (self.exception_epsilon < 0).any():
            raise ValueError("sigma and epsilon must not be negative")
        return self

    # (not the `nonbonded_` prefix: in the reference's record schema that one names energies)
    def to_dict(self) -> Dict[str, np.ndarray]:
        return {f"nbparam_{k}": getattr(self, k) for k in _KEYS}

    @classmethod
    def from_dict(cls, d) -> "NonbondedParameters":
        return cls(**{k: np.asarray(d[f"nbparam_{k}"]) for k in _KEYS})

    @classmethod
    def from_bonds(cls, bonds, charge, sigma, epsilon, coulomb14scale: float = 1 / 1.2, lj14scale: float = 0.5) -> "NonbondedParameters":
        """exceptions as OpenMM's createExceptionsFromBonds makes them: pairs one or two bonds apart are exclusions; pairs three bonds
        apart that are not also one or two bonds apart are 1-4 exceptions with qq = coulomb14scale q_i q_j, sigma = (s_i + s_j)/2,
        eps = lj14scale sqrt(e_i e_j).  `bonds`: (m, 2) atom indices.  Each pair appears once, as (low, high), in ascending order."""
        from . import _hostlib
        q, s, e = _f64(charge), _f64(sigma), _f64(epsilon)
        n = q.shape[0]
        b = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
        if b.size and (b.min() < 0 or b.max() >= n):
            raise ValueError(f"bonds: atom index outside [0, {n})")

        def keys(lo, hi):          # unordered pairs as one integer, self pairs dropped (the ends of a ring's torsion can meet)
            lo, hi = np.minimum(lo, hi).astype(np.int64), np.maximum(lo, hi).astype(np.int64)
            return np.unique((lo * n + hi)[lo != hi])

        if b.shape[0]:
            angles, propers = _hostlib.enumerate_tuples(b)          # the ends of the angles / proper torsions: two / three bonds apart
            excl = np.union1d(keys(b[:, 0], b[:, 1]), keys(angles[:, 0], angles[:, 2]))
            k14 = np.setdiff1d(keys(propers[:, 0], propers[:, 3]), excl)
        else:
            excl = k14 = np.zeros(0, dtype=np.int64)
        key = np.concatenate([excl, k14])
        is14 = np.concatenate([np.zeros(excl.shape[0], bool), np.ones(k14.shape[0], bool)])
        order = np.argsort(key, kind="stable")
        key, is14 = key[order], is14[order]
        i, j = key // max(n, 1), key % max(n, 1)
        return cls(charge=q, sigma=s, epsilon=e, exception_idx=np.stack([i, j], axis=1).reshape(-1, 2),
                   exception_chargeprod=np.where(is14, coulomb14scale * q[i] * q[j], 0.0),
                   exception_sigma=np.where(is14, 0.5 * (s[i] + s[j]), 1.0),
                   exception_epsilon=np.where(is14, lj14scale * np.sqrt(e[i] * e[j]), 0.0)).validate()


class NonbondedBatch:
    """the kernel's view of a list of molecules: concatenated per-atom tables, atom_molptr, and the exception table as a symmetric CSR
    over the atoms (every exception on both of its atoms, batch-global partner indices ascending per atom).  Built on the host with
    numpy; `.to(device)` uploads it once."""
    _TENSORS = ("atom_molptr", "charge", "sigma", "epsilon", "exc_ptr", "exc_atom", "exc_qq", "exc_sigma", "exc_eps")

    def __init__(self, params: Sequence[NonbondedParameters]):
        params = [p.validate() for p in params]
        counts = np.array([p.n_atoms for p in params], dtype=np.int64)
        ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        if ptr[-1] >= 2 ** 31:
            raise ValueError("NonbondedBatch: more than 2^31 atoms")
        self.B, self.N = len(params), int(ptr[-1])
        cat = lambda xs, dt: np.concatenate([np.asarray(x, dtype=dt).reshape(-1) for x in xs]) if xs else np.zeros(0, dt)      # noqa: E731
        a = cat([p.exception_idx[:, 0] + o for p, o in zip(params, ptr)], np.int64)
        b = cat([p.exception_idx[:, 1] + o for p, o in zip(params, ptr)], np.int64)
        own, partner = np.concatenate([a, b]), np.concatenate([b, a])
        order = np.lexsort((partner, own))
        both = lambda k: np.tile(cat([getattr(p, k) for p in params], np.float32), 2)[order]      # noqa: E731
        exc = {"exc_atom": partner[order].astype(np.int32), "exc_qq": both("exception_chargeprod"), "exc_sigma": both("exception_sigma"),
               "exc_eps": both("exception_epsilon")}
        self.n_exceptions = int(a.shape[0])
        if not self.n_exceptions:          # the C ABI wants non-NULL tables: one element nobody reads
            exc = {k: np.zeros(1, v.dtype) for k, v in exc.items()}
        host = {"atom_molptr": ptr.astype(np.int32), "charge": cat([p.charge for p in params], np.float32),
                "sigma": cat([p.sigma for p in params], np.float32), "epsilon": cat([p.epsilon for p in params], np.float32),
                "exc_ptr": np.concatenate([[0], np.cumsum(np.bincount(own, minlength=self.N))]).astype(np.int32), **exc}
        for k in self._TENSORS:
            setattr(self, k, torch.from_numpy(np.ascontiguousarray(host[k])))
        self._molptr_host = self.atom_molptr          # stays on the host: the kernel's work-item lists are built from it
        self._plans = {}                              # C -> HipBackend.nonbonded_plan(...), on the batch's device

    @property
    def atom_molptr_host(self) -> torch.Tensor:
        """atom_molptr as the int32 host tensor the batch was built with, wherever `.to` has put the tables"""
        return self._molptr_host

    def plan_for(self, n_confs: int, device):
        """the work-item list of these molecules for C = n_confs on `device` (`HipBackend.nonbonded_plan`), made once and kept: what the
        pair kernels of the nonbonded term and of the implicit solvent (`grappa_amd.solvent`) walk"""
        from .backend import get_backend
        plan = self._plans.get(n_confs)
        if plan is None or (plan[0] is not None and plan[0].device != torch.device(device)):
            plan = self._plans[n_confs] = get_backend().nonbonded_plan(self._molptr_host, self.N, n_confs, device)
        return plan

    def to(self, device) -> "NonbondedBatch":
        for k in self._TENSORS:
            setattr(self, k, getattr(self, k).to(device))
        self._plans = {}
        return self

    def exceptions_of(self, b: int):
        """the table read back: molecule b's exceptions as (idx (P,2) molecule-local with low < high, chargeprod, sigma, epsilon)"""
        ptr, eptr = self.atom_molptr.cpu().numpy(), self.exc_ptr.cpu().numpy()
        a0, a1 = int(ptr[b]), int(ptr[b + 1])
        lo, hi = int(eptr[a0]), int(eptr[a1])
        if not self.n_exceptions:
            hi = lo
        own = np.repeat(np.arange(a0, a1), np.diff(eptr[a0:a1 + 1]))
        partner = self.exc_atom.cpu().numpy()[lo:hi].astype(np.int64)
        keep = own < partner
        col = lambda t: t.cpu().numpy()[lo:hi][keep]      # noqa: E731
        return np.stack([own[keep] - a0, partner[keep] - a0], axis=1).reshape(-1, 2), col(self.exc_qq), col(self.exc_sigma), col(self.exc_eps)

    def evaluate(self, xyz: torch.Tensor, terms: bool = False, gradient: bool = True, cutoff=None):
        """xyz (N, C, 3) float32 on the batch's device (the layout of g.nodes['n1'].data['xyz']) -> energy (B, C), gradient (N, C, 3)
        [, term_energy (2, B, C): Lennard-Jones, Coulomb].  gradient=False: (energy, None [, term_energy]).  cutoff: a `Cutoff` or a
        distance (None: all pairs, the call it always was)."""
        from .backend import get_backend
        cutoff = as_cutoff(cutoff)
        if not isinstance(xyz, torch.Tensor) or xyz.dim() != 3 or xyz.shape[2] != 3 or xyz.dtype != torch.float32:
            raise ValueError(f"xyz must be a float32 (N, C, 3) tensor, got {getattr(xyz, 'dtype', type(xyz))} {tuple(getattr(xyz, 'shape', ()))}")
        if xyz.shape[0] != self.N or xyz.device != self.charge.device:
            raise ValueError(f"xyz has {xyz.shape[0]} atoms on {xyz.device}, the batch {self.N} on {self.charge.device}")
        xyz = xyz.contiguous()
        C = xyz.shape[1]
        be = get_backend()
        plan = self._plans.get(C)
        if plan is None and hasattr(be, "nonbonded_plan"):
            plan = self._plans[C] = be.nonbonded_plan(self._molptr_host, self.N, C, xyz.device)
        energy = torch.zeros(self.B, C, dtype=torch.float32, device=xyz.device)
        grad = torch.zeros_like(xyz) if gradient else None
        te = torch.zeros(2, self.B, C, dtype=torch.float32, device=xyz.device) if terms else None
        extra = {} if cutoff is None else {"cutoff": cutoff}
        be.nonbonded(xyz, self.atom_molptr, self.charge, self.sigma, self.epsilon, self.exc_ptr, self.exc_atom, self.exc_qq, self.exc_sigma,
                     self.exc_eps, energy, te, grad, plan=plan, **extra)
        return (energy, grad, te) if terms else (energy, grad)


def nonbonded_energy(params, xyz, device="cuda", terms: bool = False, cutoff=None):
    """Energies and gradients of one molecule or a list of molecules, numpy in and out.  xyz: (n_confs, n_atoms, 3) in Angstrom (the
    MolData convention), or a list of such arrays sharing n_confs, one per NonbondedParameters.
    -> (energy (n_confs,), gradient (n_confs, n_atoms, 3)) in kcal/mol and kcal/mol/A, with terms=True followed by the Lennard-Jones
    and the Coulomb part of the energy; for a list, a list of such tuples.  cutoff: a `Cutoff` or a distance (None: all pairs)."""
    cutoff = as_cutoff(cutoff)
    single = isinstance(params, NonbondedParameters)
    plist: List[NonbondedParameters] = [params] if single else list(params)
    xs = [np.asarray(xyz)] if single else [np.asarray(x) for x in xyz]
    if len(xs) != len(plist):
        raise ValueError(f"{len(plist)} parameter sets but {len(xs)} coordinate arrays")
    for p, x in zip(plist, xs):
        if x.ndim != 3 or x.shape[1:] != (p.n_atoms, 3) or x.shape[0] != xs[0].shape[0]:
            raise ValueError(f"xyz must be (n_confs, {p.n_atoms}, 3) with one n_confs for all molecules, got {x.shape}")
    nb = NonbondedBatch(plist).to(device)
    flat = np.concatenate([x.transpose(1, 0, 2) for x in xs], axis=0).astype(np.float32)
    out = nb.evaluate(torch.from_numpy(np.ascontiguousarray(flat)).to(device), terms=terms, **({} if cutoff is None else {"cutoff": cutoff}))
    energy, grad = out[0].cpu().numpy(), out[1].cpu().numpy()
    te = out[2].cpu().numpy() if terms else None
    ptr = nb.atom_molptr.cpu().numpy()
    res = []
    for b in range(len(plist)):
        r = (energy[b].astype(np.float64), grad[ptr[b]:ptr[b + 1]].transpose(1, 0, 2).astype(np.float64))
        res.append(r + (te[0, b].astype(np.float64), te[1, b].astype(np.float64)) if terms else r)
    return res[0] if single else res


def from_pdb(pdb_path: str, ffxml_path: str):
    """a protein structure file and an OpenMM force-field XML -> (the dict of pdb.graph_from_pdb, NonbondedParameters): charges, sigma
    (nm -> A) and epsilon (kJ/mol -> kcal/mol) per atom from the XML's <NonbondedForce> block, exceptions from the bonds with the
    block's coulomb14scale / lj14scale"""
    from .pdb import ForceFieldTemplates, typed_graph_from_pdb
    ff = ForceFieldTemplates(ffxml_path)
    g, types = typed_graph_from_pdb(pdb_path, ff)
    sigma = np.array([ff.sigma[t] for t in types], dtype=np.float64)
    eps = np.array([ff.epsilon[t] for t in types], dtype=np.float64)
    return g, NonbondedParameters.from_bonds(g["bonds"], g["charges"], sigma, eps, coulomb14scale=ff.coulomb14scale, lj14scale=ff.lj14scale)
