"""GB/SA implicit solvent on the device: the generalized-Born model of Onufriev, Bashford and Case with a surface-area term (OpenMM's
`GBSAOBCForce`), for a solute alone -- no box, no neighbour list.  In this project's units (Angstrom, kcal/mol, elementary charges),
with the charge q_i of the nonbonded parameters, a radius R_i and a scale S_i per atom, o_i = R_i - offset, s_j = S_j o_j:

    I_i   = sum_{j != i} H(r_ij, o_i, s_j)                      (H: include/grappa_hip.h grappa_gb_desc; every pair, bonded or not)
    B_i   = 1 / (1/o_i - tanh(alpha psi - beta psi^2 + gamma psi^3) / R_i),  psi = o_i I_i / 2                      (the Born radius)
    E_pol = -(K/2) (1/solute_dielectric - 1/solvent_dielectric) sum_{i,j, i = j included} q_i q_j / sqrt(r^2 + B_i B_j exp(-r^2/(4 B_i B_j)))
    E_sa  = sum_i 4 pi surface_tension (R_i + probe)^2 (R_i / B_i)^6

"obc2" is (alpha, beta, gamma) = (1, 0.8, 4.85), "obc1" is (0.8, 0, 2.909125).  The gradient is the exact +dE/dxyz (not the force).
The arithmetic runs in csrc/gb_obc.hip through `HipBackend.gb_obc`; there is no CPU evaluator.

`ImplicitSolvent(cutoff=rc)` truncates the model pairwise, as OpenMM's `GBSAOBCForce` does under `CutoffNonPeriodic`: an ordered pair
i != j counts in I_i, in E_pol and in the chain rule only if r_ij < rc; the terms i = j and E_sa are not cut; nothing is shifted or
switched, so the energy jumps by the pair's terms where a pair crosses rc, and Born radii under a short cutoff differ from the all-pairs
ones.  Far 64 x 64 tiles are skipped (prune=True; the same bits as prune=False).  The cutoff serves the energy (`GBBatch.evaluate`,
`solvent_energy`) and the stepwise dynamics (`simulate(..., implicit_solvent=ImplicitSolvent(cutoff=))`); the minimiser refuses a
solvent that carries one.  Out of scope: the HCT and GBn models, a salt term, a smoothed truncation, a separate cutoff for the Born
integral.
"""
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

MODELS = {"obc2": (1.0, 0.8, 4.85), "obc1": (0.8, 0.0, 2.909125)}

# the published mbondi2 radii (A) and OBC screening factors by atomic number; H bonded to N: 1.3
_RADIUS = {1: 1.2, 6: 1.7, 7: 1.55, 8: 1.5, 9: 1.5, 14: 2.1, 15: 1.85, 16: 1.8, 17: 1.7}
_RADIUS_OTHER, _RADIUS_H_ON_N = 1.5, 1.3
_SCALE = {1: 0.85, 6: 0.72, 7: 0.79, 8: 0.85, 9: 0.88, 15: 0.86, 16: 0.96}
_SCALE_OTHER = 0.8


def _num(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)


@dataclass(frozen=True)
class ImplicitSolvent:
    """the options of the GB/SA model (grappa_gb_desc): model "obc2" or "obc1"; the dielectrics finite and > 0; surface_tension
    (kcal/mol/A^2; 0.0054 is OpenMM's 2.25936 kJ/mol/nm^2) and probe (A) finite and >= 0; offset (A) finite and >= 0; cutoff (A): None
    (all pairs) or finite and > 0 with a square float32 holds (grappa_gb_cut); prune: skip far tiles (the same bits either way)"""
    model: str = "obc2"
    solute_dielectric: float = 1.0
    solvent_dielectric: float = 78.5
    surface_tension: float = 0.0054
    probe: float = 1.4
    offset: float = 0.09
    cutoff: Optional[float] = None
    prune: bool = True

    def __post_init__(self):
        if self.model not in MODELS:
            raise ValueError(f"implicit solvent: model must be one of {sorted(MODELS)}, got {self.model!r}")
        for k in ("solute_dielectric", "solvent_dielectric"):
            if not _num(getattr(self, k)) or not getattr(self, k) > 0:
                raise ValueError(f"implicit solvent: {k} must be a finite number > 0, got {getattr(self, k)!r}")
        for k in ("surface_tension", "probe", "offset"):
            if not _num(getattr(self, k)) or getattr(self, k) < 0:
                raise ValueError(f"implicit solvent: {k} must be a finite number >= 0, got {getattr(self, k)!r}")
        if self.cutoff is not None:
            ok = _num(self.cutoff) and self.cutoff > 0 and float(self.cutoff) * float(self.cutoff) <= float(np.finfo(np.float32).max)
            if not ok:
                raise ValueError(f"implicit solvent: cutoff must be None or a finite number > 0 whose square float32 holds, got {self.cutoff!r}")
        if not isinstance(self.prune, (bool, np.bool_)):
            raise ValueError(f"implicit solvent: prune must be True or False, got {self.prune!r}")

    def as_opts(self) -> dict:
        """the eight options of grappa_gb_desc by name"""
        a, b, g = MODELS[self.model]
        return {"offset": float(self.offset), "alpha": a, "beta": b, "gamma": g, "eps_in": float(self.solute_dielectric),
                "eps_out": float(self.solvent_dielectric), "surface_tension": float(self.surface_tension), "probe": float(self.probe)}

    def cut_opts(self) -> Optional[dict]:
        """None without a cutoff, else the two options of grappa_gb_cut by name"""
        if self.cutoff is None:
            return None
        return {"cutoff": float(self.cutoff), "prune": int(bool(self.prune))}


def as_implicit_solvent(solvent: Union[None, str, "ImplicitSolvent"]) -> Optional["ImplicitSolvent"]:
    """None, an `ImplicitSolvent`, or a model name (-> ImplicitSolvent(model)), checked"""
    if solvent is None or isinstance(solvent, ImplicitSolvent):
        return solvent
    if isinstance(solvent, str):
        return ImplicitSolvent(solvent)
    raise ValueError(f"implicit solvent: expected None, a model name or an ImplicitSolvent, got {type(solvent).__name__}")


@dataclass
class GBParameters:
    """per-atom GB radius (A) and screening scale of one molecule, as OpenMM's GBSAOBCForce holds them (the charges are the
    NonbondedParameters')"""
    radius: np.ndarray
    scale: np.ndarray

    def __post_init__(self):
        self.radius, self.scale = np.asarray(self.radius, dtype=np.float64), np.asarray(self.scale, dtype=np.float64)

    @property
    def n_atoms(self) -> int:
        return int(self.radius.shape[0])

    def validate(self, offset: float = 0.09) -> "GBParameters":
        """shapes; every radius finite and above the offset as float32 holds it (o_i = R_i - offset > 0); every scale finite and > 0"""
        if self.radius.ndim != 1 or self.scale.shape != self.radius.shape:
            raise ValueError(f"radius and scale must share the shape (n,), got {self.radius.shape}, {self.scale.shape}")
        r32, s32 = self.radius.astype(np.float32), self.scale.astype(np.float32)
        if not np.isfinite(r32).all() or not (r32 - np.float32(offset) > 0).all():
            raise ValueError(f"radius: every radius must be finite and above the offset of {offset} A")
        if not np.isfinite(s32).all() or not (s32 > 0).all():
            raise ValueError("scale: every scale must be finite and > 0")
        return self

    def to_dict(self) -> Dict[str, np.ndarray]:
        return {"gbparam_radius": self.radius, "gbparam_scale": self.scale}

    @classmethod
    def from_dict(cls, d) -> "GBParameters":
        return cls(np.asarray(d["gbparam_radius"]), np.asarray(d["gbparam_scale"]))

    @classmethod
    def from_elements(cls, atomic_numbers, bonds) -> "GBParameters":
        """the published mbondi2 radii (H 1.2, H bonded to N 1.3, C 1.7, N 1.55, O 1.5, F 1.5, Si 2.1, P 1.85, S 1.8, Cl 1.7, anything
        else 1.5 A) and OBC screening factors (H 0.85, C 0.72, N 0.79, O 0.85, F 0.88, P 0.86, S 0.96, anything else 0.8).
        bonds: (m, 2) atom indices."""
        z = np.asarray(atomic_numbers, dtype=np.int64).reshape(-1)
        n = z.shape[0]
        b = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
        if b.size and (b.min() < 0 or b.max() >= n):
            raise ValueError(f"bonds: atom index outside [0, {n})")
        radius = np.array([_RADIUS.get(int(v), _RADIUS_OTHER) for v in z], dtype=np.float64)
        scale = np.array([_SCALE.get(int(v), _SCALE_OTHER) for v in z], dtype=np.float64)
        for h, x in ((b[:, 0], b[:, 1]), (b[:, 1], b[:, 0])):
            on_n = (z[h] == 1) & (z[x] == 7)
            radius[h[on_n]] = _RADIUS_H_ON_N
        return cls(radius, scale).validate()


class GBBatch:
    """the kernel's view of a list of molecules: the concatenated radius and scale tables.  `.to(device)` uploads them once."""
    _TENSORS = ("radius", "scale")

    def __init__(self, params: Sequence[GBParameters], offset: float = 0.09):
        params = [p.validate(offset) for p in params]
        self.B, self.N = len(params), int(sum(p.n_atoms for p in params))
        self.counts = [p.n_atoms for p in params]
        self.offset = float(offset)          # what the radii were checked against
        cat = lambda xs: np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1) for x in xs]) if xs else np.zeros(0, np.float32)      # noqa: E731
        self.radius = torch.from_numpy(np.ascontiguousarray(cat([p.radius for p in params])))
        self.scale = torch.from_numpy(np.ascontiguousarray(cat([p.scale for p in params])))
        self._radius_host = self.radius.numpy().copy()          # stays on the host, wherever `.to` puts the tables

    def check_offset(self, offset: float) -> "GBBatch":
        """the radii against another offset than the batch was built with (an `ImplicitSolvent` may carry its own): every radius must
        lie above it as float32 holds it, or o_i = R_i - offset is not positive.  Reads the host copy of the radii: no device sync."""
        if float(offset) != self.offset and not (self._radius_host - np.float32(offset) > 0).all():
            raise ValueError(f"radius: every radius must lie above the offset of {offset} A (the batch was checked against {self.offset} A)")
        return self

    def to(self, device) -> "GBBatch":
        for k in self._TENSORS:
            setattr(self, k, getattr(self, k).to(device))
        return self

    def evaluate(self, nb, xyz: torch.Tensor, solvent="obc2", terms: bool = False, gradient: bool = True, born_radii: bool = False,
                 tiles: bool = False):
        """nb: the `NonbondedBatch` of the same molecules on the same device (its charges, atom_molptr and cache of plans); xyz (N, C, 3)
        float32 there -> dict of energy (B, C), grad (N, C, 3) or None, terms (2, B, C: polar, surface area) or None, born (N, C) or
        None, tiles (n_items,) int32 or None.  A solvent with a cutoff runs grappa_gb_obc_fwd_cut_f32; tiles=True (which needs one)
        returns the 64 x 64 tiles each work item of the plan evaluated."""
        from .backend import get_backend
        solvent = as_implicit_solvent(solvent)
        if solvent is None:
            raise ValueError("GBBatch.evaluate: an implicit solvent model is required")
        if not isinstance(xyz, torch.Tensor) or xyz.dim() != 3 or xyz.shape[2] != 3 or xyz.dtype != torch.float32:
            raise ValueError(f"xyz must be a float32 (N, C, 3) tensor, got {getattr(xyz, 'dtype', type(xyz))} {tuple(getattr(xyz, 'shape', ()))}")
        if nb.N != self.N or nb.B != self.B or [int(v) for v in np.diff(nb.atom_molptr_host.numpy())] != self.counts:
            raise ValueError(f"the nonbonded batch describes {nb.B} molecules / {nb.N} atoms, the GB batch {self.B} / {self.N}")
        if xyz.shape[0] != self.N or xyz.device != self.radius.device or nb.charge.device != xyz.device:
            raise ValueError(f"xyz has {xyz.shape[0]} atoms on {xyz.device}, the batch {self.N} on {self.radius.device} (charges on {nb.charge.device})")
        xyz = xyz.contiguous()
        C = xyz.shape[1]
        self.check_offset(solvent.offset)
        be = get_backend()
        plan = nb.plan_for(C, xyz.device)
        energy = torch.zeros(self.B, C, dtype=torch.float32, device=xyz.device)
        grad = torch.zeros_like(xyz) if gradient else None
        te = torch.zeros(2, self.B, C, dtype=torch.float32, device=xyz.device) if terms else None
        born = torch.zeros(self.N, C, dtype=torch.float32, device=xyz.device) if born_radii else None
        cut = solvent.cut_opts()
        if cut is None:
            if tiles:
                raise ValueError("GBBatch.evaluate: tiles needs a solvent with a cutoff")
            be.gb_obc(xyz, nb.atom_molptr, nb.charge, self.radius, self.scale, solvent.as_opts(), energy, te, grad, born, plan=plan)
            return {"energy": energy, "grad": grad, "terms": te, "born": born, "tiles": None}
        nt = torch.zeros(int(plan[1]) if plan[0] is not None else 0, dtype=torch.int32, device=xyz.device) if tiles else None
        be.gb_obc(xyz, nb.atom_molptr, nb.charge, self.radius, self.scale, solvent.as_opts(), energy, te, grad, born, plan=plan, cut=cut,
                  tiles=nt)
        return {"energy": energy, "grad": grad, "terms": te, "born": born, "tiles": nt}


def solvent_energy(nonbonded_params, gb_params, xyz, device="cuda", model="obc2", terms: bool = False, born_radii: bool = False,
                   tiles: bool = False):
    """Solvation energies and gradients of one molecule or a list of molecules, numpy in and out.  nonbonded_params: the
    `NonbondedParameters` (they carry the charges); gb_params: the `GBParameters`; xyz: (n_confs, n_atoms, 3) in Angstrom, or a list
    of such arrays sharing n_confs; model: "obc2", "obc1" or an `ImplicitSolvent`.
    -> (energy (n_confs,), gradient (n_confs, n_atoms, 3)) in kcal/mol and kcal/mol/A, with terms=True followed by the polar and the
    surface-area part of the energy, with born_radii=True by the Born radii (n_confs, n_atoms) in A; for a list, a list of such tuples.
    An `ImplicitSolvent` with a cutoff is evaluated under it; tiles=True (which needs one) then returns (that result, tiles): the second
    the int array of 64 x 64 tiles each work item of the batch evaluated."""
    from .nonbonded import NonbondedBatch, NonbondedParameters
    solvent = as_implicit_solvent(model)
    if solvent is None:
        raise ValueError("solvent_energy: model must name an implicit solvent")
    single = isinstance(nonbonded_params, NonbondedParameters)
    plist: List[NonbondedParameters] = [nonbonded_params] if single else list(nonbonded_params)
    glist: List[GBParameters] = [gb_params] if isinstance(gb_params, GBParameters) else list(gb_params)
    xs = [np.asarray(xyz)] if single else [np.asarray(x) for x in xyz]
    if len(xs) != len(plist) or len(glist) != len(plist):
        raise ValueError(f"{len(plist)} nonbonded parameter sets, {len(glist)} GB parameter sets and {len(xs)} coordinate arrays")
    for p, g, x in zip(plist, glist, xs):
        if g.n_atoms != p.n_atoms:
            raise ValueError(f"GB parameters of {g.n_atoms} atoms for a molecule of {p.n_atoms}")
        if x.ndim != 3 or x.shape[1:] != (p.n_atoms, 3) or x.shape[0] != xs[0].shape[0]:
            raise ValueError(f"xyz must be (n_confs, {p.n_atoms}, 3) with one n_confs for all molecules, got {x.shape}")
    gb = GBBatch(glist, solvent.offset).to(device)
    nb = NonbondedBatch(plist).to(device)
    flat = np.concatenate([x.transpose(1, 0, 2) for x in xs], axis=0).astype(np.float32)
    out = gb.evaluate(nb, torch.from_numpy(np.ascontiguousarray(flat)).to(device), solvent, terms=terms, born_radii=born_radii, tiles=tiles)
    energy, grad = out["energy"].cpu().numpy(), out["grad"].cpu().numpy()
    te = out["terms"].cpu().numpy() if terms else None
    born = out["born"].cpu().numpy() if born_radii else None
    ptr = nb.atom_molptr_host.numpy()
    res = []
    for b in range(len(plist)):
        r = (energy[b].astype(np.float64), grad[ptr[b]:ptr[b + 1]].transpose(1, 0, 2).astype(np.float64))
        if terms:
            r = r + (te[0, b].astype(np.float64), te[1, b].astype(np.float64))
        if born_radii:
            r = r + (born[ptr[b]:ptr[b + 1]].T.astype(np.float64),)
        res.append(r)
    res = res[0] if single else res
    return (res, out["tiles"].cpu().numpy()) if tiles else res
