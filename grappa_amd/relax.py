"""Relaxation (energy minimisation) of molecules on the device under the full MM force field: the bonded terms Grappa predicts plus,
optionally, Lennard-Jones + Coulomb (`grappa_amd.nonbonded`).  The reference hands this step to OpenMM / GROMACS; here one launch of
csrc/relax.hip (`grappa_relax_fire_f32` through `HipBackend.relax_fire`) runs the whole minimisation of every (molecule, conformation):
one workgroup each, coordinates in LDS, no host round trip per step.  That fused kernel takes molecules of up to `relax_max_atoms()`
atoms.  Larger ones -- a protein -- go through the stepwise path (`stepwise=True` or `"auto"`; csrc/relax_steps.hip,
`grappa_relax_steps_*_f32` through `HipBackend.relax_steps`): the same loop with a molecule spread over many workgroups, the state in
device memory and four launches per step; the host syncs with the device once per chunk of `check_every` steps, never per step.

The minimiser is FIRE (Bitzek et al., Phys. Rev. Lett. 97, 170201 (2006)) with unit masses and semi-implicit Euler; the loop is stated
in include/grappa_hip.h.  Units: Angstrom, kcal/mol, kcal/mol/A.  An item stops with a status:
    0  max_steps reached        1  converged: the largest atomic gradient norm <= tolerance
    2  non-finite gradient (for example two non-excluded atoms on one point): stopped at once, the coordinates are those it held
    3  the molecule has more than `relax_max_atoms()` atoms: not run (the fused kernel only)
The defaults (`RELAX_DEFAULTS`; tolerance = 10 kJ/mol/nm, OpenMM's `minimizeEnergy` default) were checked on small chain molecules only
and are not tuned.  With `stepwise=False` (the default) a molecule above `relax_max_atoms()` atoms is refused; `stepwise="auto"` takes
the stepwise path for a batch that holds one.  The two paths add in different orders: the same trajectory within rounding, not the same bits.

Cutoff (`cutoff=`, a `grappa_amd.nonbonded.Cutoff` or a distance in Angstrom): the nonbonded term under OpenMM's `CutoffNonPeriodic`
conventions, as `grappa_amd.nonbonded` states them and `simulate(..., cutoff=)` moves under them, on the stepwise path
(`grappa_relax_steps_*_cut_f32`), whose force launch then skips the 64 x 64 atom tiles that lie beyond the cutoff; a step stays four
launches.  The minimiser then works on that energy: `RelaxResult.energy` (and the backend's `term_energy`) are the CUT terms, the
Hamiltonian a `simulate` with the same cutoff starts under.  It needs `nonbonded`; `stepwise="auto"` goes stepwise whenever a cutoff
is given, `stepwise=False` is refused.  The fused kernels, restraints (and so `torsion_scan`), periodic boxes, PME and a long-range
Lennard-Jones correction have no cutoff.

Implicit solvent (`implicit_solvent=`, `grappa_amd.solvent`): the minimisation under the GB/SA Hamiltonian that
`simulate(..., implicit_solvent=)` runs under, on the stepwise path (`grappa_relax_steps_*_gb_f32` through `HipBackend.relax_steps_gb`):
three more passes of the tiled pair loop behind the force launch, seven launches per step.  `RelaxResult.energy` then includes the
solvent term and `RelaxResult.esolv` holds it alone.  The rules are `simulate`'s: it needs `nonbonded` and the per-atom radii and
screening factors (`gb=`), `stepwise="auto"` goes stepwise whenever it is given, and `stepwise=False`, a cutoff and restraints are
refused.  All pairs only; the fused minimiser, restraints and `torsion_scan` have no solvent; no HCT / GBn model and no salt term.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .constants import TUPLE_LEVELS
from .energy import mm_tables
from .nonbonded import NonbondedBatch, NonbondedParameters, as_cutoff
from .parameters import Parameters

RELAX_DEFAULTS = {"tolerance": 10.0 / 4.184 / 10.0, "max_steps": 1000, "dt_start": 0.002, "dt_max": 0.02, "max_disp": 0.1, "n_min": 5,
                  "f_inc": 1.1, "f_dec": 0.5, "alpha_start": 0.1, "f_alpha": 0.99}
MAX_STEPS_CAP = 1000000
CHECK_EVERY_DEFAULT = 32          # steps the stepwise path enqueues between two host syncs.  Untuned: nobody has measured another value.


def relax_max_atoms() -> int:
    """atoms per molecule the fused minimiser takes at most"""
    from . import _lib
    return _lib.relax_max_atoms()


def relax_options(**opts) -> dict:
    """the ten options of a call: RELAX_DEFAULTS overridden by `opts`, checked (the library checks them again)"""
    unknown = sorted(set(opts) - set(RELAX_DEFAULTS))
    if unknown:
        raise TypeError(f"unknown relaxation option(s) {unknown}; the options are {sorted(RELAX_DEFAULTS)}")
    o = {**RELAX_DEFAULTS, **opts}
    for k in ("max_steps", "n_min"):
        if int(o[k]) != o[k] or o[k] < 0:
            raise ValueError(f"{k} must be a non-negative integer, got {o[k]}")
        o[k] = int(o[k])
    if o["max_steps"] > MAX_STEPS_CAP:
        raise ValueError(f"max_steps must not exceed {MAX_STEPS_CAP}, got {o['max_steps']}")
    for k in ("dt_start", "dt_max", "max_disp", "f_inc", "f_dec", "f_alpha"):
        if not (np.isfinite(o[k]) and o[k] > 0):
            raise ValueError(f"{k} must be positive and finite, got {o[k]}")
    if not (np.isfinite(o["tolerance"]) and o["tolerance"] >= 0):
        raise ValueError(f"tolerance must be non-negative and finite, got {o['tolerance']}")
    if not 0 <= o["alpha_start"] <= 1:
        raise ValueError(f"alpha_start must lie in [0, 1], got {o['alpha_start']}")
    return o


@dataclass
class RelaxResult:
    """xyz: the relaxed coordinates; energy: the total energy there (under a cutoff: the sum of the cut terms); gradient_max: the largest atomic gradient norm there; steps;
    status (see the module text).  From `relax_graph`: tensors on the graph's device, xyz (N, C, 3), the others (B, C).  From `relax`:
    numpy arrays of one molecule, xyz (n_confs, n_atoms, 3), the others (n_confs,)."""
    xyz: object
    energy: object
    gradient_max: object
    steps: object
    status: object
    restraint_energy: object = None          # with restraints: E_r at xyz (energy stays the force field's), else None
    dihedrals: object = None                 # with restraints: the restrained dihedrals at xyz, (R, C) / (R, n_confs) in radians, else None
    esolv: object = None                     # with an implicit solvent: its part of energy, shaped like it; else None

    @property
    def converged(self):
        return self.status == 1


def _stepwise_options(stepwise, check_every):
    if not (stepwise is True or stepwise is False or stepwise == "auto"):
        raise ValueError(f"stepwise must be False, True or 'auto', got {stepwise!r}")
    if isinstance(check_every, bool) or not isinstance(check_every, (int, np.integer)) or check_every < 1:
        raise ValueError(f"check_every must be an integer >= 1, got {check_every!r}")
    return stepwise, int(check_every)


def check_restraint_batch(restraints, B, C, counts, dev):
    """a `RestraintBatch` against the graph it is to restrain (B molecules of `counts` atoms in C conformations on `dev`): the checks
    `relax_graph` and `simulate_graph` share"""
    if restraints.B != B or restraints.C != C:
        raise ValueError(f"the restraint batch describes {restraints.B} molecules in {restraints.C} conformations, the graph {B} in {C}")
    if restraints.atom_counts is not None and list(restraints.atom_counts) != counts:
        raise ValueError("the restraint batch does not describe the graph's molecules (atoms per molecule differ)")
    for b, r in enumerate(restraints.items):
        if r is not None and r.n_dihedrals and int(r.dihedrals.max()) >= counts[b]:
            raise ValueError(f"molecule {b}: a restrained dihedral names atom {int(r.dihedrals.max())}, the molecule has {counts[b]} atoms")
    if restraints.dih_molptr.device != dev:
        raise ValueError(f"the restraint batch is on {restraints.dih_molptr.device}, the graph on {dev}")


def _cutoff_options(cutoff, nonbonded, stepwise, restraints):
    """the rules of a cutoff (those of `simulate`), decided on the host before anything is built -> a `Cutoff` or None"""
    cutoff = as_cutoff(cutoff)
    if cutoff is not None:
        if nonbonded is None:
            raise ValueError("relax: a cutoff needs the nonbonded parameters (nonbonded=)")
        if stepwise is False:
            raise ValueError('relax: a cutoff runs on the stepwise path only: pass stepwise="auto" (or True)')
        if restraints is not None:
            raise ValueError("relax: restraints are taken by the fused minimiser only, a cutoff on the stepwise path only")
    return cutoff


def _solvent_options(implicit_solvent, gb, nonbonded, stepwise, restraints, cutoff, gb_type):
    """the rules of an implicit solvent (those of `simulate`), decided on the host before anything is built -> an `ImplicitSolvent` or
    None; gb_type: what gb= has to be at this door"""
    from .solvent import as_implicit_solvent
    solvent = as_implicit_solvent(implicit_solvent)
    if solvent is None:
        if gb is not None:
            raise ValueError("relax: gb= needs implicit_solvent=")
        return None
    if solvent.cutoff is not None:
        raise ValueError("relax: the implicit solvent's cutoff (ImplicitSolvent(cutoff=)) serves the energy entry and the stepwise dynamics: the "
                         "minimiser does not run under it, and does not silently minimise on the all-pairs surface")
    if cutoff is not None:
        raise ValueError("relax: an implicit solvent under a cutoff is not implemented: pass one of the two")
    if nonbonded is None:
        raise ValueError("relax: an implicit solvent needs the nonbonded parameters (nonbonded=): they carry the charges")
    if stepwise is False:
        raise ValueError('relax: an implicit solvent runs on the stepwise path only: pass stepwise="auto" (or True)')
    if restraints is not None:
        raise ValueError("relax: restraints are taken by the fused minimiser only, an implicit solvent on the stepwise path only")
    if not isinstance(gb, gb_type):
        raise TypeError(f"relax: an implicit solvent needs gb=, the {gb_type.__name__} of the molecules, got {type(gb).__name__}")
    return solvent


def graph_coordinates(g, terms):
    """what the fused kernels read of a parametrised batched graph before anything is checked against it: -> xyz (N, C, 3) float32
    contiguous on the graph's device, the graph's plan and the atoms per molecule as host numbers (no device sync)"""
    for t in terms:
        if t not in TUPLE_LEVELS:
            raise ValueError(f"term {t} not in {TUPLE_LEVELS}")
    n1 = g.nodes["n1"].data
    if "xyz" not in n1:
        raise ValueError("xyz coordinates must be stored in g.nodes['n1'].data['xyz']")
    xyz = n1["xyz"].detach()
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError(f"xyz must be (N, C, 3), got {tuple(xyz.shape)}")
    return xyz.float().contiguous(), g.plan(), [int(c) for c in g.batch_num_nodes_host("n1")]


def graph_force_field(g, plan, counts, nonbonded, terms, suffix, dev):
    """checks that `nonbonded` (a NonbondedBatch or None) describes the graph's molecules on its device -> the MM tables ks, eqs, n_per"""
    if nonbonded is not None:
        if not isinstance(nonbonded, NonbondedBatch):
            raise TypeError(f"nonbonded must be a NonbondedBatch or None, got {type(nonbonded).__name__}")
        if nonbonded.N != plan.N or nonbonded.B != plan.B or nonbonded.atom_molptr_host.tolist() != np.concatenate([[0], np.cumsum(counts)]).tolist():
            raise ValueError(f"the nonbonded batch ({nonbonded.B} molecules, {nonbonded.N} atoms) does not describe the graph's molecules "
                             f"({plan.B} molecules, {plan.N} atoms)")
        if nonbonded.charge.device != dev:
            raise ValueError(f"the nonbonded batch is on {nonbonded.charge.device}, the graph on {dev}")
    ks, eqs, n_per = mm_tables(g, plan, list(terms), suffix, dev)
    return [k.detach().contiguous() for k in ks], [None if q is None else q.detach().contiguous() for q in eqs], n_per


def relax_graph(g, nonbonded: Optional[NonbondedBatch] = None, *, terms=("n2", "n3", "n4", "n4_improper"), suffix: str = "",
                offset_torsion: bool = False, stepwise=False, check_every: int = CHECK_EVERY_DEFAULT, restraints=None, cutoff=None,
                implicit_solvent=None, gb=None, **opts) -> RelaxResult:
    """Relax every (molecule, conformation) of a parametrised batched graph: `xyz` (N, C, 3) at n1 and `k` / `eq` at the tuple levels,
    exactly what `Energy` reads, through the same plan.  nonbonded: the batch's `NonbondedBatch` on the graph's device (None: bonded
    terms only).  **opts: see RELAX_DEFAULTS.  The graph is not modified.
    stepwise=False (the default): the fused kernel, one launch, no host sync; a molecule above `relax_max_atoms()` atoms is refused.
    stepwise=True: the whole batch through the stepwise path, which takes molecules of any size: four launches per step, and the host
    SYNCS with the device once per chunk of `check_every` steps (an integer >= 1; the default 32 is untuned) to see whether any item
    still runs.  stepwise="auto": the fused kernel if every molecule is within the limit, else the whole batch stepwise -- a batch is
    never split between the two paths (one batch, one decomposition, one set of bits).
    restraints: a `grappa_amd.restraints.RestraintBatch` for the graph's molecules and C on the graph's device (None: no restraints,
    the call as it always was).  The minimiser then works on E + E_r; `energy` stays the force field's, and the result carries
    `restraint_energy` (B, C) and `dihedrals` (R, C).  An item whose tables the kernel refuses comes back with status 5.  The fused
    path only: with restraints stepwise=True raises, and "auto" raises for a batch that holds a molecule above the limit.
    cutoff: a `grappa_amd.nonbonded.Cutoff` or a distance (None: all pairs, the calls made are exactly those without this argument):
    see the module text.  `energy` is then the sum of the cut terms.  It needs `nonbonded` and the stepwise path: "auto" then goes
    stepwise whatever the sizes, stepwise=False and restraints are refused.
    implicit_solvent: "obc2", "obc1" or a `grappa_amd.solvent.ImplicitSolvent` (None: vacuum, the calls made are exactly those without
    this argument) -- the GB/SA term of `grappa_amd.solvent` added to the minimised energy, with gb, the batch's
    `grappa_amd.solvent.GBBatch` on the graph's device.  `energy` then includes the solvent term and the result's `esolv` (B, C) holds
    it alone.  It needs `nonbonded` and the stepwise path: "auto" then goes stepwise whatever the sizes; stepwise=False, a cutoff and
    restraints are refused."""
    from .backend import get_backend
    from .solvent import GBBatch
    o = relax_options(**opts)
    stepwise, check_every = _stepwise_options(stepwise, check_every)
    cutoff = _cutoff_options(cutoff, nonbonded, stepwise, restraints)
    solvent = _solvent_options(implicit_solvent, gb, nonbonded, stepwise, restraints, cutoff, GBBatch)
    if solvent is not None and getattr(get_backend(), "relax_steps_gb", None) is None:
        raise ValueError("relax: the backend has no implicit solvent for the minimiser (relax_steps_gb)")
    terms = list(terms)
    if restraints is not None:
        from .restraints import RestraintBatch
        if not isinstance(restraints, RestraintBatch):
            raise TypeError(f"restraints must be a RestraintBatch or None, got {type(restraints).__name__}")
        if stepwise is True:
            raise ValueError("relax: restraints are taken by the fused minimiser only (stepwise=False or 'auto')")
    xyz, plan, counts = graph_coordinates(g, terms)
    dev = xyz.device
    limit = get_backend().relax_max_atoms()
    above = bool(counts) and max(counts) > limit
    if above and restraints is not None:
        raise ValueError(f"relax: a molecule of {max(counts)} atoms is above the limit of {limit} atoms per molecule of the fused "
                         f"minimiser, and restraints are not available on the stepwise path")
    if above and stepwise is False:
        raise ValueError(f"relax: a molecule of {max(counts)} atoms is above the limit of {limit} atoms per molecule of the fused "
                         f"minimiser (stepwise=True or stepwise='auto' relaxes molecules of any size)")
    use_steps = stepwise is True or (stepwise == "auto" and (above or cutoff is not None or solvent is not None))
    B, C = plan.B, xyz.shape[1]
    if solvent is not None:
        if gb.counts != list(counts):
            raise ValueError(f"the GB parameters describe molecules of {gb.counts} atoms, the batch has {list(counts)}")
        if gb.radius.device != dev:
            raise ValueError(f"the GB parameters are on {gb.radius.device}, the graph on {dev}")
        gb.check_offset(solvent.offset)          # (the batch may have been checked against another offset than the solvent's)
    if restraints is not None:
        check_restraint_batch(restraints, B, C, counts, dev)
    ks, eqs, n_per = graph_force_field(g, plan, counts, nonbonded, terms, suffix, dev)
    out = torch.empty_like(xyz)
    energy, gmax = torch.zeros(B, C, dtype=torch.float32, device=dev), torch.zeros(B, C, dtype=torch.float32, device=dev)
    steps, status = torch.zeros(B, C, dtype=torch.int32, device=dev), torch.zeros(B, C, dtype=torch.int32, device=dev)
    er, phi, restr = None, None, {}          # (without restraints the backend is called exactly as it always was)
    if restraints is not None:
        er, phi = torch.zeros(B, C, dtype=torch.float32, device=dev), torch.zeros(restraints.R, C, dtype=torch.float32, device=dev)
        restr = dict(restraints=restraints, restraint_energy=er, dihedral_out=phi)
    if solvent is not None:
        es = torch.zeros(B, C, dtype=torch.float32, device=dev)
        get_backend().relax_steps_gb(plan, xyz, ks, eqs, n_per, bool(offset_torsion), nonbonded, o, out, energy, gmax, steps, status,
                                     atom_counts_host=counts, check_every=check_every, gb=gb, solvent=solvent, esolv=es)
        return RelaxResult(out, energy, gmax, steps, status, er, phi, es)
    if use_steps:
        get_backend().relax_steps(plan, xyz, ks, eqs, n_per, bool(offset_torsion), nonbonded, o, out, energy, gmax, steps, status,
                                  atom_counts_host=counts, check_every=check_every, **({} if cutoff is None else {"cutoff": cutoff}))
    else:
        get_backend().relax_fire(plan, xyz, ks, eqs, n_per, bool(offset_torsion), nonbonded, o, out, energy, gmax, steps, status,
                                 atom_counts_host=counts, **restr)
    return RelaxResult(out, energy, gmax, steps, status, er, phi)


def graph_from_parameters(parameters: Parameters, xyz):
    """one molecule's `Parameters` (atom-id space, torsions as magnitude and phase) and its conformations (n_confs, n_atoms, 3) -> the
    parametrised single-molecule graph `relax_graph` and `Energy` read: atom ids mapped to indices, signed torsion constants rebuilt
    (phase pi = a negative constant)"""
    from .batch import single_graph
    atoms = np.asarray(parameters.atoms).reshape(-1)
    n = atoms.shape[0]
    if np.unique(atoms).shape[0] != n:
        raise ValueError("Parameters.atoms holds an atom id twice")
    x = np.asarray(xyz)
    if x.ndim != 3 or x.shape[1:] != (n, 3):
        raise ValueError(f"xyz must be (n_confs, {n}, 3), got {x.shape}")
    order = np.argsort(atoms, kind="stable")

    def index_of(ids, arity, name):
        ids = np.asarray(ids if ids is not None else np.zeros((0, arity)), dtype=np.int64).reshape(-1, arity)
        pos = np.searchsorted(atoms[order], ids)
        if ids.size and (pos.max() >= n or not np.array_equal(atoms[order][np.minimum(pos, n - 1)], ids)):
            raise ValueError(f"Parameters.{name} names an atom id that is not in Parameters.atoms")
        return order[pos].reshape(-1, arity)

    idxs = {"n2": index_of(parameters.bonds, 2, "bonds"), "n3": index_of(parameters.angles, 3, "angles"),
            "n4": index_of(parameters.propers, 4, "propers"), "n4_improper": index_of(parameters.impropers, 4, "impropers")}
    f32 = lambda a, shape: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(shape)))      # noqa: E731

    def signed(ks, phases, T, name):
        if ks is None or phases is None:
            ks, phases = np.zeros((T, 1)), np.zeros((T, 1))
        ks, phases = np.asarray(ks, dtype=np.float64), np.asarray(phases, dtype=np.float64)
        if ks.shape != phases.shape or ks.shape[0] != T:
            raise ValueError(f"Parameters.{name}_ks {ks.shape} and {name}_phases {phases.shape} must share a shape with {T} rows")
        ks = ks.reshape(T, -1) if T else ks.reshape(0, max(ks.shape[-1] if ks.ndim == 2 else 1, 1))
        return f32(np.where(np.cos(phases.reshape(ks.shape)) >= 0, ks, -ks), ks.shape)

    for (lvl, name) in (("n2", "bond"), ("n3", "angle")):
        T = idxs[lvl].shape[0]
        for key in ("k", "eq"):
            if np.asarray(getattr(parameters, f"{name}_{key}")).reshape(-1).shape[0] != T:
                raise ValueError(f"Parameters.{name}_{key} must hold {T} values")
    g = single_graph(n, idxs["n2"], idxs, {"xyz": f32(x.transpose(1, 0, 2), (n, x.shape[0], 3))}, ids=atoms)
    for lvl, name in (("n2", "bond"), ("n3", "angle")):
        T = idxs[lvl].shape[0]
        g.nodes[lvl].data["k"] = f32(getattr(parameters, name + "_k"), (T,))
        g.nodes[lvl].data["eq"] = f32(getattr(parameters, name + "_eq"), (T,))
    for lvl, name in (("n4", "proper"), ("n4_improper", "improper")):
        g.nodes[lvl].data["k"] = signed(getattr(parameters, name + "_ks"), getattr(parameters, name + "_phases"), idxs[lvl].shape[0], name)
    return g


def relax(parameters: Parameters, xyz, nonbonded: Optional[NonbondedParameters] = None, device="cuda", *, stepwise=False,
          check_every: int = CHECK_EVERY_DEFAULT, restraints=None, cutoff=None, implicit_solvent=None, gb=None, **opts) -> RelaxResult:
    """Relax the conformations of ONE molecule under the parameters `Grappa.predict` returned (+ `nonbonded`, whose atoms are in the
    order of `parameters.atoms`), numpy in and out: xyz (n_confs, n_atoms, 3) in Angstrom -> RelaxResult with xyz of the same shape
    (float64) and energy / gradient_max / steps / status of shape (n_confs,).  stepwise, check_every: see `relax_graph` (the stepwise
    path takes a molecule of any size and syncs with the host once per chunk of `check_every` steps).
    restraints: a `grappa_amd.restraints.Restraints` whose indices are in the order of `parameters.atoms` (None: none); the result
    then carries restraint_energy (n_confs,) and dihedrals (R, n_confs), and `energy` stays the force field's.  The fused path only.
    cutoff: see `relax_graph` (`energy` is then the sum of the cut terms; the stepwise path only, no restraints).
    implicit_solvent: see `relax_graph`; gb: the molecule's `grappa_amd.solvent.GBParameters` in the order of `parameters.atoms`.  The
    result then carries esolv (n_confs,), and `energy` includes it."""
    from .solvent import GBBatch, GBParameters
    relax_options(**opts)
    _stepwise_options(stepwise, check_every)
    extra = {}
    if _cutoff_options(cutoff, nonbonded, stepwise, restraints) is not None:
        extra["cutoff"] = as_cutoff(cutoff)
    solvent = _solvent_options(implicit_solvent, gb, nonbonded, stepwise, restraints, extra.get("cutoff"), GBParameters)
    if solvent is not None:
        if gb.n_atoms != np.asarray(parameters.atoms).reshape(-1).shape[0]:
            raise ValueError(f"the GB parameters describe {gb.n_atoms} atoms, the molecule has {np.asarray(parameters.atoms).reshape(-1).shape[0]}")
        extra.update(implicit_solvent=solvent, gb=GBBatch([gb], solvent.offset).to(device))
    g = graph_from_parameters(parameters, xyz)
    batch = None
    if restraints is not None:
        from .restraints import RestraintBatch, Restraints
        if not isinstance(restraints, Restraints):
            raise TypeError(f"restraints must be Restraints or None, got {type(restraints).__name__}")
        if stepwise is True:
            raise ValueError("relax: restraints are taken by the fused minimiser only (stepwise=False or 'auto')")
        batch = RestraintBatch([restraints], int(np.asarray(xyz).shape[0]), atom_counts=[g.num_nodes("n1")])
    nb = None
    if nonbonded is not None:
        if not isinstance(nonbonded, NonbondedParameters):
            raise TypeError(f"nonbonded must be NonbondedParameters or None, got {type(nonbonded).__name__}")
        if nonbonded.n_atoms != g.num_nodes("n1"):
            raise ValueError(f"the nonbonded parameters describe {nonbonded.n_atoms} atoms, the molecule has {g.num_nodes('n1')}")
        nb = NonbondedBatch([nonbonded]).to(device)
    r = relax_graph(g.to(device), nb, stepwise=stepwise, check_every=check_every, restraints=None if batch is None else batch.to(device), **extra,
                    **opts)
    res = RelaxResult(r.xyz.cpu().numpy().transpose(1, 0, 2).astype(np.float64), r.energy.cpu().numpy()[0].astype(np.float64),
                      r.gradient_max.cpu().numpy()[0].astype(np.float64), r.steps.cpu().numpy()[0], r.status.cpu().numpy()[0])
    if batch is not None:
        res.restraint_energy, res.dihedrals = r.restraint_energy.cpu().numpy()[0].astype(np.float64), r.dihedrals.cpu().numpy().astype(np.float64)
    if r.esolv is not None:
        res.esolv = r.esolv.cpu().numpy()[0].astype(np.float64)
    return res


SCAN_K_DEFAULT = 239.0          # kcal/mol: 1000 kJ/mol, the usual stiffness of a torsion restraint.  A default, not a tuned value.


@dataclass
class ScanResult:
    """angles (P,): the targets; dihedrals (P,): the dihedral achieved at each; energy (P,): the FORCE FIELD's energy there (what a scan
    plots); restraint_energy (P,); xyz (P, n_atoms, 3); steps, status (P,) as for `relax`.  numpy, radians, kcal/mol, Angstrom."""
    angles: object
    dihedrals: object
    energy: object
    restraint_energy: object
    xyz: object
    steps: object
    status: object


def scan_starts(parameters: Parameters, xyz, dihedral, angles):
    """-> (the start coordinates of a torsion scan, (P, n_atoms, 3) float64; the dihedral as four atom indices): for each angle the
    input with the l-side of the j-k bond rotated rigidly about that bond so that the dihedral equals the angle
    (`grappa_amd.restraints.set_dihedral`, on the bond graph of `parameters.bonds`); if j-k lies in a ring nothing is rotated and every
    point starts from the input"""
    from .restraints import set_dihedral
    atoms = np.asarray(parameters.atoms).reshape(-1)
    pos = {int(a): k for k, a in enumerate(atoms.tolist())}
    x = np.asarray(xyz, dtype=np.float64)
    if x.shape != (atoms.shape[0], 3):
        raise ValueError(f"xyz must be one conformation ({atoms.shape[0]}, 3), got {x.shape}")
    ids = [int(a) for a in np.asarray(dihedral).reshape(-1)]
    if len(ids) != 4 or any(a not in pos for a in ids) or len(set(ids)) != 4:
        raise ValueError(f"dihedral must name four distinct atom ids of parameters.atoms, got {ids}")
    idx = [pos[a] for a in ids]
    bonds = np.array([[pos[int(a)], pos[int(b)]] for a, b in np.asarray(parameters.bonds).reshape(-1, 2).tolist()], dtype=np.int64).reshape(-1, 2)
    return np.stack([set_dihedral(x, bonds, idx, float(a)) for a in angles]), idx


def torsion_scan(parameters: Parameters, xyz, dihedral, angles=None, nonbonded: Optional[NonbondedParameters] = None, k: float = SCAN_K_DEFAULT,
                 device="cuda", **opts) -> ScanResult:
    """A relaxed torsion scan of ONE molecule: the dihedral (four atom ids of `parameters.atoms`) is held near each of `angles`
    (radians; default 24 points from -pi in steps of 15 degrees) by the restraint k (1 - cos(phi - angle)), k in kcal/mol, and everything
    else is relaxed.  xyz: one conformation (n_atoms, 3).  The grid points are the conformations of ONE restrained `relax` call: one
    launch, one workgroup per point.  The points are INDEPENDENT: each starts from the input with one side of the bond rotated to its
    angle (`scan_starts`), nothing is propagated from a neighbouring point -- so a point can end in another basin than its neighbours.
    **opts: the options of `relax` (RELAX_DEFAULTS).  With the default k FIRE's defaults are stable (the restraint is softer than
    every bond); whether a point reached the tolerance is in `status`.  It takes no cutoff and no implicit solvent: restraints are the
    fused minimiser's."""
    from .restraints import Restraints
    if "cutoff" in opts:
        raise ValueError("torsion_scan: takes no cutoff (restraints are taken by the fused minimiser only, a cutoff runs on the stepwise path only)")
    if "implicit_solvent" in opts or "gb" in opts:
        raise ValueError("torsion_scan: takes no implicit solvent (restraints are taken by the fused minimiser only, a solvent runs on the "
                         "stepwise path only)")
    if angles is None:
        angles = -np.pi + np.deg2rad(15.0) * np.arange(24)
    angles = np.asarray(angles, dtype=np.float64).reshape(-1)
    if not np.isfinite(angles).all():
        raise ValueError("angles must be finite")
    if not (np.isfinite(k) and k >= 0):
        raise ValueError(f"k must be finite and non-negative, got {k}")
    starts, idx = scan_starts(parameters, xyz, dihedral, angles)
    P = angles.shape[0]
    if P == 0:
        z = np.zeros(0)
        return ScanResult(angles, z, z, z, starts.reshape(0, np.asarray(xyz).shape[0], 3), np.zeros(0, np.int32), np.zeros(0, np.int32))
    r = relax(parameters, starts, nonbonded, device=device,
              restraints=Restraints(dihedrals=[idx], dihedral_k=[float(k)], dihedral_targets=angles[None, :]), **opts)
    return ScanResult(angles, r.dihedrals[0], r.energy, r.restraint_energy, r.xyz, r.steps, r.status)
