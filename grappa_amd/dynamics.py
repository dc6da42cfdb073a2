"""Langevin molecular dynamics of molecules on the device under the full MM force field: the bonded terms Grappa predicts plus,
optionally, Lennard-Jones + Coulomb (`grappa_amd.nonbonded`), in vacuum with all pairs (or, stepwise, in implicit solvent).  Two paths run
the same loop:
  fused     one launch of csrc/dynamics.hip (`grappa_md_langevin_f32` through `HipBackend.md_langevin`) runs many steps of every
            (molecule, conformation): one workgroup each, coordinates in LDS, velocities in registers, no host round trip per step.
            Molecules of up to `relax_max_atoms()` atoms.  `stepwise=False` (the default) takes it and refuses a larger molecule.
  stepwise  csrc/dynamics_steps.hip (`grappa_md_steps_*_f32` through `HipBackend.md_steps`): a molecule of ANY size -- a protein --
            spread over many workgroups, the state in device memory, two launches per step, all of them only enqueued: the host never
            waits for the device.  `stepwise=True` takes it for the whole batch, `stepwise="auto"` for a batch that holds a molecule
            above the limit (a batch is never split between the two paths).
The two paths add in different orders: the same trajectory within rounding, not the same bits.  Which of them is faster for a batch
that both take has not been decided here (tools/md_steps_bench.py measures it).

Cutoff (`cutoff=`, a `grappa_amd.nonbonded.Cutoff` or a distance in Angstrom): the nonbonded term under OpenMM's `CutoffNonPeriodic`
conventions -- reaction field, optional switch, exceptions uncut (`grappa_amd.nonbonded` states them) -- on the stepwise path only,
whose force launch then skips the 64 x 64 atom tiles that lie beyond the cutoff; a step stays two launches (four with constraints).  It needs `nonbonded`;
`stepwise="auto"` goes stepwise whenever a cutoff is given.  The stepwise minimiser, the fused kernels, periodic boxes, PME and a
long-range Lennard-Jones correction are out of scope (OpenMM / GROMACS).

Constraints (`constraints=`, `grappa_amd.constraints`): X-H bonds held at fixed lengths, on either path.  The loop is then
g-BAOAB (Leimkuhler and Matthews, Proc. R. Soc. A 472, 20160138 (2016)) with one geodesic sub-step: positions by a cluster-wise Newton
iteration (M-SHAKE) of at most eight updates, velocities by a direct projection (csrc/md_cons.h, one copy for both paths).  Fused:
csrc/dynamics_cons.hip (`grappa_md_langevin_cons_f32`), at most 256 clusters in a molecule.  Stepwise: `grappa_md_steps_*_cons_f32`
through `HipBackend.md_steps_cons`, molecules of any size with any number of clusters, with or without a cutoff; a cluster is
integrated by the workgroup that holds its centre, and a step is three launches, four under a cutoff -- what a 2 fs step for a protein
needs.  An atom draws the same noise with and without constraints, on either path.  Rigid water is out of scope.

Implicit solvent (`implicit_solvent=`, `grappa_amd.solvent`): the GB/SA term of Onufriev, Bashford and Case added to the potential, on
the stepwise path only (`grappa_md_steps_*_gb_f32` through `HipBackend.md_steps_gb`): three more passes of the tiled pair loop behind
the force launch, a step of five launches, six with constraints.  It needs `nonbonded` (the charges) and the per-atom radii and scales
(`gb=`), goes with constraints and not with a cutoff; `stepwise="auto"` goes stepwise whenever it is given.
A solvent with a cutoff of its own, `implicit_solvent=ImplicitSolvent("obc2", cutoff=12.0)`, runs under the pairwise truncation of
`grappa_amd.solvent` (`grappa_md_steps_*_gbcut_f32`): far tiles are skipped in all three passes, and a step gains no launch (with
constraints the box launch that a nonbonded cutoff adds as well).  Beside such a solvent -- and only beside it -- `cutoff=` is taken too:
the nonbonded cutoff of the paragraph above, on one set of boxes.  A reaction field already screens the Coulomb term; OpenMM runs GB
with the reaction-field dielectric 1, so `cutoff=Cutoff(rc, rs, rf_dielectric=1.0)` is the usual companion (what the caller passes is
not overridden).  The truncated solvent energy jumps where a pair crosses the cutoff: such a run does not conserve energy.

Restraints (`restraints=`, `grappa_amd.restraints`): harmonic tethers to a reference structure and periodic dihedral restraints
k (1 - cos(phi - target)) with one target per conformation, on the stepwise path only (`grappa_md_steps_*_restr_f32` through
`HipBackend.md_steps_restr`), with every combination of cutoff, constraints and implicit solvent that path takes: their gradient is
added in the force launch, a step gains no launch.  Two protocols: restrained equilibration (heavy atoms tethered while the rest
thermalises) and umbrella sampling along a torsion -- the C conformations of one call are the C windows, and `frames_dihedrals` is the
time series of the biased dihedral that WHAM / MBAR read (WHAM itself is not here).  `stepwise="auto"` goes stepwise whenever they are
given.  The tethers' reference is `restraint_reference` (default: the call's xyz); a run continued with `first_step` must pass the
ORIGINAL reference, or the tethers move to the start of the continuing call.  Frozen atoms (`Restraints.frozen`) become atoms of mass 0.
The potential energies stay the force field's (plus the solvent's); `restraint_energy` is reported beside them.  Not built: restraints in
the fused dynamics, distance, angle or flat-bottomed restraints, more than 16 dihedrals per molecule, time-dependent targets.

Replicas (`replicas=`, `grappa_amd.replica.ReplicaExchange`): a temperature ladder over the C conformations of the call, with or
without replica exchange, on the stepwise path only (`grappa_md_remd_*_f32` through `HipBackend.md_steps_remd`), with every combination
of cutoff, constraints, implicit solvent and restraints that path takes.  Conformation c is a replica that keeps its coordinates and its
noise stream; the thermostat step reads the temperature of the slot it holds, and behind every `exchange_every`-th step neighbouring
slots attempt a Metropolis swap on the potential energy (plus the restraint energy); a step gains no launch, a step with an attempt the
energy launches of a frame and two small ones.  `temperature` is then unused; velocities that are drawn are drawn at the replica's
slot temperature unless `init_temperature` is given.  `stepwise="auto"` goes stepwise whenever they are given.  The result carries
`slots`, `exchange_slots` and `exchange_energy`; `grappa_amd.replica.acceptance` gives the acceptance per pair.

The integrator is BAOAB (Leimkuhler and Matthews, J. Chem. Phys. 138, 174102 (2013)); the loop, the random stream and the units are
stated in include/grappa_hip.h.  Units: Angstrom, kcal/mol, amu, ps, K.  With friction = 0 it is velocity Verlet (NVE).  An atom of
mass 0 is frozen.  The random stream has no state: an atom's noise is a function of its molecule's 64-bit key (`mol_keys`), its index
in the molecule, the conformation and the global step, so a molecule's trajectory does not depend on its place in a batch, and a run can
be cut into launches anywhere (`steps_per_launch`) without changing a bit.  An item stops with a status:
    0  ran n_steps steps
    2  non-finite gradient (for example two non-excluded atoms on one point): stopped, the state is the one it held
    3  the molecule has more than `relax_max_atoms()` atoms: not run by the fused path (`simulate_graph` refuses such a batch before
       the launch); it cannot occur on the stepwise path
    4  (with constraints) a position constraint did not converge within its eight updates: stopped, the state is the one it held;
       `steps` counts the steps before the one that failed
    5  (with constraints or restraints) constraint or restraint tables refused on the device (an index outside the molecule, an atom
       in two clusters, a length that is not positive and finite, on the fused path more than 256 clusters; a restrained dihedral
       with a repeated atom, a negative or non-finite stiffness, a non-finite target, more than 16 rows): nothing else was written
       for the item; with replicas also a row of start slots that is no permutation, or a temperature the ladder refuses
The defaults (`MD_DEFAULTS`: 1 fs, 300 K, 1/ps) are common choices for unconstrained small molecules and are NOT tuned: nothing here
has measured which time step a given molecule tolerates (a step of 1 fs with free X-H bonds is at the edge of what BAOAB resolves).
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .nonbonded import NonbondedBatch, NonbondedParameters, as_cutoff
from .parameters import Parameters
from .relax import _stepwise_options, graph_coordinates, graph_force_field, graph_from_parameters

MD_DEFAULTS = {"dt": 0.001, "temperature": 300.0, "friction": 1.0, "init_temperature": None, "n_steps": 1000, "save_every": 0}
MAX_STEPS_PER_LAUNCH = 1000000      # the library's cap on n_steps of one call
STEPS_PER_LAUNCH_DEFAULT = 10000    # untuned: it only keeps one launch short
KB = 0.0019872041                   # kcal/mol/K (the library's value)


def md_options(**opts) -> dict:
    """the six options of a run: MD_DEFAULTS overridden by `opts`, checked (the library checks them again, per launch).
    init_temperature None (the default): the thermostat's temperature"""
    unknown = sorted(set(opts) - set(MD_DEFAULTS))
    if unknown:
        raise TypeError(f"unknown dynamics option(s) {unknown}; the options are {sorted(MD_DEFAULTS)}")
    o = {**MD_DEFAULTS, **opts}
    if o["init_temperature"] is None:
        o["init_temperature"] = o["temperature"]
    for k in ("n_steps", "save_every"):
        if isinstance(o[k], bool) or int(o[k]) != o[k] or o[k] < 0:
            raise ValueError(f"{k} must be a non-negative integer, got {o[k]}")
        o[k] = int(o[k])
    for k in ("dt", "temperature", "friction", "init_temperature"):
        if isinstance(o[k], bool) or not isinstance(o[k], (int, float, np.integer, np.floating)):
            raise ValueError(f"{k} must be a number, got {o[k]!r}")
    if not (np.isfinite(o["dt"]) and o["dt"] > 0):
        raise ValueError(f"dt must be positive and finite, got {o['dt']}")
    for k in ("temperature", "friction", "init_temperature"):
        if not (np.isfinite(o[k]) and o[k] >= 0):
            raise ValueError(f"{k} must be non-negative and finite, got {o[k]}")
    return o


def mol_keys(seed: int, B: int) -> np.ndarray:
    """(B,) uint64: the key of molecule b is output b of splitmix64 seeded with `seed` -- distinct molecules of a batch get distinct
    streams, and the same (seed, b) the same one"""
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    m = (1 << 64) - 1
    out = np.empty(B, dtype=np.uint64)
    for b in range(B):
        z = (int(seed) + (b + 1) * 0x9E3779B97F4A7C15) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        out[b] = z ^ (z >> 31)
    return out


@dataclass
class MDResult:
    """xyz, velocities: the state after the last step; potential_energy, kinetic_energy (kcal/mol) and temperature
    (2 ekin / (3 n_moving kB), n_moving = the molecule's atoms of non-zero mass; no degrees of freedom are removed -- except with
    constraints: 2 ekin / ((3 n_moving - n_constraints) kB), n_constraints = the constrained bonds with a moving end, the divisor
    floored at 1) there; steps; status (see the module text: 0, 2, 3, and with constraints 4 and 5; 3 cannot occur on the stepwise path); frames, frame_potential_energy, frame_kinetic_energy: one entry per `save_every` steps, or None.
    From `simulate_graph`: tensors on the graph's device, xyz / velocities (N, C, 3), frames (F, N, C, 3), frame energies (F, B, C),
    the others (B, C); a frame that was not reached (status 2) is NaN.  From `simulate`: numpy arrays of one molecule, xyz / velocities
    (n_confs, n_atoms, 3), frames (n_confs, n_frames, n_atoms, 3), frame energies (n_confs, n_frames), the others (n_confs,)."""
    xyz: object
    velocities: object
    potential_energy: object
    kinetic_energy: object
    temperature: object
    steps: object
    status: object
    frames: object = None
    frame_potential_energy: object = None
    frame_kinetic_energy: object = None
    esolv: object = None              # with an implicit solvent: its part of potential_energy, shaped like it; else None
    frames_esolv: object = None       # ... and of frame_potential_energy
    slots: object = None                      # with replicas: the slot of the ladder every replica holds at the end, (B, C) / (n_confs,)
    exchange_slots: object = None             # ... the slots after each of the run's X attempts, (X, B, C) / (X, n_confs)
    exchange_energy: object = None            # ... epot + E_r as the decisions read them, float64, (X, B, C) / (X, n_confs); NaN: stopped
    restraint_energy: object = None           # with restraints: E_r at xyz (potential_energy stays the force field's), (B, C) / (n_confs,)
    dihedrals: object = None                  # with restraints: the restrained dihedrals at xyz in radians, (R, C) / (R, n_confs)
    frames_restraint_energy: object = None    # ... per frame: (F, B, C) / (n_confs, n_frames); a frame not reached is NaN
    frames_dihedrals: object = None           # ... per frame: (F, R, C) / (R, n_confs, n_frames)


def _steps_take_constraints() -> bool:
    """does the backend run constraints on the stepwise path (`md_steps_cons`)?  Without it they run on the fused path only"""
    from .backend import get_backend
    return getattr(get_backend(), "md_steps_cons", None) is not None


def _host_masses(masses, N):
    """(N,) float32 on the host, checked: finite and >= 0"""
    if isinstance(masses, torch.Tensor):
        masses = masses.detach().cpu().numpy()
    m = np.asarray(masses, dtype=np.float64).reshape(-1)
    if m.shape[0] != N:
        raise ValueError(f"masses must hold one value per atom ({N}), got {m.shape[0]}")
    if not (np.isfinite(m).all() and (m >= 0).all()):
        raise ValueError("masses must be finite and >= 0 (0: a frozen atom)")
    return m.astype(np.float32)


def _host_keys(keys, seed, B):
    if keys is None:
        return mol_keys(seed, B)
    k = np.asarray(keys)
    if k.dtype.kind not in "ui" or k.reshape(-1).shape[0] != B:
        raise ValueError(f"keys must hold one 64-bit integer per molecule ({B})")
    return k.reshape(-1).astype(np.uint64)


def simulate_graph(g, masses, nonbonded: Optional[NonbondedBatch] = None, *, velocities=None, seed: int = 0, keys=None, first_step: int = 0,
                   steps_per_launch: int = STEPS_PER_LAUNCH_DEFAULT, terms=("n2", "n3", "n4", "n4_improper"), suffix: str = "",
                   offset_torsion: bool = False, stepwise=False, constraints=None, constrain_start: bool = True, cutoff=None,
                   implicit_solvent=None, gb=None, restraints=None, restraint_reference=None, replicas=None, **opts) -> MDResult:
    """Run `n_steps` BAOAB steps of every (molecule, conformation) of a parametrised batched graph: `xyz` (N, C, 3) at n1 and `k` /
    `eq` at the tuple levels, exactly what `Energy` and `relax_graph` read.  masses: (N,) in amu on the host (0: a frozen atom),
    checked before the upload.  nonbonded: the batch's `NonbondedBatch` on the graph's device (None: bonded terms only).
    velocities: (N, C, 3) on the graph's device, or None: drawn at `init_temperature`.  keys: one 64-bit key per molecule (default
    `mol_keys(seed, B)`).  first_step: the global index of the first step -- to continue a run, pass its xyz, its velocities and
    first_step + the steps it ran.  steps_per_launch: a run is cut into launches of at most this many steps (rounded down to a
    multiple of `save_every`); the result does not depend on it, it only keeps one launch short.  **opts: see MD_DEFAULTS.
    stepwise=False (the default): the fused kernel; a molecule above `relax_max_atoms()` atoms is refused here, on the host.
    stepwise=True: the whole batch through the stepwise path, which takes molecules of any size, two launches per step;
    `steps_per_launch` then bounds the steps one run call enqueues.  stepwise="auto": the fused kernel if every molecule is within the
    limit, else the whole batch stepwise -- a batch is never split between the two paths (one batch, one decomposition, one set of
    bits).  No device sync on either path.  The graph is not modified.
    constraints: a `grappa_amd.constraints.ConstraintBatch` holding the batch's molecules in order (None: unconstrained, the calls
    made are exactly those without this argument).  They run on the path that `stepwise` chooses: fused, or stepwise (`md_steps_cons`:
    stepwise=True, or "auto" for a batch above the size limit or with a cutoff).  A backend without `md_steps_cons` runs them on the fused
    path only and refuses the rest.  constrain_start=True: the start coordinates are brought to the constraint lengths and the start
    velocities projected first; False continues a run (with its xyz, velocities and first_step) bit for bit.  The first launch of
    a run gets the caller's constrain_start, later launches continue.  Statuses 4 and 5: see the module text; an item that ends with
    either in one launch of a run keeps that launch's results: later launches add no steps and no frames (NaN) for it.  A moving centre
    whose frozen leaves alone number four is refused (ValueError): they over-determine it.
    cutoff: a `grappa_amd.nonbonded.Cutoff` or a distance (None: all pairs, the calls made are exactly those without this argument):
    see the module text.  It needs `nonbonded` and the stepwise path: "auto" then goes stepwise whatever the sizes, stepwise=False is
    refused; constraints go with it.
    implicit_solvent: "obc2", "obc1" or a `grappa_amd.solvent.ImplicitSolvent` (None: vacuum, the calls made are exactly those without
    this argument) -- the GB/SA term of `grappa_amd.solvent` added to the potential, with gb, the batch's `grappa_amd.solvent.GBBatch`
    on the graph's device (radius and scale per atom).  It needs `nonbonded` (the charges) and the stepwise path: "auto" then goes
    stepwise whatever the sizes, stepwise=False is refused; constraints go with it, a cutoff does not (ValueError) unless the solvent
    carries a cutoff of its own (`ImplicitSolvent(cutoff=)`: the solvent is truncated pairwise, and `cutoff=` beside it is taken).  The result's
    potential energies include the solvent term; `esolv` / `frames_esolv` hold it alone.
    restraints: a `grappa_amd.restraints.RestraintBatch` for the graph's molecules and C on the graph's device (None: none, the calls
    made are exactly those without this argument): tethers and dihedral restraints, see the module text.  The stepwise path only:
    stepwise=False raises, "auto" goes stepwise; they go with every combination of cutoff, constraints and implicit solvent.  Frozen
    atoms of the batch get mass 0 before anything reads the masses.  restraint_reference: (N, C, 3) on the graph's device, the
    tethers' reference (None: xyz, resolved once; every launch of a long run gets that tensor, never its own start).  The result carries
    restraint_energy (B, C), dihedrals (R, C) and, with frames, frames_restraint_energy (F, B, C) and frames_dihedrals (F, R, C).
    replicas: a `grappa_amd.replica.ReplicaExchange` whose ladder has one temperature per conformation (None: none, the calls made are
    exactly those without this argument): see the module text.  The stepwise path only: stepwise=False raises, "auto" goes stepwise;
    it goes with every combination of cutoff, constraints, implicit solvent and restraints.  Exchanges need friction > 0 and a
    first_step that is a multiple of exchange_every.  Velocities that are drawn are drawn at the replica's slot temperature iff
    init_temperature was left at None.  The result carries slots (B, C), exchange_slots (X, B, C) and exchange_energy (X, B, C); a run
    is continued with `ReplicaExchange(..., slots=result.slots)`, velocities= and first_step=."""
    from .backend import get_backend
    from .solvent import GBBatch, as_implicit_solvent
    o = md_options(**opts)
    stepwise, _ = _stepwise_options(stepwise, 1)
    if replicas is not None:
        from .replica import ReplicaExchange
        if not isinstance(replicas, ReplicaExchange):
            raise TypeError(f"replicas must be a ReplicaExchange or None, got {type(replicas).__name__}")
        if stepwise is False:
            raise ValueError('simulate: replicas run on the stepwise path only: pass stepwise="auto" (or True)')
        if getattr(get_backend(), "md_steps_remd", None) is None:
            raise ValueError("simulate: the backend has no temperature ladders on the stepwise dynamics (md_steps_remd)")
        if constraints is not None and not _steps_take_constraints():
            raise ValueError("simulate: constraints run on the fused path only, replicas on the stepwise path only")
        if replicas.exchange_every > 0 and not o["friction"] > 0:
            raise ValueError("simulate: replica exchange needs a thermostat (friction > 0)")
        if replicas.exchange_every > 0 and int(first_step) % replicas.exchange_every != 0:
            raise ValueError(f"simulate: first_step must be a multiple of exchange_every ({replicas.exchange_every}), got {first_step!r}")
    if restraints is not None:
        from .restraints import RestraintBatch
        if not isinstance(restraints, RestraintBatch):
            raise TypeError(f"restraints must be a RestraintBatch or None, got {type(restraints).__name__}")
        if stepwise is False:
            raise ValueError('simulate: restraints run on the stepwise path only: pass stepwise="auto" (or True)')
        if getattr(get_backend(), "md_steps_restr", None) is None:
            raise ValueError("simulate: the backend has no restraints on the stepwise dynamics (md_steps_restr)")
        if constraints is not None and not _steps_take_constraints():
            raise ValueError("simulate: constraints run on the fused path only, restraints on the stepwise path only")
    elif restraint_reference is not None:
        raise ValueError("simulate: restraint_reference needs restraints=")
    cutoff = as_cutoff(cutoff)
    solvent = as_implicit_solvent(implicit_solvent)
    if solvent is not None:
        if cutoff is not None and solvent.cutoff is None:          # (beside a solvent that has a cutoff of its own it is taken)
            raise ValueError("simulate: an implicit solvent under a cutoff is not implemented: pass one of the two")
        if nonbonded is None:
            raise ValueError("simulate: an implicit solvent needs the nonbonded parameters (nonbonded=): they carry the charges")
        if stepwise is False:
            raise ValueError('simulate: an implicit solvent runs on the stepwise path only: pass stepwise="auto" (or True)')
        if not isinstance(gb, GBBatch):
            raise TypeError(f"simulate: an implicit solvent needs gb=, the batch's GBBatch, got {type(gb).__name__}")
        if getattr(get_backend(), "md_steps_gb", None) is None:
            raise ValueError("simulate: the backend has no implicit solvent (md_steps_gb)")
    elif gb is not None:
        raise ValueError("simulate: gb= needs implicit_solvent=")
    if cutoff is not None:
        if nonbonded is None:
            raise ValueError("simulate: a cutoff needs the nonbonded parameters (nonbonded=)")
        if stepwise is False:
            raise ValueError('simulate: a cutoff runs on the stepwise path only: pass stepwise="auto" (or True)')
        if constraints is not None and not _steps_take_constraints():
            raise ValueError("simulate: constraints run on the fused path only, a cutoff on the stepwise path only")
    if isinstance(steps_per_launch, bool) or not isinstance(steps_per_launch, (int, np.integer)) or steps_per_launch < 1:
        raise ValueError(f"steps_per_launch must be an integer >= 1, got {steps_per_launch!r}")
    if isinstance(first_step, bool) or int(first_step) != first_step or first_step < 0 or int(first_step) + o["n_steps"] >= 2 ** 32:
        raise ValueError(f"first_step must be a non-negative integer with first_step + n_steps < 2^32, got {first_step!r}")
    terms = list(terms)
    xyz, plan, counts = graph_coordinates(g, terms)
    dev = xyz.device
    limit = get_backend().relax_max_atoms()
    above = bool(counts) and max(counts) > limit
    if above and stepwise is False:
        raise ValueError(f"simulate: a molecule of {max(counts)} atoms is above the limit of {limit} atoms per molecule of the fused dynamics "
                         f"(stepwise=True or stepwise='auto' runs molecules of any size)")
    use_steps = stepwise is True or (stepwise == "auto" and (above or cutoff is not None or solvent is not None or restraints is not None
                                                             or replicas is not None))
    if solvent is not None:
        if gb.counts != list(counts):
            raise ValueError(f"the GB parameters describe molecules of {gb.counts} atoms, the batch has {list(counts)}")
        gb.check_offset(solvent.offset)          # (the batch may have been checked against another offset than the solvent's)
    if constraints is not None:
        from .constraints import ConstraintBatch
        if not isinstance(constraints, ConstraintBatch):
            raise TypeError(f"constraints must be a ConstraintBatch or None, got {type(constraints).__name__}")
        if use_steps and not _steps_take_constraints():
            raise ValueError("simulate: constraints run on the fused path only (stepwise=False, or 'auto' with every molecule within the limit)")
        if constraints.B != len(counts):
            raise ValueError(f"the constraints describe {constraints.B} molecules, the batch has {len(counts)}")
    ks, eqs, n_per = graph_force_field(g, plan, counts, nonbonded, terms, suffix, dev)
    N, B, C = plan.N, plan.B, xyz.shape[1]
    if replicas is not None and replicas.C != C:
        raise ValueError(f"the ladder has {replicas.C} temperatures, the batch has {C} conformations")
    m_host = _host_masses(masses, N)
    ref = None
    if restraints is not None:
        from .relax import check_restraint_batch
        check_restraint_batch(restraints, B, C, counts, dev)
        if restraints.frozen is not None:          # frozen atoms: mass 0, before n_moving, the degrees of freedom and check_masses read it
            m_host = np.where(restraints.frozen.cpu().numpy().reshape(-1) != 0, np.float32(0.0), m_host).astype(np.float32)
            import copy
            restraints = copy.copy(restraints)          # (the `frozen` array is not sent down)
            restraints.frozen = None
        ref = xyz
        if restraint_reference is not None:
            if not isinstance(restraint_reference, torch.Tensor) or restraint_reference.shape != xyz.shape or restraint_reference.device != dev:
                raise ValueError(f"restraint_reference must be a {tuple(xyz.shape)} tensor on {dev}")
            ref = restraint_reference.detach().float().contiguous()
    k_host = _host_keys(keys, seed, B)
    mass = torch.from_numpy(m_host).to(dev)
    key = torch.from_numpy(k_host.view(np.int64).copy()).to(dev)
    n_moving = torch.tensor([[max(int((m_host[p0:p0 + n] > 0).sum()), 1)] for p0, n in zip(np.cumsum([0] + counts[:-1]), counts)],
                            dtype=torch.float32).reshape(B, 1).to(dev)
    if constraints is not None:
        constraints.check_masses(m_host, counts)
        dof = 3.0 * n_moving - torch.from_numpy(constraints.n_constraints_host(m_host, counts).astype(np.float32)).reshape(B, 1).to(dev)
        constraints = constraints.to(dev)
    else:
        dof = 3.0 * n_moving
    vel = None
    if velocities is not None:
        if not isinstance(velocities, torch.Tensor) or velocities.shape != xyz.shape or velocities.device != dev:
            raise ValueError(f"velocities must be a {tuple(xyz.shape)} tensor on {dev}")
        vel = velocities.detach().float().contiguous()
    n_steps, every = o["n_steps"], o["save_every"]
    chunk = min(int(steps_per_launch), MAX_STEPS_PER_LAUNCH)
    if every > 0:
        chunk = max(chunk // every, 1) * every
        if chunk > MAX_STEPS_PER_LAUNCH:
            raise ValueError(f"save_every must not exceed {MAX_STEPS_PER_LAUNCH}, got {every}")
    F = n_steps // every if every > 0 else 0
    f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)      # noqa: E731
    frames = fe = fk = None
    if F:
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)      # noqa: E731
        frames, fe, fk = nan(F, N, C, 3), nan(F, B, C), nan(F, B, C)
    es = f32(B, C) if solvent is not None else None
    fs = torch.full((F, B, C), float("nan"), dtype=torch.float32, device=dev) if solvent is not None and F else None
    er = phi = fer = fphi = None
    if restraints is not None:
        er, phi = f32(B, C), f32(restraints.R, C)
        if F:
            fer, fphi = nan(F, B, C), nan(F, restraints.R, C)
    ladder = None
    if replicas is not None:          # the ladder on the device, the slots of the run and the logs of its X attempts
        K = replicas.exchange_every
        X = n_steps // K if K > 0 else 0
        i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)      # noqa: E731
        s0 = replicas.slots_for(B)
        ladder = {"T": torch.from_numpy(replicas.temperatures).to(dev), "slots": None if s0 is None else torch.from_numpy(s0).to(dev),
                  "out": i32(B, C), "xs": i32(X, B, C) if X else None,
                  "xe": torch.full((X, B, C), float("nan"), dtype=torch.float32, device=dev) if X else None,
                  "xr": torch.full((X, B, C), float("nan"), dtype=torch.float32, device=dev) if X and restraints is not None else None,
                  "at_ladder": opts.get("init_temperature") is None}
    # one call of a seam runs `seg` steps: a launch of the fused kernel, or init / run calls of at most `chunk` steps / finish of the
    # stepwise path, whose options carry the library's cap on n_steps too; calls continue one another bit for bit
    seg = chunk if not use_steps else (MAX_STEPS_PER_LAUNCH // every * every if every > 0 else MAX_STEPS_PER_LAUNCH)
    if ladder is not None and replicas.exchange_every > 0:          # (a call of the seam ends where frames and attempts both allow)
        import math
        both = math.lcm(every if every > 0 else 1, replicas.exchange_every)
        if both > MAX_STEPS_PER_LAUNCH:
            raise ValueError(f"save_every and exchange_every must have a common multiple of at most {MAX_STEPS_PER_LAUNCH}, got {both}")
        seg = MAX_STEPS_PER_LAUNCH // both * both
    bufs = [(torch.empty_like(xyz), torch.empty_like(xyz)) for _ in range(2 if n_steps > seg else 1)]
    epot, ekin = f32(B, C), f32(B, C)
    steps, status = torch.zeros(B, C, dtype=torch.int32, device=dev), torch.zeros(B, C, dtype=torch.int32, device=dev)
    total = torch.zeros(B, C, dtype=torch.int32, device=dev)
    x_in, v_in, done, launch = xyz, vel, 0, 0
    # With constraints and more than one launch: the items that have ended, and what they ended with.  The stepwise path needs none of it
    # within a call (init .. finish): there statuses 4 and 5 are sticky in the workspace, whatever the number of run calls; only a run
    # longer than the library's cap on n_steps makes a second call, and this bookkeeping then carries an ended item across it.
    held = None
    if (constraints is not None or restraints is not None) and n_steps > seg:
        held = {"dead": torch.zeros(B, C, dtype=torch.bool, device=dev)}
        atom_item = torch.repeat_interleave(torch.arange(B), torch.tensor(counts, dtype=torch.long)).to(dev)
        if restraints is not None:
            row_item = torch.repeat_interleave(torch.arange(B, device=dev), (restraints.dih_molptr[1:] - restraints.dih_molptr[:-1]).long())
    while True:
        n = min(seg, n_steps - done)
        f0, f1 = (done // every, (done + n) // every) if every > 0 else (0, 0)
        x_out, v_out = bufs[launch % len(bufs)]
        call = {"dt": o["dt"], "temperature": o["temperature"], "friction": o["friction"], "init_temperature": o["init_temperature"],
                "n_steps": n, "save_every": every, "first_step": int(first_step) + done}
        args = (plan, x_in, ks, eqs, n_per, bool(offset_torsion), nonbonded, call, mass, key, v_in, x_out, v_out, epot, ekin, steps, status)
        kw = dict(frames_xyz=frames[f0:f1] if f1 > f0 else None, frames_epot=fe[f0:f1] if f1 > f0 else None,
                  frames_ekin=fk[f0:f1] if f1 > f0 else None, atom_counts_host=counts)
        if ladder is not None:
            K = replicas.exchange_every
            a0, a1 = (done // K, (done + n) // K) if K > 0 else (0, 0)
            rows = lambda t: t[a0:a1] if t is not None and a1 > a0 else None      # noqa: E731
            rkw = {} if restraints is None else dict(
                restraints=restraints, restraint_reference=ref, restraint_energy=er, dihedral_out=phi,
                frames_restraint_energy=fer[f0:f1] if f1 > f0 else None, frames_dihedrals=fphi[f0:f1] if f1 > f0 else None)
            get_backend().md_steps_remd(*args, steps_per_call=chunk, **kw, constraints=constraints,
                                        constrain_start=bool(constrain_start) and launch == 0, gb=gb, solvent=solvent, esolv=es,
                                        frames_esolv=fs[f0:f1] if fs is not None and f1 > f0 else None,
                                        **({} if cutoff is None else {"cutoff": cutoff}), **rkw, temperatures=ladder["T"],
                                        slots=ladder["slots"], exchange_every=K, init_at_ladder=ladder["at_ladder"], slots_out=ladder["out"],
                                        exchange_slots=rows(ladder["xs"]), exchange_epot=rows(ladder["xe"]), exchange_erestr=rows(ladder["xr"]))
            ladder["slots"] = ladder["out"].clone() if n_steps > seg else ladder["out"]          # (the next call of a long run starts there)
        elif restraints is not None:
            get_backend().md_steps_restr(*args, steps_per_call=chunk, **kw, constraints=constraints,
                                         constrain_start=bool(constrain_start) and launch == 0, gb=gb, solvent=solvent, esolv=es,
                                         frames_esolv=fs[f0:f1] if fs is not None and f1 > f0 else None,
                                         **({} if cutoff is None else {"cutoff": cutoff}), restraints=restraints, restraint_reference=ref,
                                         restraint_energy=er, dihedral_out=phi, frames_restraint_energy=fer[f0:f1] if f1 > f0 else None,
                                         frames_dihedrals=fphi[f0:f1] if f1 > f0 else None)
        elif solvent is not None:
            get_backend().md_steps_gb(*args, steps_per_call=chunk, **kw, constraints=constraints,
                                      constrain_start=bool(constrain_start) and launch == 0, gb=gb, solvent=solvent, esolv=es,
                                      frames_esolv=fs[f0:f1] if fs is not None and f1 > f0 else None,
                                      **({} if cutoff is None else {"cutoff": cutoff}))
        elif use_steps and constraints is not None:
            get_backend().md_steps_cons(*args, steps_per_call=chunk, **kw, **({} if cutoff is None else {"cutoff": cutoff}),
                                        constraints=constraints, constrain_start=bool(constrain_start) and launch == 0)
        elif use_steps:
            get_backend().md_steps(*args, steps_per_call=chunk, **kw, **({} if cutoff is None else {"cutoff": cutoff}))
        elif constraints is not None:
            get_backend().md_langevin(*args, **kw, constraints=constraints, constrain_start=bool(constrain_start) and launch == 0)
        else:
            get_backend().md_langevin(*args, **kw)
        if held is None:
            total += steps
        else:
            # A non-finite state (status 2) is found again by every later launch; a constraint failure (4) is not: the next launch
            # would constrain the broken geometry afresh and run on.  So an item that has ended with 4 or 5 keeps the results of the
            # launch that ended it, and nothing a later launch writes for it counts: no steps, NaN frames.  Tensor ops only, no sync.
            alive = ~held["dead"]
            atoms = alive[atom_item][:, :, None]
            total += torch.where(alive, steps, torch.zeros_like(steps))
            for name, new, mask in (("x", x_out, atoms), ("v", v_out, atoms), ("epot", epot, alive), ("ekin", ekin, alive), ("status", status, alive)) \
                    + ((("esolv", es, alive),) if es is not None else ()) + ((("er", er, alive), ("phi", phi, None)) if er is not None else ()):
                if name == "phi":          # (a row belongs to the molecule that holds it)
                    mask = alive[row_item]
                held[name] = torch.where(mask, new, held[name]) if name in held else new.clone()
            if f1 > f0 and launch > 0:
                nanf = torch.full((), float("nan"), dtype=torch.float32, device=dev)
                frames[f0:f1] = torch.where(atoms[None], frames[f0:f1], nanf)
                fe[f0:f1], fk[f0:f1] = torch.where(alive[None], fe[f0:f1], nanf), torch.where(alive[None], fk[f0:f1], nanf)
                if fs is not None:
                    fs[f0:f1] = torch.where(alive[None], fs[f0:f1], nanf)
                if fer is not None:
                    fer[f0:f1], fphi[f0:f1] = torch.where(alive[None], fer[f0:f1], nanf), torch.where(alive[row_item][None], fphi[f0:f1], nanf)
            held["dead"] = held["dead"] | (alive & (status >= 4))
        x_in, v_in, done, launch = x_out, v_out, done + n, launch + 1
        if done >= n_steps:
            break
    if held is not None:
        x_in, v_in, epot, ekin, status = held["x"], held["v"], held["epot"], held["ekin"], held["status"]
        es = held.get("esolv", es)
        er, phi = held.get("er", er), held.get("phi", phi)
    if fer is not None and restraints.R == 0 and restraints.pos_k is None:
        fer = torch.where(torch.isnan(fe), fe, torch.zeros_like(fe))          # (nothing restrains: the library writes no frame of E_r; it is 0)
    temperature = 2.0 * ekin / (3.0 * KB * n_moving) if constraints is None else 2.0 * ekin / (KB * dof.clamp_min(1.0))
    if ladder is None:
        return MDResult(x_in, v_in, epot, ekin, temperature, total, status, frames, fe, fk, es, fs, restraint_energy=er, dihedrals=phi,
                        frames_restraint_energy=fer, frames_dihedrals=fphi)
    xen = None
    if ladder["xe"] is not None:
        xen = ladder["xe"].double() + (ladder["xr"].double() if ladder["xr"] is not None else 0.0)
    return MDResult(x_in, v_in, epot, ekin, temperature, total, status, frames, fe, fk, es, fs, slots=ladder["out"], exchange_slots=ladder["xs"],
                    exchange_energy=xen, restraint_energy=er, dihedrals=phi, frames_restraint_energy=fer, frames_dihedrals=fphi)


def simulate(parameters: Parameters, xyz, masses, nonbonded: Optional[NonbondedParameters] = None, device="cuda", *, velocities=None,
             seed: int = 0, keys=None, first_step: int = 0, steps_per_launch: int = STEPS_PER_LAUNCH_DEFAULT, stepwise=False, constraints=None,
             constrain_start: bool = True, cutoff=None, implicit_solvent=None, gb=None, restraints=None, restraint_reference=None,
             replicas=None, **opts) -> MDResult:
    """Run the conformations of ONE molecule under the parameters `Grappa.predict` returned (+ `nonbonded`; masses, nonbonded and
    velocities in the order of `parameters.atoms`), numpy in and out: xyz (n_confs, n_atoms, 3) in Angstrom, masses (n_atoms,) in amu,
    velocities (n_confs, n_atoms, 3) in A/ps or None -> MDResult (float64) with xyz and velocities of that shape, frames
    (n_confs, n_frames, n_atoms, 3), frame energies (n_confs, n_frames) and the others (n_confs,).  stepwise: see `simulate_graph`
    (the stepwise path takes a molecule of any size).  constraints: the molecule's `grappa_amd.constraints.Constraints` in the order of
    `parameters.atoms` (None: unconstrained), constrain_start: see `simulate_graph`.  cutoff: see `simulate_graph`.
    implicit_solvent: see `simulate_graph`; gb: the molecule's `grappa_amd.solvent.GBParameters` in the order of `parameters.atoms`.
    restraints: the molecule's `grappa_amd.restraints.Restraints` in the order of `parameters.atoms` (None: none), restraint_reference
    (n_confs, n_atoms, 3) or None (xyz): see `simulate_graph`; the result then carries restraint_energy (n_confs,), dihedrals
    (R, n_confs), frames_restraint_energy (n_confs, n_frames) and frames_dihedrals (R, n_confs, n_frames).
    replicas: a `grappa_amd.replica.ReplicaExchange` with one temperature per conformation (None: none): see `simulate_graph`; the
    result then carries slots (n_confs,), exchange_slots (X, n_confs) and exchange_energy (X, n_confs)."""
    from .solvent import GBBatch, GBParameters, as_implicit_solvent
    md_options(**opts)
    _stepwise_options(stepwise, 1)
    extra = {}
    if replicas is not None:
        from .replica import ReplicaExchange
        if not isinstance(replicas, ReplicaExchange):
            raise TypeError(f"replicas must be a ReplicaExchange or None, got {type(replicas).__name__}")
        if stepwise is False:
            raise ValueError('simulate: replicas run on the stepwise path only: pass stepwise="auto" (or True)')
        if replicas.C != int(np.asarray(xyz).shape[0]):
            raise ValueError(f"the ladder has {replicas.C} temperatures, the molecule has {int(np.asarray(xyz).shape[0])} conformations")
        extra["replicas"] = replicas
    if restraints is not None:
        from .restraints import Restraints
        if not isinstance(restraints, Restraints):
            raise TypeError(f"restraints must be Restraints or None, got {type(restraints).__name__}")
        if stepwise is False:
            raise ValueError('simulate: restraints run on the stepwise path only: pass stepwise="auto" (or True)')
    elif restraint_reference is not None:
        raise ValueError("simulate: restraint_reference needs restraints=")
    cutoff = as_cutoff(cutoff)
    solvent = as_implicit_solvent(implicit_solvent)
    if solvent is not None:
        if cutoff is not None and solvent.cutoff is None:          # (beside a solvent that has a cutoff of its own it is taken)
            raise ValueError("simulate: an implicit solvent under a cutoff is not implemented: pass one of the two")
        if nonbonded is None:
            raise ValueError("simulate: an implicit solvent needs the nonbonded parameters (nonbonded=): they carry the charges")
        if stepwise is False:
            raise ValueError('simulate: an implicit solvent runs on the stepwise path only: pass stepwise="auto" (or True)')
        if not isinstance(gb, GBParameters):
            raise TypeError(f"simulate: an implicit solvent needs gb=, the molecule's GBParameters, got {type(gb).__name__}")
        extra.update(implicit_solvent=solvent, gb=GBBatch([gb], solvent.offset).to(device))
    elif gb is not None:
        raise ValueError("simulate: gb= needs implicit_solvent=")
    if cutoff is not None:
        if nonbonded is None:
            raise ValueError("simulate: a cutoff needs the nonbonded parameters (nonbonded=)")
        if stepwise is False:
            raise ValueError('simulate: a cutoff runs on the stepwise path only: pass stepwise="auto" (or True)')
        if constraints is not None and not _steps_take_constraints():
            raise ValueError("simulate: constraints run on the fused path only, a cutoff on the stepwise path only")
        extra["cutoff"] = cutoff
    if constraints is not None:
        from .constraints import ConstraintBatch, Constraints
        if not isinstance(constraints, Constraints):
            raise TypeError(f"constraints must be a Constraints or None, got {type(constraints).__name__}")
        extra.update(constraints=ConstraintBatch([constraints]), constrain_start=constrain_start)
    g = graph_from_parameters(parameters, xyz)
    n = g.num_nodes("n1")
    nb = None
    if nonbonded is not None:
        if not isinstance(nonbonded, NonbondedParameters):
            raise TypeError(f"nonbonded must be NonbondedParameters or None, got {type(nonbonded).__name__}")
        if nonbonded.n_atoms != n:
            raise ValueError(f"the nonbonded parameters describe {nonbonded.n_atoms} atoms, the molecule has {n}")
        nb = NonbondedBatch([nonbonded]).to(device)
    m_host = _host_masses(masses, n)
    vel = None
    if velocities is not None:
        v = np.asarray(velocities, dtype=np.float32)
        if v.shape != np.asarray(xyz).shape:
            raise ValueError(f"velocities must have the shape of xyz {np.asarray(xyz).shape}, got {v.shape}")
        vel = torch.from_numpy(np.ascontiguousarray(v.transpose(1, 0, 2))).to(device)
    if restraints is not None:
        from .restraints import RestraintBatch
        extra["restraints"] = RestraintBatch([restraints], int(np.asarray(xyz).shape[0]), atom_counts=[n]).to(device)
        if restraint_reference is not None:
            ref = np.asarray(restraint_reference, dtype=np.float32)
            if ref.shape != np.asarray(xyz).shape:
                raise ValueError(f"restraint_reference must have the shape of xyz {np.asarray(xyz).shape}, got {ref.shape}")
            extra["restraint_reference"] = torch.from_numpy(np.ascontiguousarray(ref.transpose(1, 0, 2))).to(device)
    r = simulate_graph(g.to(device), m_host, nb, velocities=vel, seed=seed, keys=keys, first_step=first_step, steps_per_launch=steps_per_launch,
                       stepwise=stepwise, **extra, **opts)
    np64 = lambda t: t.cpu().numpy().astype(np.float64)      # noqa: E731
    confs = lambda t: np64(t).transpose(1, 0, 2)      # noqa: E731  (N, C, 3) -> (C, N, 3)
    has = r.frames is not None
    return MDResult(confs(r.xyz), confs(r.velocities), np64(r.potential_energy)[0], np64(r.kinetic_energy)[0], np64(r.temperature)[0],
                    r.steps.cpu().numpy()[0], r.status.cpu().numpy()[0], np64(r.frames).transpose(2, 0, 1, 3) if has else None,
                    np64(r.frame_potential_energy)[:, 0].T if has else None, np64(r.frame_kinetic_energy)[:, 0].T if has else None,
                    np64(r.esolv)[0] if r.esolv is not None else None, np64(r.frames_esolv)[:, 0].T if r.frames_esolv is not None else None,
                    slots=r.slots.cpu().numpy()[0] if r.slots is not None else None,
                    exchange_slots=r.exchange_slots.cpu().numpy()[:, 0] if r.exchange_slots is not None else None,
                    exchange_energy=np64(r.exchange_energy)[:, 0] if r.exchange_energy is not None else None,
                    restraint_energy=np64(r.restraint_energy)[0] if r.restraint_energy is not None else None,
                    dihedrals=np64(r.dihedrals) if r.dihedrals is not None else None,
                    frames_restraint_energy=np64(r.frames_restraint_energy)[:, 0].T if r.frames_restraint_energy is not None else None,
                    frames_dihedrals=np64(r.frames_dihedrals).transpose(1, 2, 0) if r.frames_dihedrals is not None else None)
