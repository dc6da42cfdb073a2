"""`Grappa`: inference wrapper, `predict(Molecule) -> Parameters` (reference grappa.py:14-57)."""
import torch

from . import constants, settings
from .batch import check_disconnected_graphs
from .model import GrappaModel
from .molecule import Molecule
from .parameters import Parameters


class Grappa:
    def __init__(self, model: GrappaModel, max_element: int = constants.MAX_ELEMENT, device: str = "cuda", reference_water_guard: bool = False) -> None:
        # reference_water_guard=True: `predict` behaves exactly like the reference's on a graph that holds water (it parametrises it: the
        # reference's guard never fires, see batch.check_disconnected_graphs); default: the intended guard, which raises
        self.reference_water_guard = bool(reference_water_guard)
        self.model = model.to(device)
        self.model.eval()
        self.max_element = max_element
        self.device = device
        self.field_of_view = model.field_of_view
        # repeated shapes replay a recorded hipGraph instead of issuing ~450 launches from Python (grappa_amd/capture.py; GRAPPA_PREDICT_GRAPHS=0: never)
        self._graphs = None
        if str(device).startswith("cuda") and settings.read("predict_graphs"):
            from .capture import ForwardCache
            self._graphs = ForwardCache(self.model, device)

    @classmethod
    def from_tag(cls, tag: str = "latest", max_element=constants.MAX_ELEMENT, device: str = "cuda", models_dir=None, reference_water_guard: bool = False) -> "Grappa":
        """a released model ('latest', 'grappa-1.2', 'grappa-1.1', ...) or a `.pth` exported into the models directory (grappa.py:26-35)"""
        from .loading import model_from_tag
        return cls(model_from_tag(tag, models_dir), max_element, device, reference_water_guard)

    @classmethod
    def from_file(cls, path, max_element=constants.MAX_ELEMENT, device: str = "cuda", config=None, trusted=None, reference_water_guard: bool = False) -> "Grappa":
        """an exported `.pth` container or a training checkpoint (`best-model.ckpt`) of the reference or of `grappa_amd.trainer`.  trusted=True:
        the caller vouches for a file that holds pickled objects beyond tensors (loading._torch_load; default: tensors only)"""
        from .loading import model_from_path
        return cls(model_from_path(path, config, trusted), max_element, device, reference_water_guard)

    def predict(self, molecule: Molecule) -> Parameters:
        if self.model.training:                  # (eval() walks every sub-module: 1 ms of a 7 ms call when there is nothing to switch)
            self.model.eval()
        g = molecule.to_dgl(max_element=self.max_element, exclude_feats=[])
        # water guard.  NOTE: the reference compares argmax(one-hot) (= Z-1) with {1, 8} and therefore never
        # fires (utils/dgl_utils.py:231-234); the intended check (elements {H, O}) is implemented here.
        check_disconnected_graphs(g, reference_water_guard=self.reference_water_guard)
        if self._graphs is not None:
            done = self._graphs(g)
            if done is not None:
                return Parameters.from_dgl(done)
        g = g.to(self.device)
        with torch.no_grad():
            g = self.model(g)
        g = g.to("cpu")
        return Parameters.from_dgl(g)

    def relax(self, molecule: Molecule, xyz, nonbonded=None, *, stepwise=False, check_every: int = 32, cutoff=None, implicit_solvent=None,
              **opts):
        """`predict` followed by `grappa_amd.relax.relax`: the conformations xyz (n_confs, n_atoms, 3) of `molecule` minimised on the
        device under the predicted bonded parameters (+ `nonbonded`: NonbondedParameters in the molecule's atom order) -> RelaxResult.
        stepwise=False: the fused kernel (molecules up to `relax_max_atoms()` atoms); True or "auto": the stepwise path for molecules
        of any size, which syncs with the host once per chunk of `check_every` steps (see `grappa_amd.relax.relax_graph`).
        cutoff: a `grappa_amd.nonbonded.Cutoff` or a distance in Angstrom (None: all pairs): the minimisation under the nonbonded
        cutoff that `simulate(..., cutoff=)` runs under, on the stepwise path; the result's energy is then the sum of the cut terms;
        it needs `nonbonded` and stepwise="auto" (or True).
        implicit_solvent: "obc2", "obc1" or a `grappa_amd.solvent.ImplicitSolvent` (None: vacuum): the minimisation under the GB/SA
        Hamiltonian that `simulate(..., implicit_solvent=)` runs under, with the radii and screening factors of the molecule's
        elements and bonds (`GBParameters.from_elements`; gb= in **opts overrides them); the result's energy then includes the
        solvent term and `esolv` holds it alone; it needs `nonbonded` and stepwise="auto" (or True) and goes with neither a cutoff
        nor restraints"""
        from .relax import relax
        if cutoff is not None:
            opts = {**opts, "cutoff": cutoff}
        if implicit_solvent is not None:
            from .solvent import GBParameters
            opts = {**opts, "implicit_solvent": implicit_solvent}
            if opts.get("gb") is None:
                pos = {int(a): i for i, a in enumerate(molecule.atoms)}          # bonds name atoms by id; the tables go by position
                opts["gb"] = GBParameters.from_elements(molecule.atomic_numbers, [(pos[int(a)], pos[int(b)]) for a, b in molecule.bonds])
        return relax(self.predict(molecule), xyz, nonbonded, device=self.device, stepwise=stepwise, check_every=check_every, **opts)

    def torsion_scan(self, molecule: Molecule, xyz, dihedral, angles=None, nonbonded=None, **kw):
        """`predict` followed by `grappa_amd.relax.torsion_scan`: a relaxed scan of the dihedral (four atom ids of the molecule) from the
        conformation xyz (n_atoms, 3) under the predicted bonded parameters (+ `nonbonded`) -> ScanResult.  All grid points run in one
        launch and are independent of each other.  **kw: k and the options of `relax`"""
        from .relax import torsion_scan
        return torsion_scan(self.predict(molecule), xyz, dihedral, angles, nonbonded, device=self.device, **kw)

    def simulate(self, molecule: Molecule, xyz, nonbonded=None, *, stepwise=False, constraints=None, cutoff=None, implicit_solvent=None,
                 restraints=None, restraint_reference=None, replicas=None, **kw):
        """`predict` followed by `grappa_amd.dynamics.simulate`: Langevin dynamics (BAOAB) of the conformations xyz
        (n_confs, n_atoms, 3) of `molecule` on the device under the predicted bonded parameters (+ `nonbonded`: NonbondedParameters in
        the molecule's atom order), with the atomic masses of `constants.ATOMIC_MASSES` -> MDResult.  stepwise=False: the fused kernel
        (molecules up to `relax_max_atoms()` atoms); True or "auto": the stepwise path for molecules of any size.  **kw: velocities,
        seed, keys, first_step, steps_per_launch, constrain_start and the options of `MD_DEFAULTS` (see
        `grappa_amd.dynamics.simulate_graph`).  constraints: None, "h-bonds" (every X-H bond held at its predicted equilibrium length:
        `grappa_amd.constraints.hydrogen_constraints`) or a `Constraints` in the molecule's atom order, on either path
        (`constraints="h-bonds", stepwise="auto", cutoff=9.0`: a protein at 2 fs steps).
        cutoff: a `grappa_amd.nonbonded.Cutoff` or a distance in Angstrom (None: all pairs): the nonbonded term with a cutoff and a
        reaction field on the stepwise path, which skips the atom tiles beyond it -- what makes a protein fast, not only movable; it
        needs `nonbonded` and stepwise="auto" (or True).
        implicit_solvent: "obc2", "obc1" or a `grappa_amd.solvent.ImplicitSolvent` (None: vacuum): the GB/SA term of
        `grappa_amd.solvent` with the mbondi2 radii and OBC screening factors of the molecule's elements and bonds
        (`GBParameters.from_elements`; gb= in **kw overrides them); it needs `nonbonded` and stepwise="auto" (or True), goes with
        constraints and not with a cutoff (`implicit_solvent="obc2", constraints="h-bonds", stepwise="auto"`) -- unless the solvent
        carries a cutoff of its own: `implicit_solvent=ImplicitSolvent("obc2", cutoff=12.0)` truncates the solvent pairwise and skips
        far tiles, and then `cutoff=` (usually `Cutoff(rc, rs, rf_dielectric=1.0)`) is taken beside it.
        restraints: a `grappa_amd.restraints.Restraints` in the molecule's atom order (None: none) -- tethers to
        restraint_reference (n_confs, n_atoms, 3; None: xyz), dihedral restraints with one target per conformation (the windows of an
        umbrella run) and frozen atoms, on the stepwise path with any of the above (stepwise="auto" or True): see
        `grappa_amd.dynamics.simulate`
        replicas: a `grappa_amd.replica.ReplicaExchange` with one temperature per conformation (None: none) -- a temperature ladder
        over the conformations, with or without replica exchange, on the stepwise path with any of the above (stepwise="auto" or True)"""
        from .dynamics import simulate
        if replicas is not None:
            kw = {**kw, "replicas": replicas}
        if restraints is not None:
            kw = {**kw, "restraints": restraints, "restraint_reference": restraint_reference}
        elif restraint_reference is not None:
            raise ValueError("simulate: restraint_reference needs restraints=")
        if cutoff is not None:
            kw = {**kw, "cutoff": cutoff}
        if implicit_solvent is not None:
            from .solvent import GBParameters
            kw = {**kw, "implicit_solvent": implicit_solvent}
            if kw.get("gb") is None:
                pos = {int(a): i for i, a in enumerate(molecule.atoms)}          # bonds name atoms by id; the tables go by position
                kw["gb"] = GBParameters.from_elements(molecule.atomic_numbers, [(pos[int(a)], pos[int(b)]) for a, b in molecule.bonds])
        masses = [constants.ATOMIC_MASSES[int(z)] for z in molecule.atomic_numbers]
        parameters = self.predict(molecule)
        if isinstance(constraints, str):
            if constraints != "h-bonds":
                raise ValueError(f"constraints must be None, 'h-bonds' or a Constraints, got {constraints!r}")
            from .constraints import hydrogen_constraints
            constraints = hydrogen_constraints(parameters, molecule.atomic_numbers)
        if constraints is None:
            return simulate(parameters, xyz, masses, nonbonded, device=self.device, stepwise=stepwise, **kw)
        return simulate(parameters, xyz, masses, nonbonded, device=self.device, stepwise=stepwise, constraints=constraints, **kw)
