"""grappa_amd: MI355X-native engine for the Grappa hot path (GrappaModel forward / predict, Energy,
MolwiseLoss train step) behind the reference's Python API.  See DESIGN.md."""
from .batch import MolBatch, batch, unbatch, set_number_confs, delete_dummy_confs
from .molecule import Molecule
from .parameters import Parameters
from .model import GrappaModel
from .energy import Energy
from .loss import MolwiseLoss
from .deploy import get_default_model_config, model_from_config, model_from_dict
from .grappa import Grappa
from .loading import model_from_tag, model_from_path
from .evaluation import Evaluator, FastEvaluator, eval_model
from .schedule import TrainSchedule
from .device_dataset import DeviceDataset
from .dataset import Dataset
from .moldata import MolData
from .trainer import Trainer
from .relax import RelaxResult, ScanResult, relax, relax_graph, torsion_scan
from .dynamics import MDResult, simulate, simulate_graph
from .constraints import ConstraintBatch, Constraints, hydrogen_constraints
from .restraints import RestraintBatch, Restraints, set_dihedral
from .replica import ReplicaExchange, acceptance

__all__ = ["MolBatch", "batch", "unbatch", "set_number_confs", "delete_dummy_confs", "Molecule", "Parameters", "GrappaModel",
           "Energy", "MolwiseLoss", "get_default_model_config", "model_from_config", "model_from_dict", "model_from_tag", "model_from_path", "Grappa", "FastEvaluator", "Evaluator", "eval_model",
           "TrainSchedule", "DeviceDataset", "Dataset", "MolData", "Trainer", "RelaxResult", "relax", "relax_graph", "MDResult", "simulate", "simulate_graph",
           "Constraints", "ConstraintBatch", "hydrogen_constraints", "Restraints", "RestraintBatch", "set_dihedral", "ScanResult", "torsion_scan",
           "ReplicaExchange", "acceptance"]
