"""Writes tests/golden/ref_evaluator.npz: the reference's own bootstrapped `Evaluator` (training/evaluation.py:164-386) on four batches.

    python tools/make_evaluator_golden.py

Runs only where the reference is installed (it is imported through oracle/make_goldens.py, whose helpers build the graphs: the
reference's Molecule.to_dgl -> set_number_confs -> dgl_utils.batch on the pure-torch DGL shim).  22 molecules in 4 batches, three
dataset names of which 'dsC' holds a single molecule, two batches with dummy-padded conformations; predictions, references and the
classical force field's values ('_classical_ff' against '_qm') are seeded random numbers written into the batched graphs -- the
evaluator never looks at where they came from.  Dummy slots hold large values: whatever reads them is off by orders of magnitude.

The file holds
  b{i}::*                     the inputs of batch i (the tensors of the batched graph, atoms per molecule, dataset names)
  ds_names, ds_counts         datasets in the order of their first molecule, molecules of each
  index_matrix                (64, 22) int32: row 0 the full datasets, rows 1.. the reference's own np.random.choice draws of
                              pool(n_bootstrap=64, seed=3), recorded while it ran; columns grouped by dataset, local indices
  ref::pool0::{ds}::{m}       pool(0)                                   f64::pool0::{ds}::{m}
  ref::boot::{ds}::{m}::mean / ::std   pool(n_bootstrap=64, seed=3)     f64::boot::{ds}::{m}::mean / ::std
where f64:: is the same quantity from the same inputs and the same resamples in float64: centring, differences and norms in double,
np.std (two passes) for the unbiased stds, exactly rounded sums (math.fsum) for the mean and the two-pass std over the replicates."""
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_goldens as mg  # noqa: E402  (puts the reference and the DGL shim on sys.path)
for _name in ("matplotlib", "matplotlib.pyplot"):          # plot helpers of the evaluation module only, never called here
    sys.modules.setdefault(_name, types.ModuleType(_name))
from grappa.training.evaluation import Evaluator as RefEvaluator  # noqa: E402

N_BOOTSTRAP, SEED = 64, 3
SUFFIXES = dict(suffix="", suffix_ref="_ref", suffix_classical="_classical_ff", suffix_classical_ref="_qm")
SPECS = [dict(ids=(40, 6), n_confs=5, seed=31, pad={1: 2, 4: 3}, names=["dsA", "dsB", "dsA", "dsB", "dsA", "dsB"]),
         dict(ids=(500, 6), n_confs=6, seed=37, pad=None, names=["dsB", "dsB", "dsA", "dsC", "dsA", "dsB"]),
         dict(ids=(900, 5), n_confs=4, seed=41, pad={0: 3}, names=["dsA", "dsA", "dsB", "dsB", "dsA"]),
         dict(ids=(1300, 5), n_confs=7, seed=43, pad=None, names=["dsB", "dsA", "dsB", "dsA", "dsA"])]


def batches():
    out = []
    for bi, sp in enumerate(SPECS):
        ids = mg.pick_small(sp["ids"][1], 8, 22, start=sp["ids"][0])
        mols = mg.build_inputs(ids, n_confs=sp["n_confs"], seed=sp["seed"], charge_model="amber99", pad_confs_of=sp["pad"])
        g = mg.ref_dgl_utils.batch([mg.ref_graph(m, sp["n_confs"], False)[0] for m in mols])
        rng = np.random.default_rng(1000 + bi)
        B, C, N = len(mols), sp["n_confs"], g.num_nodes("n1")
        e_ref = g.nodes["g"].data["energy_ref"].numpy()
        g_ref = g.nodes["n1"].data["gradient_ref"].numpy()
        dummy = g.nodes["g"].data["is_dummy"].numpy() != 0
        new = {("g", "energy"): e_ref + rng.normal(0, 0.8, (B, C)) + rng.normal(0, 5, (B, 1)),
               ("g", "energy_qm"): rng.normal(0, 4, (B, C)) + 40.0, ("n1", "gradient"): g_ref + rng.normal(0, 2.5, (N, C, 3)),
               ("n1", "gradient_qm"): rng.normal(0, 12, (N, C, 3))}
        new[("g", "energy_classical_ff")] = new[("g", "energy_qm")] + rng.normal(0, 1.5, (B, C)) - 25.0
        new[("n1", "gradient_classical_ff")] = new[("n1", "gradient_qm")] + rng.normal(0, 4.0, (N, C, 3))
        atom_mol = np.repeat(np.arange(B), [len(m["z"]) for m in mols])
        for (nt, k), v in new.items():
            v = v.astype(np.float32)
            if nt == "g":
                v[dummy] = 1e6                     # dummy slots: anything that reads them shows
            else:
                v[dummy[atom_mol]] = -1e6
            g.nodes[nt].data[k] = torch.from_numpy(v)
        out.append((g, sp["names"], [len(m["z"]) for m in mols]))
    return out


def per_molecule_f64(bs):
    """-> per dataset (order of the first molecule) the list of per-molecule float64 arrays the metrics are made of"""
    ds = {}
    for g, names, counts in bs:
        gd, n1 = g.nodes["g"].data, g.nodes["n1"].data
        ptr = np.concatenate([[0], np.cumsum(counts)])
        for b, name in enumerate(names):
            real = gd["is_dummy"][b].numpy() == 0
            rec = {}
            for tag, sfx in SUFFIXES.items():
                e = gd[f"energy{sfx}"][b].numpy().astype(np.float64)[real]
                rec["e" + tag] = e - e.mean()
                rec["g" + tag] = n1[f"gradient{sfx}"][ptr[b]:ptr[b + 1]].numpy().astype(np.float64)[:, real].reshape(-1, 3)
            ds.setdefault(name, []).append(rec)
    return ds


def metrics_f64(mols, sel):
    cat = {k: np.concatenate([mols[i][k] for i in sel]) for k in mols[0]}
    d, dg = cat["esuffix"] - cat["esuffix_ref"], cat["gsuffix"] - cat["gsuffix_ref"]
    dc, dgc = cat["esuffix_classical"] - cat["esuffix_classical_ref"], cat["gsuffix_classical"] - cat["gsuffix_classical_ref"]
    return {"std_energies": np.std(cat["esuffix_ref"], ddof=1), "std_gradients": np.std(cat["gsuffix_ref"], ddof=1) * np.sqrt(3.0),
            "rmse_energies": np.sqrt(np.mean(d * d)), "mae_energies": np.mean(np.abs(d)),
            "rmse_gradients": np.sqrt(np.mean((dg * dg).sum(-1))), "crmse_gradients": np.sqrt(np.mean(dg * dg)),
            "mae_gradients": np.mean(np.sqrt((dg * dg).sum(-1))),
            "rmse_classical_energies_from_ref": np.sqrt(np.mean(dc * dc)), "rmse_classical_gradients_from_ref": np.sqrt(np.mean((dgc * dgc).sum(-1))),
            "crmse_classical_gradients_from_ref": np.sqrt(np.mean(dgc * dgc))}


def main():
    bs = batches()
    ev = RefEvaluator(calculate_classical=True, **SUFFIXES)
    d = {"n_batches": np.array([len(bs)])}
    for bi, (g, names, counts) in enumerate(bs):
        with torch.no_grad():
            ev.step(g, names)
        for nt, keys in (("g", ("energy", "energy_ref", "energy_classical_ff", "energy_qm", "is_dummy")),
                         ("n1", ("gradient", "gradient_ref", "gradient_classical_ff", "gradient_qm"))):
            for k in keys:
                d[f"b{bi}::{k}"] = mg.to_np(g.nodes[nt].data[k])
        d[f"b{bi}::atoms_per_mol"], d[f"b{bi}::dsnames"] = np.array(counts), np.array(names)
    pool0 = ev.pool(0)
    # the reference's draws, recorded while its pool() runs
    draws, choice = [], np.random.choice
    np.random.choice = lambda *a, **k: draws.append(np.asarray(choice(*a, **k))) or draws[-1]
    try:
        boot = ev.pool(n_bootstrap=N_BOOTSTRAP, seed=SEED)
    finally:
        np.random.choice = choice
    ds_names = list(ev.energies.keys())
    n_of = [len(ev.energies[n]) for n in ds_names]
    assert len(draws) == (N_BOOTSTRAP - 1) * len(ds_names) and sum(n_of) >= 20 and 1 in n_of
    idx = np.empty((N_BOOTSTRAP, sum(n_of)), dtype=np.int32)
    idx[0] = np.concatenate([np.arange(n) for n in n_of])
    for r in range(1, N_BOOTSTRAP):
        idx[r] = np.concatenate(draws[(r - 1) * len(ds_names):r * len(ds_names)])
    d["ds_names"], d["ds_counts"], d["index_matrix"] = np.array(ds_names), np.array(n_of), idx
    mols = per_molecule_f64(bs)
    assert list(mols) == ds_names
    off = np.concatenate([[0], np.cumsum(n_of)])
    for j, name in enumerate(ds_names):
        reps = [metrics_f64(mols[name], idx[r, off[j]:off[j + 1]]) for r in range(N_BOOTSTRAP)]
        assert pool0[name]["n_mols"] == n_of[j] and pool0[name]["n_confs"] == sum(len(m["esuffix"]) for m in mols[name])
        d[f"ref::pool0::{name}::n_confs"], d[f"ref::pool0::{name}::n_mols"] = np.array([pool0[name]["n_confs"]]), np.array([n_of[j]])
        for m in reps[0]:
            xs = [float(r[m]) for r in reps]
            mean = math.fsum(xs) / len(xs)
            std = math.sqrt(math.fsum((x - mean) ** 2 for x in xs) / len(xs))
            ref = (pool0[name][m], boot[name][m]["mean"], boot[name][m]["std"])
            assert all(np.isfinite(v) for v in ref + (xs[0], mean, std)), (name, m)
            d[f"ref::pool0::{name}::{m}"], d[f"f64::pool0::{name}::{m}"] = np.array([ref[0]]), np.array([xs[0]])
            d[f"ref::boot::{name}::{m}::mean"], d[f"f64::boot::{name}::{m}::mean"] = np.array([ref[1]]), np.array([mean])
            d[f"ref::boot::{name}::{m}::std"], d[f"f64::boot::{name}::{m}::std"] = np.array([ref[2]]), np.array([std])
            print(f"{name:4s} {m:36s} ref {ref[0]:.9g}  f64 {xs[0]:.17g}   boot ref {ref[1]:.9g} +- {ref[2]:.9g}  f64 {mean:.17g} +- {std:.17g}")
    path = os.path.join(ROOT, "tests", "golden", "ref_evaluator.npz")
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path), "bytes;", dict(zip(ds_names, n_of)))


if __name__ == "__main__":
    main()
