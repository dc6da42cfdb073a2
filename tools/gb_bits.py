"""Digest what the ALL-PAIRS solvent kernels compute through each of their callers: SHA-256 of the bytes of

  the solvent entry     HipBackend.gb_obc without a cutoff, with and without the gradient (energy, terms, gradient, Born radii)
  simulate_graph        stepwise in the solvent, with and without a thermostat and with X-H style constraints
                        (xyz, velocities, both energies, esolv, steps, status)
  relax_graph           stepwise in the solvent, tolerance 0, a fixed step count (xyz, energy, gradient_max, steps, status)

on the pool batch of tools/nonbonded_bench.py (tools/relax_bench.py's for the stepwise paths), a 513-atom chain and a 16,448-atom
chain.  It uses nothing that came with the solvent's cutoff, so it runs on a tree from before it: an item's bits depend on its own input
only, so two builds of the library that compute the same thing print the same lines -- run it at both and compare the outputs.

    python tools/gb_bits.py [--out FILE] [--mols 32] [--confs 8] [--steps 20]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nonbonded_bench      # noqa: E402
import relax_bench      # noqa: E402
from md_bench import OPTS      # noqa: E402
from nb_bits import CARBON, CHAINS, digest      # noqa: E402
from relax_steps_bench import chain_graph      # noqa: E402

MODEL = "obc2"


def _gb(counts):
    from grappa_amd.solvent import GBBatch, GBParameters
    return GBBatch([GBParameters(np.full(int(n), 1.7), np.full(int(n), 0.72)) for n in counts]).to("cuda")


def entry_lines(params, xyz):
    from grappa_amd.nonbonded import NonbondedBatch
    nb = NonbondedBatch(params).to("cuda")
    gb = _gb([p.n_atoms for p in params])
    x = torch.from_numpy(xyz).to("cuda")
    lines = []
    for what, gradient in (("with the gradient", True), ("energy alone", False)):
        r = gb.evaluate(nb, x, MODEL, terms=True, gradient=gradient, born_radii=gradient)
        torch.cuda.synchronize()
        lines.append(f"  gb_obc, {MODEL}, all pairs, {what}")
        lines += [f"    {f:17s} {digest(r[f])}" for f in ("energy", "terms", "grad", "born")]
    return lines


def stepwise_lines(g, nb, masses, steps, cons=None):
    from grappa_amd.dynamics import simulate_graph
    from grappa_amd.relax import relax_graph
    gb = _gb(g.batch_num_nodes_host("n1"))
    lines = []
    for friction in (OPTS["friction"], 0.0):
        for c in ((None,) if cons is None else (None, cons)):
            kw = {} if c is None else {"constraints": c}
            m = simulate_graph(g, masses, nb, n_steps=steps, stepwise=True, implicit_solvent=MODEL, gb=gb, **kw, **{**OPTS, "friction": friction})
            torch.cuda.synchronize()
            lines.append(f"  simulate_graph, stepwise, {MODEL}, friction {friction}, {'free' if c is None else 'constrained'}, {steps} steps: "
                         f"steps {int(m.steps.min())}..{int(m.steps.max())}, status {sorted(set(m.status.flatten().tolist()))}")
            lines += [f"    {f:17s} {digest(getattr(m, f))}" for f in ("xyz", "velocities", "potential_energy", "kinetic_energy", "esolv", "steps", "status")]
    r = relax_graph(g, nb, tolerance=0.0, max_steps=steps, stepwise=True, implicit_solvent=MODEL, gb=gb)
    torch.cuda.synchronize()
    lines.append(f"  relax_graph, stepwise, {MODEL}, tolerance 0, {steps} steps: steps {int(r.steps.min())}..{int(r.steps.max())}, "
                 f"status {sorted(set(r.status.flatten().tolist()))}")
    lines += [f"    {f:17s} {digest(getattr(r, f))}" for f in ("xyz", "energy", "gradient_max", "steps", "status")]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mols", type=int, default=32)
    ap.add_argument("--confs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gb_bits: needs a GPU")
    from grappa_amd.constants import ATOMIC_MASSES
    from grappa_amd.datasets import pool_molecule, pool_size
    from grappa_amd.nonbonded import NonbondedBatch
    from md_steps_bench import _leaves
    from grappa_amd.constraints import ConstraintBatch
    lines = [f"pool: {args.mols} molecules x {args.confs} conformations"]
    lines += entry_lines(*nonbonded_bench.pool_batch(args.mols, args.confs))
    g, nb = relax_bench.pool_batch(args.mols, args.confs)
    masses = np.concatenate([[ATOMIC_MASSES[int(z)] for z in pool_molecule(k % pool_size())[0]] for k in range(args.mols)]).astype(np.float32)
    lines += stepwise_lines(g, nb, masses, args.steps)
    for n in CHAINS:
        lines.append(f"chain: 1 molecule of {n} atoms, 1 conformation")
        lines += entry_lines(*nonbonded_bench.chain(n))
        gh, nbp = chain_graph(n)
        m, cons = _leaves(n, CARBON)          # every second atom a leaf held to the atom before it (tools/md_steps_bench.py)
        lines += stepwise_lines(gh.to("cuda"), NonbondedBatch([nbp]).to("cuda"), m, args.steps, ConstraintBatch([cons]))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
