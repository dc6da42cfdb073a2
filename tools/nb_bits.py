"""Digest what the tiled pair loop (csrc/nb_loop.h) computes through each of its callers: SHA-256 of the bytes of

  the nonbonded term    HipBackend.nonbonded with the list built on the device, with the plan, and under a cutoff with prune = 0 and 1
                        (energy, terms, gradient; under a cutoff also tiles)
  relax_graph           stepwise, tolerance 0, a fixed step count (xyz, energy, gradient_max, steps, status)
  simulate_graph        stepwise, with and without a cutoff, with and without a thermostat (xyz, velocities, both energies, steps, status)

on the pool batch of tools/nonbonded_bench.py (tools/relax_bench.py's for the two stepwise paths, which need the bonded tables too), a
513-atom chain and a 16,448-atom chain (257 j-tiles: the second batch of verdicts of csrc/nb_cut.h).  An item's bits depend on its own
input only, so two builds of the library that compute the same thing print the same lines: run it at both and compare the outputs.

    python tools/nb_bits.py [--out FILE] [--mols 32] [--confs 8] [--steps 20] [--cutoff 10]
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nonbonded_bench      # noqa: E402
import relax_bench      # noqa: E402
from md_bench import OPTS      # noqa: E402
from relax_steps_bench import chain_graph      # noqa: E402

CHAINS = (513, 16448)
CARBON = 12.011


def digest(t):
    return "-" if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def term_lines(be, params, xyz, cutoff):
    """the nonbonded term of one workload, every way the library computes it"""
    from grappa_amd.nonbonded import Cutoff, NonbondedBatch
    nb = NonbondedBatch(params).to("cuda")
    x = torch.from_numpy(xyz).to("cuda")
    tabs = (x, nb.atom_molptr, nb.charge, nb.sigma, nb.epsilon, nb.exc_ptr, nb.exc_atom, nb.exc_qq, nb.exc_sigma, nb.exc_eps)
    plan = be.nonbonded_plan(nb.atom_molptr.cpu(), nb.N, x.shape[1], "cuda")
    runs = (("list built on the device", {}), ("planned", dict(plan=plan)),
            ("cut, prune 0", dict(plan=plan, cutoff=Cutoff(cutoff, 0.8 * cutoff, prune=False))),
            ("cut, prune 1", dict(plan=plan, cutoff=Cutoff(cutoff, 0.8 * cutoff, prune=True))))
    lines = []
    for what, kw in runs:
        e, te, g = torch.zeros(nb.B, x.shape[1], device="cuda"), torch.zeros(2, nb.B, x.shape[1], device="cuda"), torch.zeros_like(x)
        tiles = torch.zeros(plan[1], dtype=torch.int32, device="cuda") if "cutoff" in kw else None
        be.nonbonded(*tabs, e, te, g, **kw, **({} if tiles is None else {"tiles": tiles}))
        torch.cuda.synchronize()
        lines.append(f"  nonbonded, {what}" + ("" if tiles is None else f": {int(tiles.sum())} tiles over {plan[1]} items"))
        lines += [f"    {f:17s} {digest(t)}" for f, t in (("energy", e), ("terms", te), ("grad", g), ("tiles", tiles))]
    return lines


def stepwise_lines(g, nb, masses, steps, cutoff):
    from grappa_amd.dynamics import simulate_graph
    from grappa_amd.nonbonded import Cutoff
    from grappa_amd.relax import relax_graph
    r = relax_graph(g, nb, tolerance=0.0, max_steps=steps, stepwise=True)
    torch.cuda.synchronize()
    lines = [f"  relax_graph, stepwise, tolerance 0, {steps} steps: steps {int(r.steps.min())}..{int(r.steps.max())}, "
             f"status {sorted(set(r.status.flatten().tolist()))}"]
    lines += [f"    {f:17s} {digest(getattr(r, f))}" for f in ("xyz", "energy", "gradient_max", "steps", "status")]
    for cut in (None, Cutoff(cutoff, 0.8 * cutoff)):
        for friction in (OPTS["friction"], 0.0):
            kw = {} if cut is None else {"cutoff": cut}
            m = simulate_graph(g, masses, nb, n_steps=steps, stepwise=True, **kw, **{**OPTS, "friction": friction})
            torch.cuda.synchronize()
            lines.append(f"  simulate_graph, stepwise, {'all pairs' if cut is None else f'cutoff {cutoff} A'}, friction {friction}, {steps} steps: "
                         f"steps {int(m.steps.min())}..{int(m.steps.max())}, status {sorted(set(m.status.flatten().tolist()))}")
            lines += [f"    {f:17s} {digest(getattr(m, f))}" for f in ("xyz", "velocities", "potential_energy", "kinetic_energy", "steps", "status")]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mols", type=int, default=32)
    ap.add_argument("--confs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cutoff", type=float, default=10.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("nb_bits: needs a GPU")
    from grappa_amd.backend import get_backend
    from grappa_amd.constants import ATOMIC_MASSES
    from grappa_amd.datasets import pool_molecule, pool_size
    from grappa_amd.nonbonded import NonbondedBatch
    be = get_backend()
    lines = [f"pool: {args.mols} molecules x {args.confs} conformations"]
    lines += term_lines(be, *nonbonded_bench.pool_batch(args.mols, args.confs), args.cutoff)
    g, nb = relax_bench.pool_batch(args.mols, args.confs)
    masses = np.concatenate([[ATOMIC_MASSES[int(z)] for z in pool_molecule(k % pool_size())[0]] for k in range(args.mols)]).astype(np.float32)
    lines += stepwise_lines(g, nb, masses, args.steps, args.cutoff)
    for n in CHAINS:
        lines.append(f"chain: 1 molecule of {n} atoms, 1 conformation")
        lines += term_lines(be, *nonbonded_bench.chain(n), args.cutoff)
        gh, nbp = chain_graph(n)
        lines += stepwise_lines(gh.to("cuda"), NonbondedBatch([nbp]).to("cuda"), np.full(n, CARBON, dtype=np.float32), args.steps, args.cutoff)
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
