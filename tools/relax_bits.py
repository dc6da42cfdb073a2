"""Digest the results of the fused FIRE minimiser (csrc/relax.hip through the public `relax_graph`), free and restrained, on the pool
workload of tools/relax_bench.py (its `pool_batch` and `pool_restraints`): SHA-256 of the bytes of xyz, energy, gradient_max, steps,
status, restraint_energy and dihedrals after a fixed number of steps (tolerance 0) and after a call with the default tolerance.  An
item's bits depend on its own input only, so two builds of the library that compute the same thing print the same lines: run it at
both and compare the outputs.

    python tools/relax_bits.py [--out FILE] [--steps 200]
"""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from relax_bench import pool_batch, pool_restraints      # noqa: E402

FIELDS = ("xyz", "energy", "gradient_max", "steps", "status", "restraint_energy", "dihedrals")


def digest(t):
    return "-" if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mols", type=int, default=256)
    ap.add_argument("--confs", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("relax_bits: needs a GPU")
    from grappa_amd.relax import relax_graph
    g, nb = pool_batch(args.mols, args.confs)
    rb, n_restr = pool_restraints(g, args.confs)
    lines = [f"pool: {args.mols} molecules x {args.confs} conformations, bonded + nonbonded; one restrained dihedral on {n_restr} molecules"]
    runs = ((f"free, tolerance 0, {args.steps} steps", dict(tolerance=0.0, max_steps=args.steps)),
            (f"restrained, tolerance 0, {args.steps} steps", dict(tolerance=0.0, max_steps=args.steps, restraints=rb)),
            ("free, defaults", dict()), ("restrained, defaults", dict(restraints=rb)))
    for what, kw in runs:
        r = relax_graph(g, nb, **kw)
        torch.cuda.synchronize()
        lines.append(f"{what}: steps {int(r.steps.min())}..{int(r.steps.max())}, status {sorted(set(r.status.flatten().tolist()))}")
        lines += [f"  {f:17s} {digest(getattr(r, f))}" for f in FIELDS]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
