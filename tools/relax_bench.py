"""Time the fused FIRE minimiser (csrc/relax.hip through HipBackend.relax_fire) with device events, after warm-up, on 256 molecules of
the pool x 32 conformations under bonded + nonbonded terms, against the same loop composed from the entry points that existed before it:
HipBackend.mm_gradient_fwd, HipBackend.nonbonded and a FIRE update in stock torch ops with per-item state, one step per iteration
(its tables and the nonbonded work-item list are built once, outside the timed region; the fused side is timed through relax_graph,
table preparation included).

Both run a fixed number of steps (tolerance 0), so a step is the same work in both: rates are item steps per second (an item is one
(molecule, conformation)) and molecules per second at that step count.  Force constants are synthetic (k_bond 500, k_angle 100, three
proper and two improper periodicities), equilibrium values are those of the pool geometry, conformations are jittered by 0.05 A.

    python tools/relax_bench.py [--out profiles/relax_bench.txt] [--steps 200] [--composed-steps 50]

--restraints times something else on the same pool workload: the restrained instantiation of the kernel (csrc/relax.hip, one restrained dihedral,
k = 239 kcal/mol, target 0.5 rad from the start, on every molecule that has a proper) against the unrestrained one, both in this
process, device events, median of --reps runs of the same fixed number of steps.

    python tools/relax_bench.py --restraints [--out profiles/relax_restr_bench.txt]
"""
import argparse
import datetime
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from grappa_amd.constants import TUPLE_LEVELS      # noqa: E402
from grappa_amd.nonbonded import NonbondedBatch, NonbondedParameters      # noqa: E402
from grappa_amd.relax import RELAX_DEFAULTS      # noqa: E402


def pool_batch(n_mols, n_confs, seed=0):
    """-> (graph on the device with k / eq at the tuple levels, NonbondedBatch on the device)"""
    from grappa_amd.datasets import build_batch_from_pool, pool_molecule, pool_size
    ids = [k % pool_size() for k in range(n_mols)]
    g = build_batch_from_pool(ids, n_confs=n_confs, seed=seed)
    rng = np.random.default_rng(seed)
    params, x0 = [], []
    for k in ids:
        z, bonds, xyz0 = pool_molecule(k)
        q = rng.normal(0, 0.3, len(z))
        params.append(NonbondedParameters.from_bonds(bonds, q - q.mean(), np.where(z == 1, 1.1, 3.3), np.where(z == 1, 0.016, 0.1)))
        x0.append(xyz0)
    x0 = torch.from_numpy(np.concatenate(x0).astype(np.float64))
    g.nodes["n1"].data["xyz"] = (x0[:, None, :] + torch.from_numpy(rng.normal(0, 0.05, size=(x0.shape[0], n_confs, 3)))).float()
    gen = torch.Generator().manual_seed(seed)
    idx = {lv: g.nodes[lv].data["idxs"].long() for lv in TUPLE_LEVELS}
    d = x0[idx["n2"][:, 0]] - x0[idx["n2"][:, 1]]
    u, v = x0[idx["n3"][:, 0]] - x0[idx["n3"][:, 1]], x0[idx["n3"][:, 2]] - x0[idx["n3"][:, 1]]
    g.nodes["n2"].data["k"], g.nodes["n2"].data["eq"] = torch.full((len(d),), 500.0), d.norm(dim=-1).float()
    g.nodes["n3"].data["k"] = torch.full((len(u),), 100.0)
    g.nodes["n3"].data["eq"] = torch.atan2(torch.cross(u, v, dim=-1).norm(dim=-1), (u * v).sum(-1)).float()
    g.nodes["n4"].data["k"] = (torch.rand(len(idx["n4"]), 3, generator=gen) * 2 - 1) * torch.tensor([1.0, 0.5, 0.3])
    g.nodes["n4_improper"].data["k"] = (torch.rand(len(idx["n4_improper"]), 2, generator=gen) * 2 - 1) * torch.tensor([1.0, 0.5])
    return g.to("cuda"), NonbondedBatch(params).to("cuda")


def pool_restraints(g, n_confs):
    """one restrained dihedral per molecule of the batch that has a proper (its first), in every conformation 0.5 rad from the start
    dihedral of conformation 0 -> (RestraintBatch on the device, molecules restrained)"""
    from grappa_amd.restraints import RestraintBatch, Restraints, dihedral_angle
    counts = [int(c) for c in g.batch_num_nodes_host("n1")]
    ptr = np.concatenate([[0], np.cumsum(counts)])
    idx = g.nodes["n4"].data["idxs"].long().cpu().numpy()
    first = g.plan().mol_ptr["n4"].cpu().numpy()
    x = g.nodes["n1"].data["xyz"][:, 0].double().cpu().numpy()
    items = []
    for b in range(len(counts)):
        if first[b + 1] == first[b]:
            items.append(None)
            continue
        row = idx[first[b]] - ptr[b]
        phi = dihedral_angle(x[ptr[b]:ptr[b + 1]], *row)
        items.append(Restraints(dihedrals=[row], dihedral_k=239.0, dihedral_targets=[(phi + 0.5 + np.pi) % (2 * np.pi) - np.pi]))
    return RestraintBatch(items, n_confs, atom_counts=counts).to("cuda"), sum(r is not None for r in items)


class Composed:
    """the loop of include/grappa_hip.h (grappa_relax_fire_f32) one step per iteration: two gradient kernels, then torch ops"""

    def __init__(self, be, g, nb, opts):
        from grappa_amd.energy import mm_tables
        self.be, self.plan, self.nb, self.o = be, g.plan(), nb, opts
        self.x0 = g.nodes["n1"].data["xyz"].float().contiguous()
        self.x = self.x0.clone()
        ks, eqs, self.n_per = mm_tables(g, self.plan, list(TUPLE_LEVELS), "", self.x.device)
        self.ks, self.eqs = [k.contiguous() for k in ks], [None if q is None else q.contiguous() for q in eqs]
        N, C = self.x.shape[:2]
        B = self.plan.B
        counts = torch.from_numpy(g.batch_num_nodes_host("n1")).to(self.x.device)
        self.am = torch.repeat_interleave(torch.arange(B, device=self.x.device), counts)
        self.B, self.C = B, C
        self.reset()
        self.gm, self.gn = torch.empty_like(self.x), torch.empty_like(self.x)
        self.e = torch.empty(B, C, device=self.x.device)
        self.nbplan = be.nonbonded_plan(nb.atom_molptr_host, nb.N, C, self.x.device)

    def reset(self):
        """back to the start: coordinates, velocities and the per-item FIRE state (the tables and the work-item list stay)"""
        dev = self.x0.device
        self.x = self.x0.clone()
        self.v = torch.zeros_like(self.x0)
        self.h = torch.full((self.B, self.C), self.o["dt_start"], device=dev)
        self.al = torch.full((self.B, self.C), self.o["alpha_start"], device=dev)
        self.npos = torch.zeros(self.B, self.C, dtype=torch.int32, device=dev)

    def _sum(self, t):
        return torch.zeros_like(self.h).index_add_(0, self.am, t)

    def step(self):
        o, nb = self.o, self.nb
        self.be.mm_gradient_fwd(self.plan, self.x, self.ks, self.eqs, self.n_per, self.gm)
        self.be.nonbonded(self.x, nb.atom_molptr, nb.charge, nb.sigma, nb.epsilon, nb.exc_ptr, nb.exc_atom, nb.exc_qq, nb.exc_sigma, nb.exc_eps,
                          self.e, None, self.gn, plan=self.nbplan)
        F = -(self.gm + self.gn)
        P, Fn, vn = self._sum((F * self.v).sum(-1)), self._sum((F * F).sum(-1)).sqrt(), self._sum((self.v * self.v).sum(-1)).sqrt()
        pos = P > 0
        mix = torch.where(pos, self.al * (vn / Fn), torch.zeros_like(P))
        keep = torch.where(pos, 1 - self.al, torch.zeros_like(P))
        grow = pos & (self.npos >= o["n_min"])
        self.h = torch.where(pos, torch.where(grow, (self.h * o["f_inc"]).clamp_max(o["dt_max"]), self.h), self.h * o["f_dec"])
        self.al = torch.where(pos, torch.where(grow, self.al * o["f_alpha"], self.al), torch.full_like(self.al, o["alpha_start"]))
        self.npos = torch.where(pos, self.npos + 1, torch.zeros_like(self.npos))
        am = self.am
        v = keep[am][..., None] * self.v + mix[am][..., None] * F + self.h[am][..., None] * F
        d = self.h[am][..., None] * v
        dm = torch.zeros_like(self.h).index_reduce_(0, am, d.norm(dim=-1), "amax", include_self=True)
        s = torch.where(dm > 0, (o["max_disp"] / dm).clamp_max(1.0), torch.ones_like(dm))
        self.x = self.x + s[am][..., None] * d
        self.v = s[am][..., None] * v


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return float(np.median(us)), float(np.min(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mols", type=int, default=256)
    ap.add_argument("--confs", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--composed-steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--restraints", action="store_true", help="time the restrained kernel against the unrestrained one instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("relax_bench: needs a GPU (there is nothing to time without one)")
    from grappa_amd.backend import get_backend
    from grappa_amd.relax import relax_graph
    be = get_backend()
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# command: python {' '.join(sys.argv)}",
             f"# date: {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}",
             f"# device: {prop.name}, {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, {prop.total_memory / 2 ** 30:.0f} GiB; "
             f"library built for {be.lib.grappa_build_arch().decode()}; torch {torch.__version__}",
             "# device events around whole runs, median (min) after one warm-up run; this file is the tool's output, unedited"]
    g, nb = pool_batch(args.mols, args.confs)
    counts = g.batch_num_nodes_host("n1")
    items = args.mols * args.confs
    lines.append(f"pool: {args.mols} molecules, {int(counts.sum())} atoms ({int(counts.min())}..{int(counts.max())} per molecule), C = {args.confs}, "
                 f"{items} items, bonded + nonbonded, tolerance 0")
    print("\n".join(lines), flush=True)

    def report(what, steps, med, mn, launches):
        lines.append(f"{what:12s} {steps:5d} steps {med / 1e3:10.2f} ms (min {mn / 1e3:10.2f})  {items * steps / (med * 1e-6):10.3e} item steps/s  "
                     f"{args.mols / (med * 1e-6):10.3e} molecules/s at {steps} steps x {args.confs} conformations  {launches:6d} library launches")
        print(lines[-1], flush=True)
        return items * steps / (med * 1e-6)

    if args.restraints:
        rb, n_restr = pool_restraints(g, args.confs)
        lines.append(f"restraints: one dihedral (k = 239 kcal/mol, target 0.5 rad from the start) on {n_restr} of {args.mols} molecules")
        run = {"unrestrained": lambda: relax_graph(g, nb, tolerance=0.0, max_steps=args.steps),
               "restrained": lambda: relax_graph(g, nb, tolerance=0.0, max_steps=args.steps, restraints=rb)}
        rate = {}
        for what, fn in run.items():
            n0 = be.lib.grappa_launch_count(0)
            r = fn()
            n1 = be.lib.grappa_launch_count(0)
            assert bool((r.steps == args.steps).all()) and bool((r.status == 0).all())
            rate[what] = report(what, args.steps, *timed(fn, args.reps), n1 - n0)
        lines.append(f"restrained / unrestrained = {rate['restrained'] / rate['unrestrained']:.3f}x item steps/s")
        print(lines[-1], flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    opts = {**RELAX_DEFAULTS, "tolerance": 0.0}
    n0 = be.lib.grappa_launch_count(0)
    r = relax_graph(g, nb, tolerance=0.0, max_steps=args.steps)
    n1 = be.lib.grappa_launch_count(0)
    assert bool((r.steps == args.steps).all()) and bool((r.status == 0).all())
    f_rate = report("fused", args.steps, *timed(lambda: relax_graph(g, nb, tolerance=0.0, max_steps=args.steps), args.reps), n1 - n0)

    c = Composed(be, g, nb, opts)          # tables, clones and the nonbonded work-item list: built once, outside the timed region

    def composed():
        c.reset()
        for _ in range(args.composed_steps):
            c.step()
    n0 = be.lib.grappa_launch_count(0)
    composed()
    n1 = be.lib.grappa_launch_count(0)
    fx = relax_graph(g, nb, tolerance=0.0, max_steps=args.composed_steps).xyz
    lines.append(f"agreement after {args.composed_steps} steps: largest |x_fused - x_composed| = {float((fx - c.x).abs().max()):.3e} A")
    print(lines[-1], flush=True)
    c_rate = report("composed", args.composed_steps, *timed(composed, args.reps), n1 - n0)
    lines.append(f"fused / composed = {f_rate / c_rate:.1f}x item steps/s (the composed loop also issues its torch ops: not counted as library launches)")
    print(lines[-1], flush=True)
    d = relax_graph(g, nb)
    torch.cuda.synchronize()
    lines.append(f"defaults (tolerance {RELAX_DEFAULTS['tolerance']:.4f}, max_steps {RELAX_DEFAULTS['max_steps']}): {int((d.status == 1).sum())} of {items} items converged, "
                 f"steps median {int(d.steps.float().median())} max {int(d.steps.max())}; "
                 f"{timed(lambda: relax_graph(g, nb), 3)[0] / 1e3:.2f} ms per call")
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
