"""Time the fused Langevin dynamics (csrc/dynamics.hip through simulate_graph) with device events, after warm-up, on 256 molecules of
the pool x 32 conformations under bonded + nonbonded terms, against the same BAOAB step composed from the entry points that existed
before it: HipBackend.mm_gradient_fwd, HipBackend.nonbonded and an update in stock torch ops (noise from torch.randn), one step per
iteration; its tables and the nonbonded work-item list are built once, outside the timed region.

The timed quantity is item steps per second (an item is one (molecule, conformation); the steps counted are those that were run).  Force constants are synthetic and the batch is
relax_bench's (tools/relax_bench.py pool_batch); masses are the standard atomic masses.  Every stage that touches the GPU is a child
process of its own under a time limit; the parent never initialises the GPU, stops at the first stage that fails and starts nothing
after it.

    python tools/md_bench.py [--out profiles/md_bench.txt] [--steps 2000] [--composed-steps 50]

--constraints times the constrained kernel (csrc/dynamics_cons.hip) next to the unconstrained one instead: the same batch with every
X-H bond of the pool molecules held at its start length (`Constraints.from_bonds`), both kernels in one child process, the
unconstrained one at 1 fs and the constrained one at 2 fs and at 1 fs, with the workload's charges and again with them quartered (the
full charges pull atoms onto each other, which ends items early).  What constraints have to earn is a per-step cost below twice the
unconstrained kernel's: then a picosecond at 2 fs costs less wall time than at 1 fs without them.

    python tools/md_bench.py --constraints [--out profiles/md_cons_bench.txt] [--steps 2000]
"""
import argparse
import datetime
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

OPTS = dict(dt=0.001, temperature=300.0, friction=1.0, init_temperature=300.0)
ACC, KB = 418.4, 0.0019872041
STAGE_LIMIT = {"device": 300, "fused": 300, "composed": 300, "agreement": 300, "cons": 300}      # seconds


def _batch(args):
    import numpy as np
    from relax_bench import pool_batch
    from grappa_amd.constants import ATOMIC_MASSES
    from grappa_amd.datasets import pool_molecule, pool_size
    g, nb = pool_batch(args.mols, args.confs)
    masses = np.concatenate([[ATOMIC_MASSES[int(z)] for z in pool_molecule(k % pool_size())[0]] for k in range(args.mols)]).astype(np.float32)
    return g, nb, masses


def _constraints(args):
    """every bond between a hydrogen and a heavy atom of the batch's molecules, at its length in the pool's geometry"""
    import numpy as np
    from grappa_amd.constraints import ConstraintBatch, Constraints
    from grappa_amd.datasets import pool_molecule, pool_size
    items = []
    for k in range(args.mols):
        z, bonds, xyz0 = pool_molecule(k % pool_size())
        items.append(Constraints.from_bonds(bonds, z == 1, np.linalg.norm(xyz0[bonds[:, 0]] - xyz0[bonds[:, 1]], axis=-1)))
    return ConstraintBatch(items)


def _timed(fn, reps):
    import numpy as np
    import torch
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


class Composed:
    """the loop of include/grappa_hip.h (grappa_md_langevin_f32) one step per iteration: two gradient kernels, then torch ops"""

    def __init__(self, be, g, nb, masses, friction):
        import numpy as np
        import torch
        from grappa_amd.constants import TUPLE_LEVELS
        from grappa_amd.energy import mm_tables
        self.be, self.plan, self.nb = be, g.plan(), nb
        self.x0 = g.nodes["n1"].data["xyz"].float().contiguous()
        dev = self.x0.device
        ks, eqs, self.n_per = mm_tables(g, self.plan, list(TUPLE_LEVELS), "", dev)
        self.ks, self.eqs = [k.contiguous() for k in ks], [None if q is None else q.contiguous() for q in eqs]
        w = (1.0 / torch.from_numpy(masses).to(dev))[:, None, None]
        dt = OPTS["dt"]
        self.h2, self.kw = 0.5 * dt, 0.5 * dt * ACC * w
        self.c1 = float(np.exp(-friction * dt))
        self.sg = float(np.sqrt(1.0 - self.c1 ** 2)) * torch.sqrt(ACC * KB * OPTS["temperature"] * w)
        self.thermostat = friction > 0
        self.gm, self.gn = torch.empty_like(self.x0), torch.empty_like(self.x0)
        self.e = torch.empty(self.plan.B, self.x0.shape[1], device=dev)
        self.nbplan = be.nonbonded_plan(nb.atom_molptr_host, nb.N, self.x0.shape[1], dev)

    def force(self):
        nb = self.nb
        self.be.mm_gradient_fwd(self.plan, self.x, self.ks, self.eqs, self.n_per, self.gm)
        self.be.nonbonded(self.x, nb.atom_molptr, nb.charge, nb.sigma, nb.epsilon, nb.exc_ptr, nb.exc_atom, nb.exc_qq, nb.exc_sigma, nb.exc_eps,
                          self.e, None, self.gn, plan=self.nbplan)
        return self.gm + self.gn

    def reset(self, v):
        self.x, self.v = self.x0.clone(), v.clone()
        self.g = self.force()

    def step(self):
        import torch
        v = self.v - self.kw * self.g
        x = self.x + self.h2 * v
        if self.thermostat:
            v = self.c1 * v + self.sg * torch.randn_like(v)
        self.x = x + self.h2 * v
        self.g = self.force()
        self.v = v - self.kw * self.g


def stage(args):
    """one GPU stage in this (child) process -> a JSON line on stdout"""
    import torch
    if not torch.cuda.is_available():
        sys.exit("md_bench: needs a GPU (there is nothing to time without one)")
    from grappa_amd.backend import get_backend
    from grappa_amd.dynamics import simulate_graph
    be = get_backend()
    if args.stage == "device":
        prop = torch.cuda.get_device_properties(0)
        print(json.dumps({"device": f"{prop.name}, {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, "
                                    f"{prop.total_memory / 2 ** 30:.0f} GiB; library built for {be.lib.grappa_build_arch().decode()}; torch {torch.__version__}"}))
        return
    g, nb, masses = _batch(args)
    counts = g.batch_num_nodes_host("n1")
    out = {"atoms": int(counts.sum()), "smallest": int(counts.min()), "largest": int(counts.max())}
    def fused(n, constraints=None, **kw):
        extra = {} if constraints is None else {"constraints": constraints}
        return simulate_graph(g, masses, nb, n_steps=n, steps_per_launch=args.steps_per_launch, **extra, **{**OPTS, **kw})

    if args.stage == "cons":
        cb = _constraints(args).to("cuda")
        out["constraints"], out["clusters"] = int(sum(c.n_constraints for c in cb.items)), cb.K
        # twice: with the workload's charges, which pull some atoms onto each other (items then stop early, and a workgroup that leaves
        # early skews the time per step run), and with the charges quartered, where items are meant to survive
        for tag, scale in (("", 1.0), ("_calm", 0.25)):
            nb.charge.mul_(scale)
            nb.exc_qq.mul_(scale * scale)
            for name, kw in (("free_1fs", dict(dt=0.001)), ("cons_2fs", dict(dt=0.002, constraints=cb)), ("cons_1fs", dict(dt=0.001, constraints=cb))):
                r = fused(args.steps, **kw)
                med, low = _timed(lambda: fused(args.steps, **kw), args.reps)
                out[name + tag] = {"item_steps": int(r.steps.sum()), "status": {int(k): int((r.status == k).sum()) for k in r.status.unique()},
                                   "median_us": med, "min_us": low, "temperature": float(r.temperature[r.status == 0].mean())}
    elif args.stage == "fused":
        n0 = be.lib.grappa_launch_count(0)
        r = fused(args.steps)
        out["launches"] = int(be.lib.grappa_launch_count(0) - n0)
        # (an item that meets a non-finite gradient -- the synthetic charges can pull two atoms onto one point -- stops early: the rate
        # counts the steps that were run, and the report says how many items stopped)
        out["item_steps"], out["stopped"] = int(r.steps.sum()), int((r.status != 0).sum())
        out["median_us"], out["min_us"] = _timed(lambda: fused(args.steps), args.reps)
        out["temperature"] = float(r.temperature.mean())
    else:
        friction = OPTS["friction"] if args.stage == "composed" else 0.0
        c = Composed(be, g, nb, masses, friction)          # tables, clones and the nonbonded work-item list: outside the timed region
        v0 = fused(0, friction=friction).velocities

        def composed():
            c.reset(v0)
            for _ in range(args.composed_steps):
                c.step()
        if args.stage == "composed":
            n0 = be.lib.grappa_launch_count(0)
            composed()
            out["launches"] = int(be.lib.grappa_launch_count(0) - n0)
            out["median_us"], out["min_us"] = _timed(composed, args.reps)
        else:          # agreement without a thermostat: the two sides draw different noise
            composed()
            r = simulate_graph(g, masses, nb, velocities=v0, n_steps=args.composed_steps, **{**OPTS, "friction": 0.0})
            out["max_dx"] = float((r.xyz - c.x).abs().max())
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mols", type=int, default=256)
    ap.add_argument("--confs", type=int, default=32)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--steps-per-launch", type=int, default=10000)
    ap.add_argument("--composed-steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--constraints", action="store_true", help="time the constrained kernel next to the unconstrained one")
    ap.add_argument("--stage", default=None, choices=sorted(STAGE_LIMIT))
    args = ap.parse_args()
    if args.stage:
        return stage(args)
    lines = [f"# command: python {' '.join(sys.argv)}",
             f"# date: {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}"]
    items = args.mols * args.confs

    def run(name):
        cmd = ["timeout", "-k", "10", str(STAGE_LIMIT[name]), sys.executable, os.path.abspath(__file__), "--stage", name] + \
              [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("mols", "confs", "steps", "steps_per_launch", "composed_steps", "reps")]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"md_bench: stage {name} ended with status {p.returncode}; nothing more is started")
        return json.loads(p.stdout.strip().splitlines()[-1])

    def report(what, steps, r):
        rate = r.get("item_steps", items * steps) / (r["median_us"] * 1e-6)
        lines.append(f"{what:10s} {steps:6d} steps {r['median_us'] / 1e3:10.2f} ms (min {r['min_us'] / 1e3:10.2f})  {rate:10.3e} item steps/s  "
                     f"{r['launches']:6d} library launches")
        print(lines[-1], flush=True)
        return rate

    lines.append(f"# device: {run('device')['device']}")
    lines.append("# device events around whole runs, median (min) after one warm-up run; every stage a process of its own; this file is the tool's output, unedited")
    if args.constraints:
        c = run("cons")
        lines.append(f"pool: {args.mols} molecules, {c['atoms']} atoms ({c['smallest']}..{c['largest']} per molecule), C = {args.confs}, {items} items, "
                     f"bonded + nonbonded, {OPTS['temperature']} K, friction {OPTS['friction']} / ps; {c['constraints']} X-H constraints in "
                     f"{c['clusters']} clusters per conformation; the three runs in one process")
        for tag, title in (("", "the workload's charges"), ("_calm", "charges x 0.25")):
            per = {}
            lines.append(f"-- {title}")
            for name, what in (("free_1fs", "unconstrained, 1 fs"), ("cons_2fs", "constrained, 2 fs"), ("cons_1fs", "constrained, 1 fs")):
                r = c[name + tag]
                per[name] = r["median_us"] / max(r["item_steps"], 1)
                lines.append(f"{what:20s} {args.steps:6d} steps {r['median_us'] / 1e3:10.2f} ms (min {r['min_us'] / 1e3:10.2f})  "
                             f"{r['item_steps'] / (r['median_us'] * 1e-6):10.3e} item steps/s  {r['item_steps']} item steps run, items by status "
                             f"{r['status']}, mean kinetic temperature of the status-0 items at the end {r['temperature']:.1f} K")
            lines.append(f"time per item step, constrained 2 fs / unconstrained 1 fs = {per['cons_2fs'] / per['free_1fs']:.3f} (below 2: a picosecond "
                         f"costs less wall time constrained); constrained 1 fs / unconstrained 1 fs = {per['cons_1fs'] / per['free_1fs']:.3f}")
        print("\n".join(lines), flush=True)
        out = args.out or os.path.join(ROOT, "profiles", "md_cons_bench.txt")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return
    f = run("fused")
    lines.append(f"pool: {args.mols} molecules, {f['atoms']} atoms ({f['smallest']}..{f['largest']} per molecule), C = {args.confs}, {items} items, "
                 f"bonded + nonbonded, dt {OPTS['dt']} ps, {OPTS['temperature']} K, friction {OPTS['friction']} / ps")
    print("\n".join(lines), flush=True)
    f_rate = report("fused", args.steps, f)
    lines.append(f"fused: {f['item_steps']} item steps run, {f['stopped']} of {items} items stopped early on a non-finite gradient; mean kinetic "
                 f"temperature at the end: {f['temperature']:.1f} K")
    c_rate = report("composed", args.composed_steps, run("composed"))
    lines.append(f"fused / composed = {f_rate / c_rate:.1f}x item steps/s (the composed loop also issues its torch ops: not counted as library launches)")
    lines.append(f"agreement after {args.composed_steps} steps without thermostat: largest |x_fused - x_composed| = {run('agreement')['max_dx']:.3e} A")
    print("\n".join(lines[-3:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
