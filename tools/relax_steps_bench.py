"""Time the stepwise FIRE minimiser (csrc/relax_steps.hip through relax_graph(stepwise=True)) with device events, after warm-up, with
tolerance 0 and a fixed step count, so that all sides do equal work; milliseconds per step at three sizes:

  (a) pool    256 molecules of the pool x 32 conformations: the fused kernel against the stepwise path -- what stepwise=True costs where
              it is not needed, and the case for stepwise="auto"
  (b) chain   one synthetic chain of 2,600 atoms, 1 conformation: stepwise against the same loop composed from the entry points that
              existed before it (mm_gradient_fwd, the planned nonbonded kernel and a FIRE update in stock torch ops: tools/relax_bench.py's
              Composed, tables built outside the timed region), and a sweep of check_every over 1, 8, 32, 128
  (c) chain   the 50,046-atom chain of tools/nonbonded_bench.py: stepwise against composed

The sides of a size are timed alternately, `--reps` times each after one warm-up run each; every row gives the median, the minimum and
the maximum.  The chains carry bonds, angles and proper torsions along the chain (k_bond 500, k_angle 100, three periodicities) with the
lattice geometry as equilibrium, and the nonbonded parameters of tools/nonbonded_bench.py.

With --cutoff RC [--switch RS] the tool measures the nonbonded cutoff of relax(..., cutoff=) instead: at the two chains three sides --
all pairs, the cutoff with prune = 1 and with prune = 0 -- timed alternately by the same protocol (device events, one warm-up run, `--reps`
runs each), all run times printed, with the tiles the cut energy kernel evaluates at the start coordinates.  Every size is a child
process of its own under `timeout`; after one that fails nothing more is started.

With --implicit-solvent MODEL (obc2, obc1) the tool measures relax(..., implicit_solvent=) instead: per size the all-pairs vacuum step
against the step in the solvent, on the same tree, timed alternately by the same protocol (device events, one warm-up run, `--reps` runs
each), all run times printed with the library launches.  Four sizes: the pool batch, a 513-atom chain, T4 lysozyme
(grappa_amd/data/t4_lysozyme.npz with mbondi2 radii from its elements) and the 50,046-atom chain; the pool and the chains carry carbon's
radius and screening factor on every atom.  Every size is a child process of its own under `timeout`; after one that fails nothing more
is started.

    python tools/relax_steps_bench.py [--out profiles/relax_steps_bench.txt] [--steps 128] [--big-steps 16] [--reps 5]
    python tools/relax_steps_bench.py --implicit-solvent obc2 [--out profiles/relax_steps_gb_bench.txt]
    python tools/relax_steps_bench.py --cutoff 10 [--switch 8] [--out profiles/relax_steps_cutoff_bench.txt]
    python tools/relax_steps_bench.py --dry          # build the inputs on the CPU and stop (a rehearsal: nothing is timed)
"""
import argparse
import datetime
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nonbonded_bench import chain      # noqa: E402
from relax_bench import Composed, pool_batch      # noqa: E402
from grappa_amd.relax import RELAX_DEFAULTS      # noqa: E402


def chain_graph(n_atoms):
    """-> (single-molecule graph with k / eq at the tuple levels and xyz (n, 1, 3), NonbondedParameters), on the host"""
    from grappa_amd import _hostlib
    from grappa_amd.parameters import Parameters
    from grappa_amd.relax import graph_from_parameters
    (nbp,), xyz = chain(n_atoms)
    x = torch.from_numpy(xyz[:, 0, :]).double()
    k = np.arange(n_atoms)
    bonds = np.stack([k[:-1], k[1:]], axis=1)
    angles, propers = (np.asarray(a, dtype=np.int64) for a in _hostlib.enumerate_tuples(bonds))
    angles, propers = angles.reshape(-1, 3), propers.reshape(-1, 4)
    d = x[bonds[:, 0]] - x[bonds[:, 1]]
    u, v = x[angles[:, 0]] - x[angles[:, 1]], x[angles[:, 2]] - x[angles[:, 1]]
    theta = torch.atan2(torch.cross(u, v, dim=-1).norm(dim=-1), (u * v).sum(-1))
    rng = np.random.default_rng(2)
    ks = rng.uniform(-1, 1, size=(propers.shape[0], 3)) * np.array([1.0, 0.5, 0.3])
    p = Parameters(atoms=k, bonds=bonds, bond_k=np.full(len(bonds), 500.0), bond_eq=d.norm(dim=-1).numpy(), angles=angles,
                   angle_k=np.full(len(angles), 100.0), angle_eq=theta.numpy(), propers=propers, proper_ks=np.abs(ks),
                   proper_phases=np.where(ks >= 0, 0.0, np.pi), impropers=None, improper_ks=None, improper_phases=None)
    # start a little off the equilibrium geometry, so that the bonded terms pull as well
    start = xyz + np.random.default_rng(3).normal(0, 0.03, size=xyz.shape).astype(np.float32)
    return graph_from_parameters(p, start.transpose(1, 0, 2)), nbp


def timed_alternately(fns, reps):
    """fns: name -> callable.  One warm-up run each, then `reps` rounds in which every side runs once, each between device events
    -> name -> list of milliseconds"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


CUT_STAGES = ("device", "mid", "big")
CUT_STAGE_LIMIT = 300          # seconds a stage may take
CUT_SIDES = ("all pairs", "cut, prune=1", "cut, prune=0")


def cut_stage(args):
    """one stage of the cutoff measurement in this process -> one JSON line"""
    if not torch.cuda.is_available():
        sys.exit("relax_steps_bench: needs a GPU (there is nothing to time without one)")
    from grappa_amd.backend import get_backend
    from grappa_amd.nonbonded import Cutoff, NonbondedBatch
    from grappa_amd.relax import relax_graph
    be = get_backend()
    if args.stage == "device":
        prop = torch.cuda.get_device_properties(0)
        print(json.dumps({"device": f"{prop.name}, {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, "
                                    f"{prop.total_memory / 2 ** 30:.0f} GiB; library built for {be.lib.grappa_build_arch().decode()}; torch {torch.__version__}"}))
        return
    n_atoms, S = (args.mid_atoms, args.steps) if args.stage == "mid" else (args.big_atoms, args.big_steps)
    gh, nbp = chain_graph(n_atoms)
    g, nb = gh.to("cuda"), NonbondedBatch([nbp]).to("cuda")
    cuts = {"all pairs": None, "cut, prune=1": Cutoff(args.cutoff, args.switch or None, prune=True),
            "cut, prune=0": Cutoff(args.cutoff, args.switch or None, prune=False)}
    sides = {k: (lambda c=c: relax_graph(g, nb, tolerance=0.0, max_steps=S, stepwise=True, **({} if c is None else {"cutoff": c})))
             for k, c in cuts.items()}
    out = {"atoms": n_atoms, "steps": S, "tuples": {lv: int(g.num_nodes(lv)) for lv in ("n2", "n3", "n4")}, "exceptions": int(nb.n_exceptions),
           "ran": {}, "launches": {}}
    res = {}
    for k, fn in sides.items():
        n0 = be.lib.grappa_launch_count(0)
        res[k] = fn()
        torch.cuda.synchronize()
        out["launches"][k] = int(be.lib.grappa_launch_count(0) - n0)
        out["ran"][k] = bool((res[k].steps == S).all()) and bool((res[k].status == 0).all())
    out["prune_bits_equal"] = bool(torch.equal(res["cut, prune=1"].xyz.view(torch.int32), res["cut, prune=0"].xyz.view(torch.int32)))
    out["dx_cut_all_pairs"] = float((res["cut, prune=1"].xyz - res["all pairs"].xyz).abs().max())
    # what the cut energy kernel evaluates at the start coordinates, per work item
    x = g.nodes["n1"].data["xyz"].contiguous()
    plan = be.nonbonded_plan(nb.atom_molptr_host, nb.N, x.shape[1], x.device)
    e, t = torch.empty(nb.B, x.shape[1], device=x.device), {}
    for prune in (True, False):
        t[prune] = torch.zeros(plan[1], dtype=torch.int32, device=x.device)
        be.nonbonded(x, nb.atom_molptr, nb.charge, nb.sigma, nb.epsilon, nb.exc_ptr, nb.exc_atom, nb.exc_qq, nb.exc_sigma, nb.exc_eps, e, None, None,
                     plan=plan, cutoff=Cutoff(args.cutoff, args.switch or None, prune=prune), tiles=t[prune])
    out["items"], out["tiles"], out["all_tiles"] = int(plan[1]), int(t[True].sum()), int(t[False].sum())
    out["ms"] = timed_alternately(sides, args.reps)
    print(json.dumps(out))


GB_STAGES = ("gb_pool", "gb_513", "gb_t4l", "gb_big")
GB_SIDES = ("vacuum", "solvent")


def gb_stage(args):
    """one size of the solvent measurement in this process -> one JSON line"""
    if not torch.cuda.is_available():
        sys.exit("relax_steps_bench: needs a GPU (there is nothing to time without one)")
    from grappa_amd.backend import get_backend
    from grappa_amd.nonbonded import NonbondedBatch
    from grappa_amd.relax import relax_graph
    from grappa_amd.solvent import GBBatch, GBParameters
    be = get_backend()
    S = args.big_steps if args.stage == "gb_big" else args.steps
    if args.stage == "gb_pool":
        g, nb = pool_batch(args.mols, args.confs)
        what = f"pool: {args.mols} molecules, C = {args.confs}"
    elif args.stage == "gb_t4l":
        from md_steps_bench import _t4l
        gh, nbp, _, gbp = _t4l()
        g, nb = gh.to("cuda"), NonbondedBatch([nbp]).to("cuda")
        what = "T4 lysozyme: 1 molecule, C = 1"
    else:
        gh, nbp = chain_graph(513 if args.stage == "gb_513" else args.big_atoms)
        g, nb = gh.to("cuda"), NonbondedBatch([nbp]).to("cuda")
        what = "chain: 1 molecule, C = 1"
    counts = [int(c) for c in g.batch_num_nodes_host("n1")]
    gbs = [gbp] if args.stage == "gb_t4l" else [GBParameters(np.full(n, 1.7), np.full(n, 0.72)) for n in counts]
    gbb = GBBatch(gbs).to("cuda")
    sides = {"vacuum": lambda: relax_graph(g, nb, tolerance=0.0, max_steps=S, stepwise=True),
             "solvent": lambda: relax_graph(g, nb, tolerance=0.0, max_steps=S, stepwise=True, implicit_solvent=args.implicit_solvent, gb=gbb)}
    out = {"what": what, "atoms": int(sum(counts)), "steps": S, "ran": {}, "launches": {}}
    for k, fn in sides.items():
        n0 = be.lib.grappa_launch_count(0)
        r = fn()
        torch.cuda.synchronize()
        out["launches"][k] = int(be.lib.grappa_launch_count(0) - n0)
        out["ran"][k] = bool((r.steps == S).all()) and bool((r.status == 0).all())
    out["ms"] = timed_alternately(sides, args.reps)
    print(json.dumps(out))


def gb_main(args):
    """the solvent measurement: every size a child process under its own time limit"""
    lines = [f"# command: python {' '.join(sys.argv)}",
             f"# date: {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def run(name):
        cmd = ["timeout", "-k", "10", str(CUT_STAGE_LIMIT), sys.executable, os.path.abspath(__file__), "--stage", name] + \
              [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("mols", "confs", "big_atoms", "steps", "big_steps", "reps", "implicit_solvent")]
        p = subprocess.run(cmd, capture_output=True, text=True)          # (waits for the child: one GPU process at a time)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"relax_steps_bench: stage {name} ended with status {p.returncode}; nothing more is started")
        return json.loads(p.stdout.strip().splitlines()[-1])

    say(f"# device: {run('device')['device']}")
    say(f"# relax_graph(stepwise=True), tolerance 0, a fixed step count: all pairs in vacuum against GB/SA {args.implicit_solvent} on the same tree; "
        f"device events around whole runs, the two sides of a size timed alternately in one process of its own, {args.reps} runs each after one "
        "warm-up run each; all run times in ms; this file is the tool's output, unedited")
    for name in GB_STAGES:
        r = run(name)
        S = r["steps"]
        say(f"{r['what']}, {r['atoms']} atoms, bonded + nonbonded, {S} steps")
        per = {}
        for k in GB_SIDES:
            ms = np.array(r["ms"][k])
            per[k] = float(np.median(ms)) / S
            say(f"  {k:8s} {per[k]:9.4f} ms/step (min {ms.min() / S:9.4f} .. max {ms.max() / S:9.4f})  run {np.median(ms):9.2f} ms  "
                f"{r['launches'][k]} library launches per run; all items ran {S} steps: {r['ran'][k]}")
            say(f"           runs: {', '.join(f'{m:.2f}' for m in ms)} ms")
        say(f"  solvent / vacuum = {per['solvent'] / per['vacuum']:.2f}x ms per step")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def cut_main(args):
    """the cutoff measurement: every stage a child process under its own time limit"""
    lines = [f"# command: python {' '.join(sys.argv)}",
             f"# date: {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def run(name):
        cmd = ["timeout", "-k", "10", str(CUT_STAGE_LIMIT), sys.executable, os.path.abspath(__file__), "--stage", name] + \
              [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("mid_atoms", "big_atoms", "steps", "big_steps", "reps", "cutoff", "switch")]
        p = subprocess.run(cmd, capture_output=True, text=True)          # (waits for the child: one GPU process at a time)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"relax_steps_bench: stage {name} ended with status {p.returncode}; nothing more is started")
        return json.loads(p.stdout.strip().splitlines()[-1])

    say(f"# device: {run('device')['device']}")
    say(f"# relax_graph(stepwise=True), tolerance 0, a fixed step count; cutoff {args.cutoff} A, switch {args.switch or 'none'}, reaction field 78.3; "
        f"device events around whole runs, the three sides of a size timed alternately in one process of its own, {args.reps} runs each after one "
        "warm-up run each; all run times in ms; tiles: evaluated by the cut energy kernel at the start coordinates, summed over its work items; "
        "this file is the tool's output, unedited")
    for name in ("mid", "big"):
        r = run(name)
        S = r["steps"]
        say(f"chain: 1 molecule, {r['atoms']} atoms, C = 1, {', '.join(f'{lv} {n}' for lv, n in r['tuples'].items())}, {r['exceptions']} exceptions, "
            f"bonded + nonbonded, {S} steps")
        per = {}
        for k in CUT_SIDES:
            ms = np.array(r["ms"][k])
            per[k] = float(np.median(ms)) / S
            say(f"  {k:13s} {per[k]:9.4f} ms/step (min {ms.min() / S:9.4f} .. max {ms.max() / S:9.4f})  run {np.median(ms):9.2f} ms  "
                f"{r['launches'][k]} library launches per run; all items ran {S} steps: {r['ran'][k]}")
            say(f"                runs: {', '.join(f'{m:.2f}' for m in ms)} ms")
        say(f"  tiles: {r['tiles']} of {r['all_tiles']} evaluated over {r['items']} work items: mean {r['tiles'] / max(r['items'], 1):.2f} of "
            f"{r['all_tiles'] / max(r['items'], 1):.2f} per item ({100.0 * r['tiles'] / max(r['all_tiles'], 1):.1f} %)")
        say(f"  prune=1 and prune=0 end at the same bits: {r['prune_bits_equal']}; largest |x_cut - x_all pairs| after {S} steps = {r['dx_cut_all_pairs']:.3e} A")
        slow, fast = max(r["ms"]["cut, prune=1"]), min(r["ms"]["all pairs"])
        say(f"  all pairs / cut, prune=1 = {per['all pairs'] / per['cut, prune=1']:.2f}x ms per step; cut, prune=0 / all pairs = "
            f"{per['cut, prune=0'] / per['all pairs']:.2f}x; slowest pruned run {slow:.2f} ms, fastest all-pairs run {fast:.2f} ms: "
            f"{'faster' if slow < fast else 'NOT faster'}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mols", type=int, default=256)
    ap.add_argument("--confs", type=int, default=32)
    ap.add_argument("--mid-atoms", type=int, default=2600)
    ap.add_argument("--big-atoms", type=int, default=50046)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--big-steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--cutoff", type=float, default=0.0, help="A; > 0: measure the nonbonded cutoff (see the module text)")
    ap.add_argument("--switch", type=float, default=0.0, help="A; the switch distance of the cutoff (0: none)")
    ap.add_argument("--implicit-solvent", default="", help="obc2 or obc1: measure the GB/SA implicit solvent (see the module text)")
    ap.add_argument("--stage", default=None, choices=CUT_STAGES + GB_STAGES)
    args = ap.parse_args()
    if args.stage in GB_STAGES:
        return gb_stage(args)
    if args.stage:
        return cut_stage(args)
    if args.implicit_solvent and not args.dry:
        return gb_main(args)
    if args.cutoff and not args.dry:
        return cut_main(args)
    if args.dry:
        for n in (args.mid_atoms, args.big_atoms):
            g, nbp = chain_graph(n)
            print(f"chain of {n} atoms: {', '.join(f'{lv} {g.num_nodes(lv)}' for lv in ('n2', 'n3', 'n4', 'n4_improper'))}; "
                  f"{nbp.exception_idx.shape[0]} exceptions")
        return
    if not torch.cuda.is_available():
        sys.exit("relax_steps_bench: needs a GPU (there is nothing to time without one)")
    from grappa_amd.backend import get_backend
    from grappa_amd.nonbonded import NonbondedBatch
    from grappa_amd.relax import CHECK_EVERY_DEFAULT, relax_graph
    be = get_backend()
    prop = torch.cuda.get_device_properties(0)
    lines = [f"# command: python {' '.join(sys.argv)}",
             f"# date: {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}",
             f"# device: {prop.name}, {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, {prop.total_memory / 2 ** 30:.0f} GiB; "
             f"library built for {be.lib.grappa_build_arch().decode()}; torch {torch.__version__}",
             f"# device events around whole runs of a fixed step count (tolerance 0), the sides of a size timed alternately, {args.reps} runs each "
             "after one warm-up run each: ms per step = run time / steps, median (min .. max); this file is the tool's output, unedited"]
    print("\n".join(lines), flush=True)

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def report(size, what, steps, ms, launches=None):
        per = np.array(ms) / steps
        say(f"{size:6s} {what:24s} {steps:4d} steps  {np.median(per):9.4f} ms/step (min {per.min():9.4f} .. max {per.max():9.4f})  "
            f"run {np.median(ms):9.2f} ms" + (f"  {launches} library launches per run" if launches is not None else ""))
        return float(np.median(per))

    def launches_of(fn):
        n0 = be.lib.grappa_launch_count(0)
        fn()
        torch.cuda.synchronize()
        return int(be.lib.grappa_launch_count(0) - n0)

    def ran(r, steps):
        return f"all items ran {steps} steps: {bool((r.steps == steps).all()) and bool((r.status == 0).all())}"

    opts = {**RELAX_DEFAULTS, "tolerance": 0.0}

    # ---- (a) the pool: fused against stepwise
    g, nb = pool_batch(args.mols, args.confs)
    counts = g.batch_num_nodes_host("n1")
    S = args.steps
    say(f"(a) pool: {args.mols} molecules, {int(counts.sum())} atoms ({int(counts.min())}..{int(counts.max())} per molecule), C = {args.confs}, "
        f"bonded + nonbonded, check_every = {CHECK_EVERY_DEFAULT}")
    sides = {"fused": lambda: relax_graph(g, nb, tolerance=0.0, max_steps=S),
             "stepwise": lambda: relax_graph(g, nb, tolerance=0.0, max_steps=S, stepwise=True)}
    rf, rs_ = sides["fused"](), sides["stepwise"]()
    say(f"pool   fused: {ran(rf, S)}; stepwise: {ran(rs_, S)}; largest |x_fused - x_stepwise| = {float((rf.xyz - rs_.xyz).abs().max()):.3e} A")
    n = {k: launches_of(fn) for k, fn in sides.items()}
    ms = timed_alternately(sides, args.reps)
    pf, ps = report("pool", "fused", S, ms["fused"], n["fused"]), report("pool", "stepwise", S, ms["stepwise"], n["stepwise"])
    say(f"pool   stepwise / fused = {ps / pf:.2f}x ms per step")
    del g, nb

    # ---- (b), (c) the chains: stepwise against composed
    for tag, n_atoms, S, sweep in (("(b)", args.mid_atoms, args.steps, (1, 8, 32, 128)), ("(c)", args.big_atoms, args.big_steps, ())):
        gh, nbp = chain_graph(n_atoms)
        g, nb = gh.to("cuda"), NonbondedBatch([nbp]).to("cuda")
        size = f"{n_atoms}"
        say(f"{tag} chain: 1 molecule, {n_atoms} atoms, C = 1, {', '.join(f'{lv} {g.num_nodes(lv)}' for lv in ('n2', 'n3', 'n4'))}, "
            f"{nb.n_exceptions} exceptions, bonded + nonbonded")
        c = Composed(be, g, nb, opts)          # tables, clones and the nonbonded work-item list: built once, outside the timed region

        def composed(S=S, c=c):
            c.reset()
            for _ in range(S):
                c.step()
        sides = {"stepwise": lambda S=S, g=g, nb=nb: relax_graph(g, nb, tolerance=0.0, max_steps=S, stepwise=True), "composed": composed}
        r = sides["stepwise"]()
        composed()
        say(f"{size:6s} stepwise: {ran(r, S)}; largest |x_stepwise - x_composed| after {S} steps = {float((r.xyz - c.x).abs().max()):.3e} A")
        n = {k: launches_of(fn) for k, fn in sides.items()}
        ms = timed_alternately(sides, args.reps)
        ps = report(size, f"stepwise, check_every {CHECK_EVERY_DEFAULT}", S, ms["stepwise"], n["stepwise"])
        pc = report(size, "composed", S, ms["composed"], n["composed"])
        say(f"{size:6s} composed / stepwise = {pc / ps:.2f}x ms per step (the composed loop also issues its torch ops: not counted as library launches)")
        if sweep:
            sw = {f"check_every {ce}": (lambda ce=ce, S=S, g=g, nb=nb: relax_graph(g, nb, tolerance=0.0, max_steps=S, stepwise=True, check_every=ce))
                  for ce in sweep}
            ms = timed_alternately(sw, args.reps)
            for k in sw:
                report(size, "stepwise, " + k, S, ms[k])
        del g, nb, c
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
