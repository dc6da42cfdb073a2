"""Time the stepwise Langevin dynamics (csrc/dynamics_steps.hip through simulate_graph(stepwise=True)) with device events, after
warm-up, in steps per second, against (a) the fused kernel (csrc/dynamics.hip) where it applies and (c) the same BAOAB step composed
from the entry points that existed before either (tools/md_bench.py Composed: mm_gradient_fwd, the planned nonbonded kernel and an
update in stock torch ops), at three workloads:

  pool    256 molecules of the pool x 32 conformations (tools/relax_bench.py pool_batch): fused, stepwise and composed -- what
          stepwise=True costs where it is not needed; also the coordinate difference between fused and stepwise after 50 steps
          without thermostat (per item the farthest atom: median, 99th percentile, largest)
  513     one synthetic chain of 513 atoms (tools/relax_steps_bench.py chain_graph), 1 conformation -- one atom above the fused limit:
          stepwise and composed
  50046   the 50,046-atom chain of tools/nonbonded_bench.py, 1 conformation: stepwise and composed

No rate is fixed here: the tool reports stepwise against fused and composed of the same run.  Every stage that touches the GPU is a
child process of its own under a time limit; the parent never initialises the GPU, stops at the first stage that fails and starts
nothing after it; at most one GPU process runs at a time.

    python tools/md_steps_bench.py [--out profiles/md_steps_bench.txt] [--steps 500] [--big-steps 20] [--composed-steps 50]

With --cutoff RC [--switch RS] the tool measures the nonbonded cutoff instead (same protocol: device events, one warm-up run, five timed
runs, every GPU stage a child process under its own time limit).  Per workload, in the same visit: the stepwise path with all pairs,
with the cutoff and tile pruning (prune = 1), with the cutoff and every tile evaluated (prune = 0: what the per-pair test alone costs),
and the tiles the cut energy kernel evaluates per work item at the start coordinates against all tiles.  All five times of each side are
printed: the acceptance on the 50,046-atom graph is "the slowest pruned run is faster than the fastest all-pairs run".

    python tools/md_steps_bench.py --cutoff 10 [--switch 8] [--out profiles/md_steps_cutoff_bench.txt]

With --constraints the tool measures X-H constraints on the stepwise path instead (same protocol): on the 513-atom and the 50,046-atom
workload, all pairs and under a cutoff of --cutoff (default 9) A, the unconstrained stepwise run at 1 fs -- the yardstick, whose kernels
this option does not touch -- against the constrained run at 2 fs and at 1 fs.  The workloads are the tool's chains with every second
atom made the leaf of the atom before it, held at their bond's equilibrium length: half the atoms are leaves, as in a protein, though
all in one-leaf clusters (a chain has no XH2 or XH3).  The leaves keep the chain's mass (--leaf-mass gives them another): an atom of
1.008 amu INSIDE this synthetic backbone, with a second bond that is not constrained, stops the items within a few steps, and a stopped
item is skipped by every later launch, so its time is not a rate.  It reports atoms, clusters, statuses, the item steps that were run
and the time per step, constrained over unconstrained: below 2 -- the ratio of the time steps -- constraints pay.  A side whose items
stopped early is marked: its time per step counts launches that did nothing.

    python tools/md_steps_bench.py --constraints [--cutoff 9] [--out profiles/md_steps_cons_bench.txt]

With --implicit-solvent MODEL (obc2, obc1) the tool measures the GB/SA implicit solvent on the stepwise path instead (same protocol):
per workload, in the same visit, the all-pairs vacuum step of this tree against the same run with the solvent (every atom with carbon's
radius 1.7 A and scale 0.72: the cost does not depend on the values), all five times of each side, the ratio of the times per step
and the library launches.  This mode has a fourth workload, t4l: T4 lysozyme (grappa_amd/data/t4_lysozyme.npz: 2,634 atoms with their
elements, bonds, template charges and coordinates), bonded parameters made the way the chains' are (bonds and angles at rest in the
structure, random small torsions), Lennard-Jones parameters by element, and the mbondi2 radii and OBC scales of its elements.

    python tools/md_steps_bench.py --implicit-solvent obc2 [--out profiles/md_steps_gb_bench.txt]
With --gb-cutoff R beside it the solvent step is also measured under the solvent's own cutoff (`ImplicitSolvent(cutoff=R)`, the
grappa_md_steps_*_gbcut_f32 calls): prune = 1 and prune = 0, with --cutoff RC [--switch RS] also with the nonbonded cutoff
`Cutoff(RC, RS, 1.0)` beside it, and the tiles the solvent's energy entry evaluates at the start coordinates:
    python tools/md_steps_bench.py --implicit-solvent obc2 --gb-cutoff 10 [--cutoff 10] [--out profiles/md_steps_gb_cut_bench.txt]

With --restraints the tool measures restraints on the stepwise path instead (`simulate_graph(restraints=)`, the
grappa_md_steps_*_restr_f32 calls): on the 513-atom chain, T4 lysozyme and the 50,046-atom chain, a tether of 10 kcal/mol/A^2 on every
heavy atom and one restrained dihedral (on T4 lysozyme its first proper, on the chains the proper whose two angles are farthest from
straight; 239 kcal/mol, target 0.5 rad from the start) against the same run
without restraints -- whose kernels this option does not touch -- IN THE SAME PROCESS, the two sides alternating run by run after one
warm-up run of each.  All times of each side, the ratio of the medians and the library launches.  It is not a gate: no target is set.

    python tools/md_steps_bench.py --restraints [--out profiles/md_steps_restr_bench.txt]

With --replicas C [--exchange-every K] the tool measures temperature ladders on the stepwise path instead (`simulate_graph(replicas=)`,
the grappa_md_remd_*_f32 calls): on the 513-atom chain and T4 lysozyme, each with its start coordinates in C conformations, the scalar
run of the C conformations -- whose kernels this option does not touch -- against the same run on a ladder of C temperatures from 300 K
up in steps of 10 K without exchanges and, with K > 0, with an attempt every K steps, IN THE SAME PROCESS, the sides alternating run by
run after one warm-up run of each.  All times of each side, the ratios of the medians, the library launches and the accepted swaps.
It is not a gate: no target is set.

    python tools/md_steps_bench.py --replicas 8 --exchange-every 100 [--out profiles/md_steps_remd_bench.txt]
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

from md_bench import OPTS, Composed, _batch, _timed      # noqa: E402

WORKLOADS = ("pool", "mid", "big")
SIDES = {"pool": ("fused", "stepwise", "composed", "agreement"), "mid": ("stepwise", "composed"), "big": ("stepwise", "composed")}
CUT_SIDES = ("stepwise", "cut", "cut_noprune", "tiles")
GB_SIDES = ("stepwise", "gb")
GB_WORKLOADS = ("pool", "mid", "t4l", "big")
GBCUT_SIDES = ("gbcut", "gbcut_noprune", "gbboth")          # the solvent under its own cutoff; gbboth: with the nonbonded cutoff beside it
CONS_SIDES = ("free_1fs", "cons_2fs", "cons_1fs")
CONS_DT = {"free_1fs": 0.001, "cons_2fs": 0.002, "cons_1fs": 0.001}
RESTR_WORKLOADS = ("mid", "t4l", "big")
RESTR_POS_K, RESTR_DIH_K, RESTR_DIH_SHIFT = 10.0, 239.0, 0.5
REMD_WORKLOADS = ("mid", "t4l")
REMD_T0, REMD_DT = 300.0, 10.0
STAGES = ["device", "t4l:stepwise", "t4l:gb"] + [f"{w}:remd" for w in REMD_WORKLOADS] + [f"{w}:restr" for w in RESTR_WORKLOADS] + [f"{w}:{s}" for w in GB_WORKLOADS for s in GBCUT_SIDES + ("gbtiles",)] + [f"{w}:{s}" for w in WORKLOADS for s in SIDES[w] + CUT_SIDES[1:] + GB_SIDES[1:]] + \
         [f"{w}:{s}:{p}" for w in WORKLOADS[1:] for s in CONS_SIDES for p in ("pairs", "cut")]

STAGE_LIMIT = 300      # seconds, every stage
AGREEMENT_STEPS = 50
CARBON = 12.011


def _workload(args, which):
    """-> (graph on the device, NonbondedBatch on the device, masses (N,) float32 on the host, conformations, steps of a timed run)"""
    import numpy as np
    if which == "pool":
        g, nb, masses = _batch(args)
        return g, nb, masses, args.confs, args.steps
    from relax_steps_bench import chain_graph
    from grappa_amd.nonbonded import NonbondedBatch
    if which == "t4l":
        gh, nbp, masses, _ = _t4l()
        return gh.to("cuda"), NonbondedBatch([nbp]).to("cuda"), masses, 1, args.steps
    n = args.mid_atoms if which == "mid" else args.big_atoms
    gh, nbp = chain_graph(n)
    return gh.to("cuda"), NonbondedBatch([nbp]).to("cuda"), np.full(n, CARBON, dtype=np.float32), 1, args.steps if which == "mid" else args.big_steps


def _t4l():
    """T4 lysozyme -> (graph with k / eq at the tuple levels and xyz (n, 1, 3), NonbondedParameters, masses, GBParameters), on the host"""
    import numpy as np
    import torch
    from grappa_amd import _hostlib, constants
    from grappa_amd.datasets import _T4_PATH
    from grappa_amd.nonbonded import NonbondedParameters
    from grappa_amd.parameters import Parameters
    from grappa_amd.relax import graph_from_parameters
    from grappa_amd.solvent import GBParameters
    d = np.load(_T4_PATH)
    z, bonds, xyz = d["z"].astype(np.int64), d["bonds"].astype(np.int64).reshape(-1, 2), d["xyz"].astype(np.float64)
    angles, propers = (np.asarray(a, dtype=np.int64) for a in _hostlib.enumerate_tuples(bonds))
    angles, propers = angles.reshape(-1, 3), propers.reshape(-1, 4)
    x = torch.from_numpy(xyz)
    u, v = x[angles[:, 0]] - x[angles[:, 1]], x[angles[:, 2]] - x[angles[:, 1]]
    theta = torch.atan2(torch.cross(u, v, dim=-1).norm(dim=-1), (u * v).sum(-1))
    ks = np.random.default_rng(2).uniform(-1, 1, size=(propers.shape[0], 3)) * np.array([1.0, 0.5, 0.3])
    p = Parameters(atoms=np.arange(len(z)), bonds=bonds, bond_k=np.full(len(bonds), 500.0), bond_eq=(x[bonds[:, 0]] - x[bonds[:, 1]]).norm(dim=-1).numpy(),
                   angles=angles, angle_k=np.full(len(angles), 100.0), angle_eq=theta.numpy(), propers=propers, proper_ks=np.abs(ks),
                   proper_phases=np.where(ks >= 0, 0.0, np.pi), impropers=None, improper_ks=None, improper_phases=None)
    nbp = NonbondedParameters.from_bonds(bonds, d["charges"].astype(np.float64), np.where(z == 1, 1.1, 3.3), np.where(z == 1, 0.016, 0.1))
    masses = np.array([constants.ATOMIC_MASSES[int(a)] for a in z], dtype=np.float32)
    return graph_from_parameters(p, xyz[None].astype(np.float32)), nbp, masses, GBParameters.from_elements(z, bonds)


def _leaves(n, leaf_mass):
    """every second atom of the n-atom chain a leaf held to the atom before it at the bond's equilibrium length
    -> (masses (n,) float32, Constraints)"""
    import numpy as np
    from relax_steps_bench import chain
    from grappa_amd.constraints import MAX_LEAVES, Constraints
    _, xyz = chain(n)
    x = xyz[:, 0, :].astype(np.float64)
    centre = np.arange(0, n - 1, 2)
    clusters = np.full((centre.size, MAX_LEAVES + 1), -1, dtype=np.int32)
    clusters[:, 0], clusters[:, 1] = centre, centre + 1
    lengths = np.zeros((centre.size, MAX_LEAVES), dtype=np.float32)
    lengths[:, 0] = np.linalg.norm(x[centre + 1] - x[centre], axis=-1)          # chain_graph's bond_eq
    masses = np.full(n, CARBON, dtype=np.float32)
    masses[centre + 1] = leaf_mass
    return masses, Constraints(clusters, lengths)


def _restraints(g, which, n):
    """a tether on every heavy atom and one restrained dihedral (the first proper) of the workload's one molecule -> RestraintBatch (host)"""
    import numpy as np
    from grappa_amd.restraints import RestraintBatch, Restraints, dihedral_angle
    x = g.nodes["n1"].data["xyz"][:, 0].double().cpu().numpy()
    if which == "t4l":
        from grappa_amd import _hostlib
        from grappa_amd.datasets import _T4_PATH
        d = np.load(_T4_PATH)
        heavy = d["z"].astype(np.int64) > 1
        row = np.asarray(_hostlib.enumerate_tuples(d["bonds"].astype(np.int64).reshape(-1, 2))[1], dtype=np.int64).reshape(-1, 4)[0]
    else:
        # a chain of carbons: four consecutive atoms are a proper.  Most of the chain is nearly straight, where a dihedral is ill
        # defined (dphi/dx grows as 1 / sin of the two angles: a restraint there is stiff beyond what a 1 fs step resolves), so the
        # proper with the two angles farthest from 180 degrees among the first 2000 atoms is taken
        m = min(n, 2000)
        u, v = x[:m - 2] - x[1:m - 1], x[2:m] - x[1:m - 1]
        s = np.linalg.norm(np.cross(u, v), axis=1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1))
        first = int(np.minimum(s[:-1], s[1:]).argmax())
        heavy, row = np.ones(n, dtype=bool), np.arange(first, first + 4)
    target = dihedral_angle(x, *[int(a) for a in row]) + RESTR_DIH_SHIFT
    res = Restraints(position_k=np.where(heavy, RESTR_POS_K, 0.0), dihedrals=[row], dihedral_k=[RESTR_DIH_K],
                     dihedral_targets=[(target + np.pi) % (2 * np.pi) - np.pi])
    return RestraintBatch([res], 1, atom_counts=[n]), int(heavy.sum())


def _alternating(fns, reps):
    """one warm-up run of each side, then `reps` rounds in which the sides run one after the other, device events around each whole run
    -> the times of each side in us"""
    import torch
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3)
    return us


def _all_timed(fn, reps):
    """md_bench._timed's protocol (one warm-up run, device events around whole runs), every time kept"""
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
    return us


def stage(args):
    """one GPU stage in this (child) process -> a JSON line on stdout"""
    import torch
    if not torch.cuda.is_available():
        sys.exit("md_steps_bench: needs a GPU (there is nothing to time without one)")
    from grappa_amd.backend import get_backend
    from grappa_amd.dynamics import simulate_graph
    be = get_backend()
    if args.stage == "device":
        prop = torch.cuda.get_device_properties(0)
        print(json.dumps({"device": f"{prop.name}, {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, "
                                    f"{prop.total_memory / 2 ** 30:.0f} GiB; library built for {be.lib.grappa_build_arch().decode()}; torch {torch.__version__}"}))
        return
    which, side, pairs = (args.stage.split(":") + [None])[:3]
    g, nb, masses, confs, steps = _workload(args, which)
    counts = g.batch_num_nodes_host("n1")
    out = {"molecules": len(counts), "atoms": int(counts.sum()), "smallest": int(counts.min()), "largest": int(counts.max()), "confs": confs}
    sim = lambda n, stepwise, **kw: simulate_graph(g, masses, nb, n_steps=n, steps_per_launch=args.steps_per_launch, stepwise=stepwise,      # noqa: E731
                                                   **{**OPTS, **kw})
    if side == "remd":
        import numpy as np
        from grappa_amd.replica import ReplicaExchange
        C, K = args.replicas, args.exchange_every
        g.nodes["n1"].data["xyz"] = g.nodes["n1"].data["xyz"][:, :1].expand(-1, C, -1).contiguous()          # the start in C conformations
        T = REMD_T0 + REMD_DT * np.arange(C)
        sides = [("plain", lambda: sim(steps, True)), ("ladder", lambda: sim(steps, True, replicas=ReplicaExchange(T)))]
        if K > 0:
            sides.append(("exchange", lambda: sim(steps, True, replicas=ReplicaExchange(T, K))))
        for key, fn in sides:
            n0 = be.lib.grappa_launch_count(0)
            r = fn()
            torch.cuda.synchronize()
            out[key] = {"launches": int(be.lib.grappa_launch_count(0) - n0), "item_steps": int(r.steps.sum()), "stopped": int((r.status != 0).sum())}
        if K > 0:
            xs = torch.cat([torch.arange(C, dtype=torch.int32, device=r.exchange_slots.device).expand(1, len(counts), C), r.exchange_slots])
            out["attempts"], out["swapped"] = int(r.exchange_slots.shape[0]), int((xs[1:] != xs[:-1]).sum()) // 2
        for (key, _), us in zip(sides, _alternating([fn for _, fn in sides], args.reps)):
            out[key]["all_us"], out[key]["median_us"] = us, float(sorted(us)[len(us) // 2])
        out["steps"], out["confs"], out["sides"] = steps, C, [k for k, _ in sides]
        print(json.dumps(out))
        return
    if side == "restr":
        rb, tethered = _restraints(g, which, int(counts[0]))
        rb = rb.to("cuda")
        runs = (lambda: sim(steps, True), lambda: sim(steps, True, restraints=rb))
        for key, fn in zip(("plain", "restr"), runs):
            n0 = be.lib.grappa_launch_count(0)
            r = fn()
            torch.cuda.synchronize()
            out[key] = {"launches": int(be.lib.grappa_launch_count(0) - n0), "item_steps": int(r.steps.sum()), "stopped": int((r.status != 0).sum())}
        out["restraint_energy"] = float(r.restraint_energy.sum())
        for key, us in zip(("plain", "restr"), _alternating(runs, args.reps)):
            out[key]["all_us"], out[key]["median_us"] = us, float(sorted(us)[len(us) // 2])
        out["steps"], out["tethered"] = steps, tethered
        print(json.dumps(out))
        return
    if side in CONS_SIDES:
        from grappa_amd.constraints import ConstraintBatch
        from grappa_amd.nonbonded import Cutoff
        masses, cons = _leaves(int(counts[0]), args.leaf_mass)
        kw = {"dt": CONS_DT[side]}
        if pairs == "cut":
            kw["cutoff"] = Cutoff(args.cutoff or 9.0, args.switch or None)
        if side != "free_1fs":
            kw["constraints"] = ConstraintBatch([cons])
        run = lambda: simulate_graph(g, masses, nb, n_steps=steps, steps_per_launch=args.steps_per_launch, stepwise=True, **{**OPTS, **kw})      # noqa: E731
        n0 = be.lib.grappa_launch_count(0)
        r = run()
        torch.cuda.synchronize()
        out["launches"], out["steps"], out["clusters"] = int(be.lib.grappa_launch_count(0) - n0), steps, cons.n_clusters if side != "free_1fs" else 0
        out["item_steps"], out["statuses"] = int(r.steps.sum()), sorted(set(r.status.flatten().tolist()))
        out["all_us"] = _all_timed(run, args.reps)
        out["median_us"], out["min_us"] = float(sorted(out["all_us"])[len(out["all_us"]) // 2]), min(out["all_us"])
        print(json.dumps(out))
        return
    if side in ("cut", "cut_noprune", "tiles"):
        from grappa_amd.nonbonded import Cutoff
        cut = Cutoff(args.cutoff, args.switch or None, prune=side != "cut_noprune")
    if side == "tiles":          # what the cut energy kernel evaluates at the start coordinates, per work item
        x = g.nodes["n1"].data["xyz"].contiguous()
        plan = be.nonbonded_plan(nb.atom_molptr_host, nb.N, x.shape[1], x.device)
        e = torch.empty(nb.B, x.shape[1], device=x.device)
        t = {}
        for prune in (True, False):
            t[prune] = torch.zeros(plan[1], dtype=torch.int32, device=x.device)
            be.nonbonded(x, nb.atom_molptr, nb.charge, nb.sigma, nb.epsilon, nb.exc_ptr, nb.exc_atom, nb.exc_qq, nb.exc_sigma, nb.exc_eps, e, None, None,
                         plan=plan, cutoff=Cutoff(args.cutoff, args.switch or None, prune=prune), tiles=t[prune])
        out["items"], out["tiles"], out["all_tiles"] = int(plan[1]), int(t[True].sum()), int(t[False].sum())
    elif side == "gbtiles":          # what the solvent's cut energy entry evaluates at the start coordinates, per work item
        import numpy as np
        from grappa_amd.solvent import GBBatch, GBParameters, ImplicitSolvent
        gbb = GBBatch([_t4l()[3]] if which == "t4l" else [GBParameters(np.full(int(n), 1.7), np.full(int(n), 0.72)) for n in counts]).to("cuda")
        x = g.nodes["n1"].data["xyz"].contiguous()
        t = {p: gbb.evaluate(nb, x, ImplicitSolvent(args.implicit_solvent, cutoff=args.gb_cutoff, prune=p), gradient=False, tiles=True)["tiles"]
             for p in (True, False)}
        out["items"], out["tiles"], out["all_tiles"] = int(t[True].numel()), int(t[True].sum()), int(t[False].sum())
    elif side in ("fused", "stepwise", "cut", "cut_noprune", "gb") + GBCUT_SIDES:
        sw = side != "fused"
        if side.startswith("cut"):
            plain = sim
            sim = lambda n, stepwise, **kw: plain(n, stepwise, cutoff=cut, **kw)      # noqa: E731
        if side == "gb" or side in GBCUT_SIDES:
            import numpy as np
            from grappa_amd.solvent import GBBatch, GBParameters, ImplicitSolvent
            gbb = GBBatch([_t4l()[3]] if which == "t4l" else [GBParameters(np.full(int(n), 1.7), np.full(int(n), 0.72)) for n in counts]).to("cuda")
            plain = sim
            sv, more = args.implicit_solvent, {}
            if side in GBCUT_SIDES:
                sv = ImplicitSolvent(args.implicit_solvent, cutoff=args.gb_cutoff, prune=side != "gbcut_noprune")
            if side == "gbboth":          # the nonbonded cutoff beside it, reaction-field dielectric 1: OpenMM's companion of GB
                from grappa_amd.nonbonded import Cutoff
                more = {"cutoff": Cutoff(args.cutoff, args.switch or None, 1.0)}
            sim = lambda n, stepwise, **kw: plain(n, stepwise, implicit_solvent=sv, gb=gbb, **more, **kw)      # noqa: E731
        n0 = be.lib.grappa_launch_count(0)
        r = sim(steps, sw)
        torch.cuda.synchronize()
        out["launches"], out["steps"] = int(be.lib.grappa_launch_count(0) - n0), steps
        # (an item that meets a non-finite gradient stops early: the rate counts the steps that were run)
        out["item_steps"], out["stopped"] = int(r.steps.sum()), int((r.status != 0).sum())
        out["median_us"], out["min_us"] = _timed(lambda: sim(steps, sw), args.reps)
        if args.cutoff or args.implicit_solvent:          # every run of the five: the acceptance compares the slowest of one side with the fastest of another
            out["all_us"] = _all_timed(lambda: sim(steps, sw), args.reps)
            out["median_us"], out["min_us"] = float(sorted(out["all_us"])[len(out["all_us"]) // 2]), min(out["all_us"])
    elif side == "composed":
        c = Composed(be, g, nb, masses, OPTS["friction"])          # tables, clones and the nonbonded work-item list: outside the timed region
        v0 = sim(0, True).velocities

        def composed():
            c.reset(v0)
            for _ in range(args.composed_steps):
                c.step()
        n0 = be.lib.grappa_launch_count(0)
        composed()
        torch.cuda.synchronize()
        out["launches"], out["steps"] = int(be.lib.grappa_launch_count(0) - n0), args.composed_steps
        out["item_steps"], out["stopped"] = len(counts) * confs * args.composed_steps, 0
        out["median_us"], out["min_us"] = _timed(composed, args.reps)
    else:          # agreement without a thermostat (with one the two paths would still draw the same noise, but diverge faster)
        v0 = sim(0, True, friction=0.0).velocities
        a, b = (sim(AGREEMENT_STEPS, s, velocities=v0, friction=0.0) for s in (False, True))
        atom_mol = torch.repeat_interleave(torch.arange(len(counts)), torch.as_tensor(counts, dtype=torch.long)).to(a.xyz.device)
        both = (a.status == 0) & (b.status == 0)          # (B, C): items that ran all steps on both paths
        d = torch.zeros_like(a.potential_energy).index_reduce_(0, atom_mol, (a.xyz - b.xyz).abs().amax(-1), "amax", include_self=True)[both]
        # per item, the farthest atom.  The synthetic charges pull some items towards a singularity, where a trajectory amplifies
        # rounding without bound: the largest value describes those items, the quantiles the batch
        q = torch.quantile(d.double(), torch.tensor([0.5, 0.99], dtype=torch.float64, device=d.device))
        out["items"], out["median_dx"], out["p99_dx"], out["max_dx"] = int(d.numel()), float(q[0]), float(q[1]), float(d.max())
        out["above"] = int((d > 1e-3).sum())
        out["steps"], out["differ"] = AGREEMENT_STEPS, int(((a.steps != b.steps) | (a.status != b.status)).sum())
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--mols", type=int, default=256)
    ap.add_argument("--confs", type=int, default=32)
    ap.add_argument("--mid-atoms", type=int, default=513)
    ap.add_argument("--big-atoms", type=int, default=50046)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--big-steps", type=int, default=20)
    ap.add_argument("--steps-per-launch", type=int, default=10000)
    ap.add_argument("--composed-steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cutoff", type=float, default=0.0, help="A; > 0: measure the nonbonded cutoff (see the module text)")
    ap.add_argument("--switch", type=float, default=0.0, help="A; the switch distance of the cutoff (0: none)")
    ap.add_argument("--constraints", action="store_true", help="measure X-H constraints on the stepwise path (see the module text)")
    ap.add_argument("--leaf-mass", type=float, default=CARBON, help="amu; the mass of the leaves with --constraints (the chain's own by default)")
    ap.add_argument("--implicit-solvent", default="", help="obc2 or obc1: measure the GB/SA implicit solvent on the stepwise path (see the module text)")
    ap.add_argument("--gb-cutoff", type=float, default=0.0, help="A; with --implicit-solvent: also measure the solvent under this cutoff of its own")
    ap.add_argument("--restraints", action="store_true", help="measure restraints on the stepwise path (see the module text)")
    ap.add_argument("--replicas", type=int, default=0, help="C > 0: measure a temperature ladder of C slots on the stepwise path (see the module text)")
    ap.add_argument("--exchange-every", type=int, default=0, help="K; with --replicas: also measure an exchange attempt every K steps")
    ap.add_argument("--stage", default=None, choices=STAGES)
    args = ap.parse_args()
    if args.stage:
        return stage(args)
    lines = [f"# command: python {' '.join(sys.argv)}",
             f"# date: {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def run(name):
        cmd = ["timeout", "-k", "10", str(STAGE_LIMIT), sys.executable, os.path.abspath(__file__), "--stage", name] + \
              [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("mols", "confs", "mid_atoms", "big_atoms", "steps", "big_steps", "steps_per_launch",
                                                                      "composed_steps", "reps", "cutoff", "switch", "leaf_mass", "implicit_solvent", "gb_cutoff",
                                                                      "replicas", "exchange_every")]
        p = subprocess.run(cmd, capture_output=True, text=True)          # (waits for the child: one GPU process at a time)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"md_steps_bench: stage {name} ended with status {p.returncode}; nothing more is started")
        return json.loads(p.stdout.strip().splitlines()[-1])

    def report(what, r):
        steps_s = r["steps"] / (r["median_us"] * 1e-6)
        say(f"  {what:10s} {r['steps']:6d} steps {r['median_us'] / 1e3:10.2f} ms (min {r['min_us'] / 1e3:10.2f})  {steps_s:10.1f} steps/s  "
            f"{r['item_steps'] / (r['median_us'] * 1e-6):10.3e} item steps/s  {r['launches']:6d} library launches"
            + (f"  ({r['stopped']} items stopped early)" if r["stopped"] else ""))
        return steps_s

    say(f"# device: {run('device')['device']}")
    say("# device events around whole runs, median (min) after one warm-up run; every stage a process of its own; steps/s = steps of the run / "
        "run time, whatever the batch holds; this file is the tool's output, unedited")
    if args.replicas:
        say(f"# temperature ladders on the stepwise path: C = {args.replicas} conformations of the start, slots at {REMD_T0} K + {REMD_DT} K s, "
            f"exchange attempts every {args.exchange_every or 'never'} steps, against the scalar run of the same conformations, in the same process, "
            "sides alternating; all run times of each side in ms")
        names = {"plain": "scalar", "ladder": "ladder, K = 0", "exchange": f"ladder, K = {args.exchange_every}"}
        for w in REMD_WORKLOADS:
            r = run(f"{w}:remd")
            say(f"{w}: {r['molecules']} molecule(s), {r['atoms']} atoms, C = {r['confs']}, bonded + nonbonded, dt {OPTS['dt']} ps, friction {OPTS['friction']} "
                f"/ ps, {r['steps']} steps" + (f"; {r['attempts']} attempts, {r['swapped']} accepted swaps" if "attempts" in r else ""))
            for key in r["sides"]:
                q = r[key]
                say(f"  {names[key]:16s} {q['median_us'] / r['steps']:10.2f} us / step  {r['steps'] / (q['median_us'] * 1e-6):10.1f} steps/s  {q['launches']:6d} "
                    f"library launches  runs: {', '.join(f'{u / 1e3:.2f}' for u in q['all_us'])} ms" + (f"  ({q['stopped']} items stopped early)" if q["stopped"] else ""))
            say(f"  time per step, ladder / scalar = {r['ladder']['median_us'] / r['plain']['median_us']:.3f}")
            if "exchange" in r:
                extra = (r["exchange"]["median_us"] - r["ladder"]["median_us"]) / max(r["attempts"], 1)
                say(f"  time per step, exchanging / scalar = {r['exchange']['median_us'] / r['plain']['median_us']:.3f}; an attempt costs "
                    f"{extra:.1f} us = {extra / (r['plain']['median_us'] / r['steps']):.2f} scalar steps")
    elif args.restraints:
        say(f"# restraints on the stepwise path: a tether of {RESTR_POS_K} kcal/mol/A^2 on every heavy atom and one restrained dihedral ({RESTR_DIH_K} "
            f"kcal/mol, target {RESTR_DIH_SHIFT} rad from the start) against the same all-pairs run without them, in the same process, sides "
            "alternating; all run times of each side in ms")
        for w in RESTR_WORKLOADS:
            r = run(f"{w}:restr")
            say(f"{w}: {r['molecules']} molecule(s), {r['atoms']} atoms, {r['tethered']} tethered, C = {r['confs']}, bonded + nonbonded, dt {OPTS['dt']} ps, "
                f"{OPTS['temperature']} K, friction {OPTS['friction']} / ps, {r['steps']} steps; E_r at the end {r['restraint_energy']:.2f} kcal/mol")
            for key, what in (("plain", "no restraints"), ("restr", "restraints")):
                q = r[key]
                say(f"  {what:14s} {q['median_us'] / r['steps']:10.2f} us / step  {r['steps'] / (q['median_us'] * 1e-6):10.1f} steps/s  {q['launches']:6d} library "
                    f"launches  runs: {', '.join(f'{u / 1e3:.2f}' for u in q['all_us'])} ms" + (f"  ({q['stopped']} items stopped early)" if q["stopped"] else ""))
            say(f"  time per step, restraints / none = {r['restr']['median_us'] / r['plain']['median_us']:.3f}")
    elif args.constraints:
        args.cutoff = args.cutoff or 9.0
        say(f"# X-H constraints on the stepwise path: every second atom a leaf ({args.leaf_mass} amu) held to the atom before it; cutoff {args.cutoff} A, "
            f"switch {args.switch or 'none'}, reaction field 78.3; {OPTS['temperature']} K, friction {OPTS['friction']} / ps; all run times in ms")
        for w in WORKLOADS[1:]:
            for pairs, what in (("pairs", "all pairs"), ("cut", f"cutoff {args.cutoff} A")):
                res = {side: run(f"{w}:{side}:{pairs}") for side in CONS_SIDES}
                r = res["cons_2fs"]
                say(f"{w}, {what}: {r['atoms']} atoms, {r['clusters']} clusters ({r['clusters']} leaves), C = {r['confs']}")
                per = {}
                for side in CONS_SIDES:
                    q = res[side]
                    per[side] = q["median_us"] / q["steps"]
                    say(f"  {side:9s} dt {CONS_DT[side] * 1e3:.0f} fs {q['steps']:5d} steps  {per[side]:10.2f} us / step  {q['steps'] / (q['median_us'] * 1e-6) * CONS_DT[side] * 1e3 * 86.4e-3:10.3f} ns / day  "
                        f"{q['launches']:6d} library launches  statuses {q['statuses']}  {q['item_steps']} item steps  "
                        f"runs: {', '.join(f'{u / 1e3:.2f}' for u in q['all_us'])}"
                        + ("" if q["item_steps"] == q["steps"] * q["confs"] else "  STOPPED EARLY: not a rate"))
                # a constrained step costs the same at 1 fs and at 2 fs; where the 2 fs run stopped early (its time is not a rate) the
                # 1 fs run, if it ran all its steps, stands for it
                ran = {side: res[side]["item_steps"] == res[side]["steps"] * res[side]["confs"] for side in CONS_SIDES}
                side = "cons_2fs" if ran["cons_2fs"] else "cons_1fs"
                if not (ran[side] and ran["free_1fs"]):
                    say("  time per step, constrained / unconstrained: no ratio, items stopped early on both constrained runs or on the yardstick")
                    continue
                ratio = per[side] / per["free_1fs"]
                say(f"  time per step, constrained ({side}) / unconstrained (1 fs) = {ratio:.3f}: simulated time per wall time at 2 fs {2.0 / ratio:.2f}x "
                    f"({'constraints pay' if ratio < 2.0 else 'constraints do NOT pay'}: the bound is the ratio of the time steps, 2)"
                    + ("" if ran["cons_2fs"] else "; the 2 fs run itself stopped early on this synthetic chain"))
    elif args.cutoff and not args.implicit_solvent:
        say(f"# cutoff {args.cutoff} A, switch {args.switch or 'none'}, reaction field 78.3; all five run times of each side in ms; tiles: evaluated by the cut "
            "energy kernel at the start coordinates, summed over its work items")
        for w in WORKLOADS:
            res = {side: run(f"{w}:{side}") for side in CUT_SIDES}
            r = res["stepwise"]
            say(f"{w}: {r['molecules']} molecule(s), {r['atoms']} atoms ({r['smallest']}..{r['largest']} per molecule), C = {r['confs']}, "
                f"bonded + nonbonded, dt {OPTS['dt']} ps, {OPTS['temperature']} K, friction {OPTS['friction']} / ps")
            rate = {}
            for side, what in (("stepwise", "all pairs"), ("cut", "cut, prune=1"), ("cut_noprune", "cut, prune=0")):
                rate[side] = report(f"{what:12s}", res[side])
                say(f"               runs: {', '.join(f'{u / 1e3:.2f}' for u in res[side]['all_us'])} ms")
            t = res["tiles"]
            say(f"  tiles: {t['tiles']} of {t['all_tiles']} evaluated over {t['items']} work items: mean {t['tiles'] / max(t['items'], 1):.2f} of "
                f"{t['all_tiles'] / max(t['items'], 1):.2f} per item ({100.0 * t['tiles'] / max(t['all_tiles'], 1):.1f} %)")
            say(f"  cut, prune=1 / all pairs = {rate['cut'] / rate['stepwise']:.2f}x steps/s; cut, prune=0 / all pairs = {rate['cut_noprune'] / rate['stepwise']:.2f}x; "
                f"slowest pruned run {max(res['cut']['all_us']) / 1e3:.2f} ms, fastest all-pairs run {min(res['stepwise']['all_us']) / 1e3:.2f} ms: "
                f"{'faster' if max(res['cut']['all_us']) < min(res['stepwise']['all_us']) else 'NOT faster'}")
    if args.implicit_solvent:
        say(f"# GB/SA implicit solvent {args.implicit_solvent} on the stepwise path against the all-pairs vacuum step of the same tree; all five run "
            "times of each side in ms")
        for w in GB_WORKLOADS:
            res = {side: run(f"{w}:{side}") for side in GB_SIDES}
            r = res["stepwise"]
            say(f"{w}: {r['molecules']} molecule(s), {r['atoms']} atoms ({r['smallest']}..{r['largest']} per molecule), C = {r['confs']}, "
                f"bonded + nonbonded, dt {OPTS['dt']} ps, {OPTS['temperature']} K, friction {OPTS['friction']} / ps")
            rate = {}
            for side, what in (("stepwise", "vacuum"), ("gb", args.implicit_solvent)):
                rate[side] = report(f"{what:12s}", res[side])
                say(f"               runs: {', '.join(f'{u / 1e3:.2f}' for u in res[side]['all_us'])} ms")
            say(f"  time per step, {args.implicit_solvent} / vacuum = {rate['stepwise'] / rate['gb']:.2f}")
            if args.gb_cutoff > 0:
                sides = [s_ for s_ in GBCUT_SIDES if s_ != "gbboth" or args.cutoff]
                names = {"gbcut": f"cut {args.gb_cutoff:g} A, prune=1", "gbcut_noprune": f"cut {args.gb_cutoff:g} A, prune=0",
                         "gbboth": f"both cut ({args.cutoff:g} A)"}
                for side in sides:
                    res[side] = run(f"{w}:{side}")
                    rate[side] = report(f"{names[side]:20s}", res[side])
                    say(f"               runs: {', '.join(f'{u / 1e3:.2f}' for u in res[side]['all_us'])} ms")
                t = run(f"{w}:gbtiles")
                say(f"  solvent tiles: {t['tiles']} of {t['all_tiles']} evaluated over {t['items']} work items ({100.0 * t['tiles'] / max(t['all_tiles'], 1):.1f} %)")
                say(f"  steps/s, solvent cut prune=1 / all-pairs solvent = {rate['gbcut'] / rate['gb']:.2f}x; prune=0 / all-pairs solvent = "
                    f"{rate['gbcut_noprune'] / rate['gb']:.2f}x; slowest pruned run {max(res['gbcut']['all_us']) / 1e3:.2f} ms, fastest all-pairs solvent run "
                    f"{min(res['gb']['all_us']) / 1e3:.2f} ms: {'faster' if max(res['gbcut']['all_us']) < min(res['gb']['all_us']) else 'NOT faster'}"
                    + (f"; with the nonbonded cutoff beside it {rate['gbboth'] / rate['gb']:.2f}x" if "gbboth" in rate else ""))
    for w in (() if args.cutoff or args.constraints or args.implicit_solvent or args.restraints or args.replicas else WORKLOADS):
        rate, head = {}, None
        for side in SIDES[w]:
            r = run(f"{w}:{side}")
            if head is None:
                head = (f"{w}: {r['molecules']} molecule(s), {r['atoms']} atoms ({r['smallest']}..{r['largest']} per molecule), C = {r['confs']}, "
                        f"bonded + nonbonded, dt {OPTS['dt']} ps, {OPTS['temperature']} K, friction {OPTS['friction']} / ps")
                say(head)
            if side == "agreement":
                say(f"  after {r['steps']} steps without thermostat, per item the farthest atom |x_fused - x_stepwise| over the {r['items']} items that ran all "
                    f"steps on both paths: median {r['median_dx']:.3e}, 99th percentile {r['p99_dx']:.3e}, largest {r['max_dx']:.3e} A; {r['above']} items "
                    f"above 1e-3 A; {r['differ']} items differ in steps or status")
            else:
                rate[side] = report(side, r)
        if "fused" in rate:
            say(f"  stepwise / fused = {rate['stepwise'] / rate['fused']:.3f}x steps/s")
        say(f"  stepwise / composed = {rate['stepwise'] / rate['composed']:.2f}x steps/s (the composed loop also issues its torch ops: not counted as library launches)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
