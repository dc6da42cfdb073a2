"""Time the nonbonded kernel (csrc/nonbonded.hip through HipBackend.nonbonded) with device events, after warm-up, at two shapes:

  pool    256 molecules of the pool x 32 conformations (a training batch)
  chain   one synthetic 50,046-atom chain, 1 conformation (BASELINE configs[4]'s size: 2.5e9 ordered pairs)

and, at the first shape only (N^2 memory rules out the second), a plain torch broadcast implementation of the same sums on the same GPU.
Rows per shape: the kernel alone (HipBackend.nonbonded into preallocated outputs, work-item list built once on the host), the same call
without the gradient output, with the list built on the device by every call, and NonbondedBatch.evaluate (which also allocates its outputs).
Prints microseconds per call and pair interactions per second; a pair interaction is one evaluated ordered pair (i, j) of one
conformation, sum_b n_b (n_b - 1) C per call -- the kernel evaluates every unordered pair twice, once for each owner, and both count.
The share of the fp32 vector peak uses FLOP_PER_PAIR below (counted from the kernel's inner loop) and 157.3 TFLOP/s.

    python tools/nonbonded_bench.py [--out profiles/nonbonded_bench.txt] [--seconds 1.0]

With --cutoff RC [--switch RS] the tool measures the nonbonded cutoff instead: at three workloads (the pool batch, a 513-atom chain, the
50,046-atom chain) the planned kernel with all pairs, with the cutoff and tile pruning (prune = 1) and with the cutoff and every tile
evaluated (prune = 0: what the per-pair test alone costs), in calls per second, and the tiles evaluated per work item against all tiles.
Device events around single calls, one warm-up call, five timed calls (all five printed, the median reported); every workload is a child
process of its own under a time limit, the parent never initialises the GPU and starts nothing after a stage that fails.

    python tools/nonbonded_bench.py --cutoff 10 [--switch 8] [--out profiles/nb_cutoff_bench.txt]

With --gb MODEL (obc2, obc1) the tool measures the GB/SA implicit solvent (csrc/gb_obc.hip through HipBackend.gb_obc) instead, by the same
protocol at the same three workloads: the planned all-pairs nonbonded kernel (energy, terms, gradient) against the solvent entry with
and without the gradient (every atom with carbon's radius 1.7 A and scale 0.72: the cost does not depend on the values).

    python tools/nonbonded_bench.py --gb obc2 [--out profiles/gb_bench.txt]
With --gb-cutoff R beside it, the solvent is also measured under its own cutoff (`ImplicitSolvent(cutoff=R)`, grappa_gb_obc_fwd_cut_f32):
all pairs against prune = 1 against prune = 0, the three taking turns call by call, with the tiles evaluated out of all tiles:
    python tools/nonbonded_bench.py --gb obc2 --gb-cutoff 10 [--out profiles/gb_cut_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from grappa_amd.constants import COULOMB_CONSTANT      # noqa: E402
from grappa_amd.nonbonded import NonbondedBatch, NonbondedParameters      # noqa: E402

# fp32 operations of one pair in the kernel's loop without the exception lookup (an fma counts 2): 3 sub, r^2 5, rsq 1, Newton step 7,
# y^2 1, sigma / eps / qq of the pair 3, (s/r)^2 .. l12 6, Coulomb 1, two energy sums 3, (dE/dr)/r 6, gradient 6
FLOP_PER_PAIR = 42
PEAK_FP32_VECTOR = 157.3e12


def pool_batch(n_mols, n_confs, seed=0):
    from grappa_amd.datasets import pool_molecule, pool_size
    rng = np.random.default_rng(seed)
    params, xs = [], []
    for k in range(n_mols):
        z, bonds, xyz0 = pool_molecule(k % pool_size())
        n = len(z)
        q = rng.normal(0, 0.3, n)
        params.append(NonbondedParameters.from_bonds(bonds, q - q.mean(), np.where(z == 1, 1.1, 3.3), np.where(z == 1, 0.016, 0.1)))
        xs.append(xyz0[:, None, :] + rng.normal(0, 0.05, size=(n, n_confs, 3)))
    return params, np.concatenate(xs, axis=0).astype(np.float32)


def chain(n_atoms, seed=1):
    """a self-avoiding zigzag on a cubic lattice of 1.5 A, bonded along the chain"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n_atoms ** (1 / 3)))
    k = np.arange(n_atoms)
    x, y, zc = k % side, (k // side) % side, k // (side * side)
    y = np.where(zc % 2 == 1, side - 1 - y, y)
    x = np.where((k // side) % 2 == 1, side - 1 - x, x)      # boustrophedon: consecutive atoms are lattice neighbours
    xyz = 1.5 * np.stack([x, y, zc], axis=1) + rng.uniform(-0.1, 0.1, size=(n_atoms, 3))
    bonds = np.stack([k[:-1], k[1:]], axis=1)
    q = rng.normal(0, 0.3, n_atoms)
    p = NonbondedParameters.from_bonds(bonds, q - q.mean(), rng.uniform(1.0, 2.0, n_atoms), rng.uniform(0.01, 0.1, n_atoms))
    return [p], xyz[:, None, :].astype(np.float32)


def torch_broadcast(nb, pad_idx, pad_mask, xyz):
    """the same sums as padded (B, n, n, C) broadcasts in stock torch ops (exceptions as dense override tables built once, outside the
    timed region)"""
    x = xyz[pad_idx] * pad_mask[:, :, None, None]                      # (B, n, C, 3)
    d = x[:, :, None] - x[:, None, :]                                  # (B, n, n, C, 3)
    m = nb["mask"][..., None]
    r2 = torch.where(m, (d * d).sum(-1), torch.ones((), device=x.device))
    inv = torch.rsqrt(r2)
    sr6 = (nb["sij"][..., None] * inv) ** 6
    l6 = nb["e4"][..., None] * sr6
    l12 = l6 * sr6
    co = nb["kqq"][..., None] * inv
    zero = torch.zeros((), device=x.device)
    energy = 0.5 * torch.where(m, l12 - l6 + co, zero).sum((1, 2))
    f = torch.where(m, (6 * l6 - 12 * l12 - co) * inv * inv, zero)
    grad = (f[..., None] * d).sum(2)
    return energy, grad


def dense_tables(params, device):
    B, n = len(params), max(p.n_atoms for p in params)
    sij, e4, kqq = np.zeros((B, n, n), np.float32), np.zeros((B, n, n), np.float32), np.zeros((B, n, n), np.float32)
    mask = np.zeros((B, n, n), bool)
    pad_idx, pad_mask, o = np.zeros((B, n), np.int64), np.zeros((B, n), np.float32), 0
    for b, p in enumerate(params):
        k = p.n_atoms
        sij[b, :k, :k] = 0.5 * (p.sigma[:, None] + p.sigma[None, :])
        e4[b, :k, :k] = 4 * np.sqrt(p.epsilon[:, None] * p.epsilon[None, :])
        kqq[b, :k, :k] = COULOMB_CONSTANT * p.charge[:, None] * p.charge[None, :]
        mask[b, :k, :k] = ~np.eye(k, dtype=bool)
        i, j = p.exception_idx[:, 0], p.exception_idx[:, 1]
        for a, c in ((i, j), (j, i)):
            sij[b, a, c], e4[b, a, c], kqq[b, a, c] = p.exception_sigma, 4 * p.exception_epsilon, COULOMB_CONSTANT * p.exception_chargeprod
            mask[b, a, c] = ~((p.exception_epsilon == 0) & (p.exception_chargeprod == 0))
        pad_idx[b, :k], pad_mask[b, :k] = np.arange(o, o + k), 1.0
        o += k
    t = lambda a: torch.from_numpy(a).to(device)      # noqa: E731
    return {"sij": t(sij), "e4": t(e4), "kqq": t(kqq), "mask": t(mask)}, t(pad_idx), t(pad_mask)


def time_events(fn, seconds):
    """median and minimum over device-event timings of single calls, after warm-up, for about `seconds` of device time"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(), fn(), b.record()
    torch.cuda.synchronize()
    reps = int(min(max(seconds * 1e3 / max(a.elapsed_time(b), 1e-3), 5), 2000))
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    us = np.array([s.elapsed_time(e) * 1e3 for s, e in ev])
    return float(np.median(us)), float(us.min()), reps


CUT_WORKLOADS = ("pool", "mid", "big")
CUT_STAGE_LIMIT = 300      # seconds, every stage


def five(fn):
    """one warm-up call, then five calls between device events -> the five times in us"""
    fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(), fn(), b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return us


def five_in_turn(fns):
    """one warm-up call each, then five rounds in which the calls take turns, each between device events -> {name: the five times in us}"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(), fn(), b.record()
            torch.cuda.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3)
    return us


def cut_stage(args):
    """one workload of the cutoff measurement in this (child) process -> a JSON line on stdout"""
    if not torch.cuda.is_available():
        sys.exit("nonbonded_bench: needs a GPU (there is nothing to time without one)")
    from grappa_amd.backend import get_backend
    from grappa_amd.nonbonded import Cutoff
    be = get_backend()
    if args.stage == "device":
        prop = torch.cuda.get_device_properties(0)
        print(json.dumps({"device": f"{prop.name}, {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, "
                                    f"{prop.total_memory / 2 ** 30:.0f} GiB; library built for {be.lib.grappa_build_arch().decode()}; torch {torch.__version__}"}))
        return
    params, xyz = pool_batch(args.mols, args.confs) if args.stage == "pool" else chain(args.mid_atoms if args.stage == "mid" else args.chain_atoms)
    nb = NonbondedBatch(params).to("cuda")
    x = torch.from_numpy(xyz).to("cuda")
    n = np.array([p.n_atoms for p in params], dtype=np.float64)
    e_o, t_o, g_o = torch.empty(nb.B, x.shape[1], device="cuda"), torch.empty(2, nb.B, x.shape[1], device="cuda"), torch.empty_like(x)
    tabs = (x, nb.atom_molptr, nb.charge, nb.sigma, nb.epsilon, nb.exc_ptr, nb.exc_atom, nb.exc_qq, nb.exc_sigma, nb.exc_eps)
    plan = be.nonbonded_plan(nb.atom_molptr.cpu(), nb.N, x.shape[1], "cuda")
    if args.gb:
        from grappa_amd.solvent import ImplicitSolvent
        opts = ImplicitSolvent(args.gb).as_opts()
        R, S = torch.full((nb.N,), 1.7, device="cuda"), torch.full((nb.N,), 0.72, device="cuda")
        br = torch.empty(nb.N, x.shape[1], device="cuda")
        out = {"molecules": len(params), "atoms": int(n.sum()), "smallest": int(n.min()), "largest": int(n.max()), "confs": int(x.shape[1]), "items": int(plan[1])}
        n0 = be.lib.grappa_launch_count(0)
        be.gb_obc(x, nb.atom_molptr, nb.charge, R, S, opts, e_o, t_o, g_o, br, plan=plan)
        out["launches"] = int(be.lib.grappa_launch_count(0) - n0)
        out["all_pairs"] = five(lambda: be.nonbonded(*tabs, e_o, t_o, g_o, plan=plan))
        out["gb"] = five(lambda: be.gb_obc(x, nb.atom_molptr, nb.charge, R, S, opts, e_o, t_o, g_o, br, plan=plan))
        out["gb_energy"] = five(lambda: be.gb_obc(x, nb.atom_molptr, nb.charge, R, S, opts, e_o, t_o, None, None, plan=plan))
        out["finite"] = bool(torch.isfinite(e_o).all()) and bool(torch.isfinite(g_o).all())
        if args.gb_cutoff > 0:
            copts = {p: ImplicitSolvent(args.gb, cutoff=args.gb_cutoff, prune=p).cut_opts() for p in (True, False)}
            tiles = {p: torch.zeros(plan[1], dtype=torch.int32, device="cuda") for p in (True, False)}
            call = lambda p: be.gb_obc(x, nb.atom_molptr, nb.charge, R, S, opts, e_o, t_o, g_o, br, plan=plan, cut=copts[p], tiles=tiles[p])      # noqa: E731
            n0 = be.lib.grappa_launch_count(0)
            call(True)
            out["cut_launches"] = int(be.lib.grappa_launch_count(0) - n0)
            out.update(five_in_turn({"turn_all": lambda: be.gb_obc(x, nb.atom_molptr, nb.charge, R, S, opts, e_o, t_o, g_o, br, plan=plan),
                                     "turn_prune": lambda: call(True), "turn_noprune": lambda: call(False)}))
            out["tiles"], out["all_tiles"] = int(tiles[True].sum()), int(tiles[False].sum())
            out["finite"] = out["finite"] and bool(torch.isfinite(e_o).all()) and bool(torch.isfinite(g_o).all())
        print(json.dumps(out))
        return
    cut = {p: Cutoff(args.cutoff, args.switch or None, prune=p) for p in (True, False)}
    tiles = {p: torch.zeros(plan[1], dtype=torch.int32, device="cuda") for p in (True, False)}
    out = {"molecules": len(params), "atoms": int(n.sum()), "smallest": int(n.min()), "largest": int(n.max()), "confs": int(x.shape[1]), "items": int(plan[1])}
    out["all_pairs"] = five(lambda: be.nonbonded(*tabs, e_o, t_o, g_o, plan=plan))
    out["cut"] = five(lambda: be.nonbonded(*tabs, e_o, t_o, g_o, plan=plan, cutoff=cut[True], tiles=tiles[True]))
    out["cut_noprune"] = five(lambda: be.nonbonded(*tabs, e_o, t_o, g_o, plan=plan, cutoff=cut[False], tiles=tiles[False]))
    out["tiles"], out["all_tiles"] = int(tiles[True].sum()), int(tiles[False].sum())
    print(json.dumps(out))


def gb_main(args):
    import datetime
    lines = [f"# command: python {' '.join(sys.argv)}", f"# date: {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def run(name):
        cmd = ["timeout", "-k", "10", str(CUT_STAGE_LIMIT), sys.executable, os.path.abspath(__file__), "--stage", name, f"--gb={args.gb}", f"--gb-cutoff={args.gb_cutoff}",
               f"--mols={args.mols}", f"--confs={args.confs}", f"--mid-atoms={args.mid_atoms}", f"--chain-atoms={args.chain_atoms}"]
        p = subprocess.run(cmd, capture_output=True, text=True)          # (waits for the child: one GPU process at a time)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"nonbonded_bench: stage {name} ended with status {p.returncode}; nothing more is started")
        return json.loads(p.stdout.strip().splitlines()[-1])

    say(f"# device: {run('device')['device']}")
    say(f"# GB/SA implicit solvent {args.gb} against the planned all-pairs nonbonded kernel, both into preallocated outputs; device events around "
        "single calls, one warm-up call, five timed calls: median, all five; every workload a process of its own; this file is the tool's output, unedited")
    for w in CUT_WORKLOADS:
        r = run(w)
        say(f"{w}: {r['molecules']} molecule(s), {r['atoms']} atoms ({r['smallest']}..{r['largest']} per molecule), C = {r['confs']}, {r['items']} work items; "
            f"the solvent call makes {r['launches']} launches; outputs finite: {r['finite']}")
        med = {}
        for key, what in (("all_pairs", "LJ + Coulomb"), ("gb", f"{args.gb}"), ("gb_energy", f"{args.gb}, no gradient")):
            med[key] = float(np.median(r[key]))
            say(f"  {what:20s} {med[key]:12.1f} us  {1e6 / med[key]:10.1f} calls/s   runs: {', '.join(f'{u:.1f}' for u in r[key])} us")
        say(f"  time per call, {args.gb} / LJ + Coulomb = {med['gb'] / med['all_pairs']:.2f}; without the gradient {med['gb_energy'] / med['all_pairs']:.2f}")
        if args.gb_cutoff > 0:
            say(f"  under a solvent cutoff of {args.gb_cutoff:g} A ({r['cut_launches']} launches), the three taking turns; tiles evaluated {r['tiles']} of {r['all_tiles']} "
                f"({100.0 * r['tiles'] / max(r['all_tiles'], 1):.1f} %)")
            for key, what in (("turn_all", f"{args.gb}, all pairs"), ("turn_prune", "cutoff, prune = 1"), ("turn_noprune", "cutoff, prune = 0")):
                med[key] = float(np.median(r[key]))
                say(f"  {what:20s} {med[key]:12.1f} us  {1e6 / med[key]:10.1f} calls/s   runs: {', '.join(f'{u:.1f}' for u in r[key])} us")
            say(f"  all pairs / prune = 1 = {med['turn_all'] / med['turn_prune']:.2f} (fastest all pairs / slowest pruned {min(r['turn_all']) / max(r['turn_prune']):.2f}); "
                f"prune = 0 / all pairs = {med['turn_noprune'] / med['turn_all']:.2f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def cut_main(args):
    import datetime
    lines = [f"# command: python {' '.join(sys.argv)}", f"# date: {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def run(name):
        cmd = ["timeout", "-k", "10", str(CUT_STAGE_LIMIT), sys.executable, os.path.abspath(__file__), "--stage", name, f"--cutoff={args.cutoff}",
               f"--switch={args.switch}", f"--mols={args.mols}", f"--confs={args.confs}", f"--mid-atoms={args.mid_atoms}", f"--chain-atoms={args.chain_atoms}"]
        p = subprocess.run(cmd, capture_output=True, text=True)          # (waits for the child: one GPU process at a time)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"nonbonded_bench: stage {name} ended with status {p.returncode}; nothing more is started")
        return json.loads(p.stdout.strip().splitlines()[-1])

    say(f"# device: {run('device')['device']}")
    say(f"# cutoff {args.cutoff} A, switch {args.switch or 'none'}, reaction field 78.3; the planned kernel into preallocated outputs (energy, terms, gradient); "
        "device events around single calls, one warm-up call, five timed calls: median, all five; every workload a process of its own; "
        "this file is the tool's output, unedited")
    for w in CUT_WORKLOADS:
        r = run(w)
        say(f"{w}: {r['molecules']} molecule(s), {r['atoms']} atoms ({r['smallest']}..{r['largest']} per molecule), C = {r['confs']}, {r['items']} work items")
        rate = {}
        for key, what in (("all_pairs", "all pairs"), ("cut", "cut, prune=1"), ("cut_noprune", "cut, prune=0")):
            med = float(np.median(r[key]))
            rate[key] = 1e6 / med
            say(f"  {what:14s} {med:12.1f} us  {rate[key]:10.1f} calls/s   runs: {', '.join(f'{u:.1f}' for u in r[key])} us")
        say(f"  tiles: {r['tiles']} of {r['all_tiles']} evaluated: mean {r['tiles'] / max(r['items'], 1):.2f} of {r['all_tiles'] / max(r['items'], 1):.2f} per item "
            f"({100.0 * r['tiles'] / max(r['all_tiles'], 1):.1f} %)")
        say(f"  cut, prune=1 / all pairs = {rate['cut'] / rate['all_pairs']:.2f}x; cut, prune=0 / all pairs = {rate['cut_noprune'] / rate['all_pairs']:.2f}x; "
            f"slowest pruned call {max(r['cut']):.1f} us, fastest all-pairs call {min(r['all_pairs']):.1f} us: "
            f"{'faster' if max(r['cut']) < min(r['all_pairs']) else 'NOT faster'}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--mols", type=int, default=256)
    ap.add_argument("--confs", type=int, default=32)
    ap.add_argument("--chain-atoms", type=int, default=50046)
    ap.add_argument("--mid-atoms", type=int, default=513)
    ap.add_argument("--cutoff", type=float, default=0.0, help="A; > 0: measure the nonbonded cutoff (see the module text)")
    ap.add_argument("--switch", type=float, default=0.0, help="A; the switch distance of the cutoff (0: none)")
    ap.add_argument("--gb", default="", help="obc2 or obc1: measure the GB/SA implicit solvent (see the module text)")
    ap.add_argument("--gb-cutoff", type=float, default=0.0, help="A; with --gb: also measure the solvent under this cutoff of its own")
    ap.add_argument("--stage", default=None, choices=("device",) + CUT_WORKLOADS)
    args = ap.parse_args()
    if args.stage:
        return cut_stage(args)
    if args.gb:
        return gb_main(args)
    if args.cutoff:
        return cut_main(args)
    if not torch.cuda.is_available():
        sys.exit("nonbonded_bench: needs a GPU (there is nothing to time without one)")
    from grappa_amd.backend import get_backend
    import datetime
    prop = torch.cuda.get_device_properties(0)
    be = get_backend()
    # (the marketing name comes from the driver's id table and may be a generic one; the architecture and the CU count identify the chip)
    lines = [f"# command: python {' '.join(sys.argv)}",
             f"# date: {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}",
             f"# device: {prop.name}, {getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs, {prop.total_memory / 2 ** 30:.0f} GiB; "
             f"library built for {be.lib.grappa_build_arch().decode()}; torch {torch.__version__}",
             "# device events around single calls, median (min) after warm-up; this file is the tool's output, unedited"]
    print("\n".join(lines), flush=True)

    def report(name, what, pairs, med, mn, reps):
        rate = pairs / (med * 1e-6)
        lines.append(f"{name:6s} {what:18s} {med:12.1f} us (min {mn:10.1f}, {reps:4d} calls)  {rate:10.3e} pair interactions/s  "
                     f"{100 * rate * FLOP_PER_PAIR / PEAK_FP32_VECTOR:5.1f} % of {PEAK_FP32_VECTOR / 1e12:.1f} TFLOP/s at {FLOP_PER_PAIR} flop/pair")
        print(lines[-1], flush=True)
        return rate

    for name, (params, xyz) in (("pool", pool_batch(args.mols, args.confs)), ("chain", chain(args.chain_atoms))):
        nb = NonbondedBatch(params).to("cuda")
        x = torch.from_numpy(xyz).to("cuda")
        n = np.array([p.n_atoms for p in params], dtype=np.float64)
        pairs = float((n * (n - 1)).sum() * x.shape[1])
        lines.append(f"{name}: {len(params)} molecules, {int(n.sum())} atoms ({int(n.min())}..{int(n.max())} per molecule), C = {x.shape[1]}, "
                     f"{nb.n_exceptions} exceptions, {pairs:.4g} pair interactions per call")
        print(lines[-1], flush=True)
        # the kernel alone: HipBackend.nonbonded into preallocated outputs, work-item list built once on the host (two launches) ...
        e_o, t_o, g_o = torch.empty(nb.B, x.shape[1], device="cuda"), torch.empty(2, nb.B, x.shape[1], device="cuda"), torch.empty_like(x)
        tabs = (x, nb.atom_molptr, nb.charge, nb.sigma, nb.epsilon, nb.exc_ptr, nb.exc_atom, nb.exc_qq, nb.exc_sigma, nb.exc_eps)
        plan = be.nonbonded_plan(nb.atom_molptr.cpu(), nb.N, x.shape[1], "cuda")
        k_rate = report(name, "kernel", pairs, *time_events(lambda: be.nonbonded(*tabs, e_o, t_o, g_o, plan=plan), args.seconds))
        # ... the same call without the gradient output, with the list built on the device by every call (three launches, upper-bound
        # grid), and NonbondedBatch.evaluate, which also allocates and zeroes its three outputs
        report(name, "kernel, grad=NULL", pairs, *time_events(lambda: be.nonbonded(*tabs, e_o, t_o, None, plan=plan), args.seconds))
        report(name, "device-built list", pairs, *time_events(lambda: be.nonbonded(*tabs, e_o, t_o, g_o), args.seconds))
        report(name, "evaluate()", pairs, *time_events(lambda: nb.evaluate(x, terms=True), args.seconds))
        if name == "pool":
            dtabs, pad_idx, pad_mask = dense_tables(params, "cuda")
            e, g = nb.evaluate(x)
            te, tg = torch_broadcast(dtabs, pad_idx, pad_mask, x)
            ptr = nb.atom_molptr.tolist()
            tg_flat = torch.cat([tg[b, :ptr[b + 1] - ptr[b]] for b in range(nb.B)])
            lines.append(f"pool   agreement with the torch broadcast: energy {float((e - te).abs().max() / te.abs().max()):.2e}, "
                         f"gradient {float((g - tg_flat).abs().max() / tg_flat.abs().max()):.2e} (largest difference / largest magnitude)")
            print(lines[-1], flush=True)
            t_rate = report(name, "torch broadcast", pairs, *time_events(lambda: torch_broadcast(dtabs, pad_idx, pad_mask, x), args.seconds))
            lines.append(f"pool   kernel / torch broadcast = {k_rate / t_rate:.1f}x")
            print(lines[-1], flush=True)
            del dtabs, te, tg
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
