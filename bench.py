"""bench.py -- molecules/sec of one full Grappa train step (GrappaModel -> Energy with forces -> MolwiseLoss ->
backward -> all-reduce -> fused Adam with grad clipping) on N MI355X of one node.

    python bench.py --gpus 1 --steps 5 --warmup 2                     # the headline alone
    python bench.py --gpus 1 --steps 5 --warmup 2 --full              # ... and every other measurement and check listed below
    python bench.py --gpus 1 --steps 5 --warmup 2 --dump-outputs DIR  # ... and what the last timed step computed, as DIR/<name>.npy
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

N = 1 (the headline line): BASELINE.json configs[1]: 256 molecules of 20-40 atoms drawn from the Espaloma
molecule pool, 32 conformations, production model (40.8 M parameters, keyed init), fp32-grade arithmetic, train mode (dropout on),
synthetic charges / coordinates / reference energies+forces, inputs resident in HBM.  A plain run sets up, warms up, times --steps
steps and prints the line.  With --full the same JSON line also carries
  `roofline`      the dominant kernel family (the dense products): algorithmic 2MNK FLOPs / HIP-event time per call, measured in an
                  instrumented repetition of the same steps right after the timed region; plus the GAT kernels vs HBM,
  `cpu_baseline`  the oracle's CPU restatement of the same train step on a bounded sample (rank 0, N = 1 only),
  `c3`            BASELINE configs[2] (1024 molecules of the whole pool) timed right after C2 with the same fp32-grade arithmetic,
  `c3_bf16`       the same batch in the bf16 STORAGE configuration that config names ("bf16, MFMA dense heads"): never `value`,
  `scale_n1`      BASELINE configs[3]'s 4096-molecule global batch on ONE GPU (4 chunks of 1024, gradients accumulated, one
                  optimiser step) with its own roofline -- the N = 1 point of the strong-scaling curve below,
  `launches`      kernel launches and host enqueue time of one C2 step,
  `b32_train`     the reference's own operating point (32 molecules x 32 conformations, training/config.py:49-52): eager and as a recorded hipGraph,
  `predict_latency_ms`  `Grappa.predict` on one ~40-atom molecule (grappa.py:36-57): eager and through the cache of recorded forwards.
N > 1 (default): STRONG scaling of BASELINE configs[3] (C4): ONE global batch of 4096 molecules dealt to the ranks by size
(dist.shard_indices), loss scaled by 1/4096 on every rank, gradients summed with a two-bucket RCCL all-reduce of the flat gradient
buffer after backward(); `--weak` switches to weak scaling of C2 (256 molecules per GPU).  With --full: the all-reduce time of an
instrumented pass, the collective layer's self-check (`dist`) and rank 0's single-GPU run of the same global batch
(`strong_scaling_reference`, `scaling_factor`).
"""
import argparse
import hashlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_BF16_MFMA_TFLOPS = 16 * 157.3   # same table: the bf16 MFMA runs 16x the fp32 one (~2.5 PFLOP/s dense)
# dominant kernel per GEMM arithmetic: (kernel, bf16 MFMAs issued per fp32 multiply-add column, i.e. partial products)
GEMM_KERNELS = {"f32": ("gemm_f32_kernel<*> (v_mfma_f32_32x32x2_f32)", 0),
                "f32_bf16x9": ("gemm_bf16x_kernel<9,*> (fp32 operands as 3 bf16 pieces, 9 partial products, v_mfma_f32_32x32x16_bf16)", 9),
                "f32_bf16x6": ("gemm_bf16x_kernel<6,*> (fp32 operands as 3 bf16 pieces, 6 partial products, v_mfma_f32_32x32x16_bf16)", 6),
                "bf16x3": ("gemm_bf16x_kernel<3,*>", 3), "bf16": ("gemm_bf16x_kernel<1,*>", 1),
                "f32_f16x3": ("gemm_bf16x_kernel<103,*> (fp32 operands, row-scaled, as 2 fp16 pieces, 3 partial products, v_mfma_f32_32x32x16_f16)", 3)}
PEAK_HBM_GBS = 8000.0             # HBM3E spec
LOSS_KW = dict(gradient_weight=0.8, energy_weight=1.0, param_weight=0.0, proper_regularisation=1e-3)


def keyed_init(model):
    """deterministic non-trivial weights (same scheme as the parity tests)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import golden_utils as gu
    model.load_state_dict(gu.keyed_state_dict(model))


def cpu_model_name() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def kernel_source_hash() -> str:
    """sha256 over the kernel sources: ties a committed PMC summary to the code it was measured on"""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "grappa_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.startswith("host_"):                                           # libgrappa_host.so (index plans on the CPU): no kernel in it
            continue
        if name.endswith((".hip", ".h", ".cpp")) or name == "Makefile":       # the Makefile: compile flags are part of what was measured
            h.update(name.encode())
            h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:16]


def cpu_baseline_child(workload: str, n_mols: int, steps: int, warmup: int, sweep: str, limit_s: float):
    """the oracle (CPU restatement, kind 'port') timed on the host cores on a bounded sample of the same workload; runs in a child
    process of its own (`bench.py --cpu-baseline-child ...`) that never touches the GPU.  BASELINE.md section 2: a thread sweep (one warm-up +
    2 steps on a quarter of the sample per setting) picks the thread count, then `warmup` + `steps` timed steps on the whole sample."""
    from grappa_amd import get_default_model_config
    from grappa_amd.datasets import build_batch_from_pool, workload_molecule_ids
    from oracle import cpu_ref
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import golden_utils as gu
    t_begin = time.time()
    ids = workload_molecule_ids(workload, seed=0)[:n_mols]
    model = cpu_ref.RefGrappaModel(**get_default_model_config())
    model.load_state_dict(gu.keyed_state_dict(model))
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1.5e-5)
    loss_fn = cpu_ref.RefMolwiseLoss(**LOSS_KW)
    energy = cpu_ref.RefEnergy()

    def run(mol_ids, n_steps, n_warm, deadline):
        times = []
        for it in range(n_steps + n_warm):
            g = build_batch_from_pool(mol_ids, n_confs=32, seed=0)
            t0 = time.perf_counter()
            opt.zero_grad()
            loss = loss_fn(energy(model(g)))
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 10.0)
            opt.step()
            if it >= n_warm:
                times.append(time.perf_counter() - t0)
            if time.time() > deadline and times:
                break
        return sorted(times)[len(times) // 2] if times else None, len(times)

    settings = [int(x) for x in sweep.split(",") if x]
    tried = []
    probe = ids[:max(n_mols // 4, 8)]
    for th in settings:
        if time.time() - t_begin > 0.45 * limit_s and tried:
            tried.append({"threads": th, "value": None, "note": "skipped: time limit"})
            continue
        torch.set_num_threads(th)
        t, _ = run(probe, 2, 1, t_begin + 0.55 * limit_s)
        tried.append({"threads": th, "value": len(probe) / t if t else None, "molecules": len(probe)})
    ok = [r for r in tried if r.get("value")]
    best = max(ok, key=lambda r: r["value"])["threads"] if ok else settings[0]
    torch.set_num_threads(best)
    t, n_timed = run(ids, steps, warmup, t_begin + limit_s)
    print(json.dumps({"value": n_mols / t if t else None, "threads": int(torch.get_num_threads()), "median_step_s": t, "steps": n_timed,
                      "warmup": warmup, "sweep": tried}), flush=True)


def cpu_quota_cores():
    """CPUs this job may use at once: the cgroup's bandwidth limit (cpu.max = quota period) if there is one, else the affinity mask"""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            return max(1, int(round(int(q) / int(per))))
    except (OSError, ValueError):
        pass
    try:
        return len(os.sched_getaffinity(0))
    except AttributeError:
        return os.cpu_count() or 1


def numa_cpulists():
    out = []
    base = "/sys/devices/system/node"
    try:
        for name in sorted(os.listdir(base)):
            if name.startswith("node") and name[4:].isdigit():
                cpus = set()
                for part in open(os.path.join(base, name, "cpulist")).read().strip().split(","):
                    lo, _, hi = part.partition("-")
                    cpus.update(range(int(lo), int(hi or lo) + 1))
                if cpus:
                    out.append(sorted(cpus))
    except OSError:
        pass
    return out


def cpu_baseline_mp_child(rank: int, world: int, port: int, workload: str, n_mols: int, steps: int, warmup: int, threads: int, limit_s: float):
    """the same oracle train step with the sample's molecules sharded over `world` processes (one per NUMA domain, `threads`
    threads each, pinned to the domain's CPUs), gradients summed once per step (gloo all-reduce of every parameter gradient), clip + Adam on
    every process: molecules are independent, so this is the host-side analogue of the engine's own data parallelism."""
    import torch.distributed as dist
    from grappa_amd import get_default_model_config
    from grappa_amd.datasets import build_batch_from_pool, workload_molecule_ids
    from oracle import cpu_ref
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import golden_utils as gu
    nodes = numa_cpulists()
    if len(nodes) >= 2:
        try:
            os.sched_setaffinity(0, nodes[rank % len(nodes)])
        except OSError:
            pass
    torch.set_num_threads(threads)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    t_begin = time.time()
    ids = workload_molecule_ids(workload, seed=0)[:n_mols]
    mine = ids[rank::world]
    model = cpu_ref.RefGrappaModel(**get_default_model_config())
    model.load_state_dict(gu.keyed_state_dict(model))
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1.5e-5)
    loss_fn, energy = cpu_ref.RefMolwiseLoss(**LOSS_KW), cpu_ref.RefEnergy()
    params = [p for p in model.parameters()]
    times = []
    for it in range(steps + warmup):
        g = build_batch_from_pool(mine, n_confs=32, seed=0)
        dist.barrier()
        t0 = time.perf_counter()
        opt.zero_grad()
        loss = loss_fn(energy(model(g))) * (len(mine) / n_mols)          # (the loss is a mean over the batch's molecules)
        loss.backward()
        flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params])
        dist.all_reduce(flat)
        o = 0
        for p in params:
            n = p.numel()
            p.grad = flat[o:o + n].view_as(p).clone()
            o += n
        torch.nn.utils.clip_grad_norm_(params, 10.0)
        opt.step()
        dist.barrier()
        if it >= warmup:
            times.append(time.perf_counter() - t0)
        stop = torch.tensor([1.0 if (time.time() - t_begin > limit_s and times) else 0.0])
        dist.all_reduce(stop, op=dist.ReduceOp.MAX)
        if float(stop) > 0:
            break
    if rank == 0:
        t = sorted(times)[len(times) // 2] if times else None
        print(json.dumps({"value": n_mols / t if t else None, "processes": world, "threads_per_process": threads, "median_step_s": t,
                          "steps": len(times), "warmup": warmup, "numa_domains": len(nodes)}), flush=True)
    dist.destroy_process_group()


def cpu_baseline_mp(workload: str, n_mols: int, steps: int, warmup: int, limit_s: float, quota: int):
    """-> the multi-process record (one process per NUMA domain, the quota's cores split between them) or a note why there is none"""
    import socket
    import subprocess
    nodes = numa_cpulists()
    world = max(2, min(len(nodes), 8)) if len(nodes) >= 2 else 2
    threads = max(1, quota // world)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", OMP_NUM_THREADS=str(threads))
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-baseline-mp-child", str(r), str(world), str(port), workload, str(n_mols),
                               str(steps), str(warmup), str(threads), str(limit_s)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
             for r in range(world)]
    rec = None
    try:
        out0, err0 = procs[0].communicate(timeout=limit_s + 120)
        for line in reversed(out0.splitlines()):
            if line.startswith("{"):
                rec = json.loads(line)
                break
        if rec is None:
            rec = {"value": None, "note": f"rank 0 failed: {err0[-300:]}"}
    except subprocess.TimeoutExpired:
        rec = {"value": None, "note": "did not finish in time"}
    finally:
        for pr in procs:                      # (exact PIDs of the children started here)
            if pr.poll() is None:
                try:
                    pr.wait(timeout=20)
                except subprocess.TimeoutExpired:
                    pr.kill()
    rec["layout"] = f"{world} processes x {threads} threads, one per NUMA domain (sched_setaffinity), gloo all-reduce of the gradients once per step"
    return rec


def cpu_baseline(workload: str, n_mols: int, steps: int, warmup: int, limit_s: float):
    """BASELINE.md section 2 on a bounded sample, in ONE child process started before this process touches the GPU: thread sweep over
    {16, 32, 64, 128} (capped by the host), the best setting timed for `steps` steps after `warmup` on `n_mols` molecules of the workload;
    `cores` = the threads the reported figure ran on"""
    import subprocess
    ncpu = os.cpu_count() or 1
    quota = min(cpu_quota_cores(), ncpu)
    # the threads worth trying are bounded by what the job may use at once: on the driver's GPU box the cgroup grants 16 of the host's 256
    # logical CPUs (cpu.max = 1600000 100000), which is why 64 and 128 threads measured SLOWER than 16 in round 5
    settings = sorted({max(1, min(t, ncpu)) for t in (quota // 2, quota, 2 * quota)})
    limit_total, limit_s = limit_s, 0.6 * limit_s
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-child", workload, str(n_mols), str(steps), str(warmup),
           ",".join(map(str, settings)), str(limit_s)]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", OMP_NUM_THREADS=str(max(settings)))
    rec = None
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=limit_s + 90, env=env)
        for line in reversed(out.stdout.splitlines()):
            if line.startswith("{"):
                rec = json.loads(line)
                break
        if rec is None:
            rec = {"value": None, "note": f"child failed: {out.stderr[-300:]}"}
    except subprocess.TimeoutExpired:
        rec = {"value": None, "note": f"did not finish within {limit_s + 90:.0f} s"}
    sweep = ", ".join(f"{r['threads']} -> {r['value']:.1f} mol/s" if r.get("value") else f"{r['threads']} -> {r.get('note')}" for r in rec.get("sweep", []))
    sample = (f"{n_mols} molecules of {workload} x 32 conformations in one batch, production model fp32, full train step (forward, energy+force "
              f"loss, backward, clip, Adam), median of {rec.get('steps')} timed steps after {warmup} warm-up on {rec.get('threads')} threads "
              f"(oracle/cpu_ref.py, torch {torch.__version__} CPU); thread sweep on {max(n_mols // 4, 8)} molecules (1 warm-up + 2 steps each): {sweep}"
              + (f"; {rec['note']}" if rec.get("note") else ""))
    single = {"value": rec.get("value"), "cores": rec.get("threads"), "median_step_s": rec.get("median_step_s")}
    # the same sample sharded over one process per NUMA domain (molecules are independent), gradients summed once per step
    try:
        mp = cpu_baseline_mp(workload, n_mols, max(2, steps - 2), 1, 0.4 * limit_total, quota)
    except Exception as e:  # noqa: BLE001
        mp = {"value": None, "note": repr(e)[:200]}
    best_is_mp = bool(mp.get("value")) and (not single["value"] or mp["value"] > single["value"])
    value = mp["value"] if best_is_mp else single["value"]
    cores = (mp.get("processes", 0) * mp.get("threads_per_process", 0)) if best_is_mp else rec.get("threads")
    sample += (f"; ALSO sharded over processes: {mp.get('layout')}: " + (f"{mp['value']:.1f} molecules/s (median of {mp.get('steps')} steps)" if mp.get("value") else f"no figure ({mp.get('note')})")
               + f"; the job may use {quota} of the host's {ncpu} logical CPUs at once (cgroup cpu.max), `value` = the faster of the two layouts")
    return {"value": value, "unit": "molecules/s", "cores": cores, "host_cores": ncpu, "cpu_quota_cores": quota, "threads_used": rec.get("threads"),
            "cpu_model": cpu_model_name(), "kind": "port", "sample": sample, "median_step_s": rec.get("median_step_s"),
            "single_process": single, "multi_process": mp}


def distinct_devices(ranks, world: int, enforce: bool) -> int:
    """-> how many distinct devices the ranks of this job sit on (index + uuid as each rank reports them).  enforce (RCCL on GPUs): fewer than
    `world` means several ranks share a GPU -- a "scaling" figure from such a run would be meaningless, so the job REFUSES to print a line"""
    distinct = len({(r["device_index"], r["device_uuid"]) for r in ranks})
    if enforce and distinct != world:
        raise SystemExit(f"{world} ranks over RCCL but only {distinct} distinct devices: no scaling line is reported ({ranks})")
    return distinct


def finite_loss(what: str, loss) -> float:
    """the loss of the last timed step of `what`; a step that ends in a NaN / inf loss is not a measurement (NaN operands even run FASTER on
    this chip -- the matrix pipes draw less power and the clock rises: a racy refresh of the operand scales once read as an 11 % gain at
    C2): the run dies instead of printing a line"""
    v = float(loss)
    if not math.isfinite(v):
        raise SystemExit(f"bench.py: the {what} step ended with a non-finite loss ({v}); no number is reported from such a run")
    return v


DUMP_ROWS_CAP = 1 << 20          # elements per dumped array beyond which a fixed sample of its rows is written
DUMP_WEIGHTS_SAMPLE = 1 << 20     # draws for the sample of the flat weight / gradient buffers


def dump_outputs(path: str, graphs, flat, loss: float) -> dict:
    """what the last timed train step handed its caller, as `path`/<name>.npy (float32): the loss, per conformation the energies
    (molecules, C) and forces (atoms, C, 3), the parameters each tuple level was given (k, eq), and a fixed sample of the updated
    weights and of the gradients they were updated with.  Several chunks: their rows one after another.  An array above DUMP_ROWS_CAP
    elements keeps a sample of its rows drawn by a generator seeded with its name, so that two builds write the same rows.
    -> {name: shape}"""
    import zlib
    import numpy as np
    os.makedirs(path, exist_ok=True)

    def rows_sample(name, a):
        if a.size <= DUMP_ROWS_CAP or a.shape[0] < 2:
            return a
        per_row = a.size // a.shape[0]
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        return a[np.unique(rng.integers(0, a.shape[0], size=max(DUMP_ROWS_CAP // per_row, 1)))]

    arrays = {"loss": np.array([loss], dtype=np.float32),
              "energy": torch.cat([g.nodes["g"].data["energy"].detach() for g in graphs]),
              "forces": torch.cat([g.nodes["n1"].data["gradient"].detach() for g in graphs])}
    for lvl in ("n2", "n3", "n4", "n4_improper"):
        for k in ("k", "eq"):
            if k in graphs[0].nodes[lvl].data:
                arrays[f"{lvl}_{k}"] = torch.cat([g.nodes[lvl].data[k].detach() for g in graphs])
    idx = torch.from_numpy(np.unique(np.random.default_rng(0).integers(0, flat.numel, size=DUMP_WEIGHTS_SAMPLE))).to(flat.data.device)
    arrays["weights_sample"] = flat.data[idx]
    arrays["weight_grads_sample"] = flat.grad[idx]
    for name, a in arrays.items():
        a = a.float().cpu().numpy() if torch.is_tensor(a) else a
        arrays[name] = np.ascontiguousarray(rows_sample(name, a), dtype=np.float32)
    total = sum(a.nbytes for a in arrays.values())
    assert total <= 64 * 2 ** 20, total
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


def log(*a):
    print(f"[bench {time.strftime('%H:%M:%S')}]", *a, file=sys.stderr, flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-baseline-mp-child":
        a = sys.argv[2:]
        cpu_baseline_mp_child(int(a[0]), int(a[1]), int(a[2]), a[3], int(a[4]), int(a[5]), int(a[6]), int(a[7]), float(a[8]))
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-baseline-child":
        cpu_baseline_child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6], float(sys.argv[7]))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default=None, help="default: C2-pubchem-b256 at N = 1 (and with --weak), C4-espaloma-b4096 (strong scaling) at N > 1")
    ap.add_argument("--weak", action="store_true", help="N > 1: weak scaling, the workload's batch on every GPU (default at N > 1 is strong scaling of C4)")
    ap.add_argument("--strong-global-batch", type=int, default=0, help="strong scaling of this many molecules of the workload's molecule range (default at N > 1: 4096 of C4)")
    ap.add_argument("--chunk", type=int, default=1024, help="molecules per forward/backward pass of a rank (larger shards are accumulated over chunks)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--shape-table", default="", help="append a per-shape account of the dense products of every instrumented job to this file "
                    "(shape, layout, operand format, launches and kernel time per step, TFLOP/s, fraction of the ceiling, share of the products' time)")
    ap.add_argument("--no-extras", action="store_true", help="N = 1: skip the C3 and C4-on-one-GPU timings that follow the headline measurement")
    ap.add_argument("--gemm-precision", default=None, help="arithmetic of the dense products (default: the backend's, f32_f16x3)")
    ap.add_argument("--act-dtype", default="f32", choices=["f32", "bf16"], help="bf16: the bf16 STORAGE configuration for the main job (profiling / "
                    "BASELINE configs[2] runs; the line's dtype then reads bf16 -- never the default)")
    ap.add_argument("--alt-precision", default="f32,f32_bf16x6", help="also time K steps with these GEMM arithmetics (comma separated; reported beside the default); '' to skip")
    ap.add_argument("--bwd-precision", default="", help="also time K steps with the backward-pass products in this arithmetic (reported beside the default, never as `value`); '' to skip")
    ap.add_argument("--cpu-sample", type=int, default=128, help="molecules in the CPU baseline sample")
    ap.add_argument("--cpu-limit", type=float, default=150.0, help="wall-clock limit of the CPU baseline child's timed work, seconds")
    ap.add_argument("--no-scaling-reference", action="store_true", help="N > 1, strong scaling: skip rank 0's single-GPU run of the whole global batch")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL over xGMI; default) | gloo (functional test of the N>1 path on one GPU)")
    ap.add_argument("--device", default="cuda", choices=["cuda", "cpu"], help="cpu: TEST ONLY (tests/test_bench_launch.py) -- the host logic of the "
                    "N-rank path on a machine without a GPU; the caller must have installed a test backend (the product has none for the CPU), "
                    "no kernel timing, never a measurement")
    ap.add_argument("--tiny-model", action="store_true", help="TEST ONLY: a 60 k-parameter model instead of the production one (with --device cpu)")
    ap.add_argument("--full", action="store_true", help="also measure and check everything beyond the headline: CPU baseline, instrumented "
                    "roofline pass, other GEMM arithmetics, weight planes, the other writer-head stream setting, C3 / C3-bf16 / C4 on one GPU, "
                    "recorded steps, launch counts, b32, predict, C5; at N > 1 the collective self-check and the single-GPU scaling reference.  "
                    "--no-cpu-baseline, --no-extras, --alt-precision, --bwd-precision, --shape-table and --no-scaling-reference act within it")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed steps, write what the last timed step computed (loss, "
                    "energies, forces, the parameters per tuple level, a fixed sample of the updated weights and of their gradients) as "
                    "DIR/<name>.npy, float32, at most 64 MB in all (larger arrays: a fixed, seeded sample of their rows); rank 0 only")
    args = ap.parse_args()
    for opt_name, given in (("--shape-table", args.shape_table), ("--bwd-precision", args.bwd_precision)):
        if given and not args.full:
            ap.error(f"{opt_name} belongs to the measurements of --full")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N`: this process has not touched the GPU; it starts the N ranks (one process per GPU) as children and
        # relays their output (rank 0 prints the JSON line) and exit code
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        log("launching", " ".join(cmd))
        sys.exit(subprocess.run(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1")).returncode)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    strong = world > 1 and not args.weak or args.strong_global_batch > 0
    workload = args.workload or ("C4-espaloma-b4096" if strong else "C2-pubchem-b256")
    # CPU baseline first, in child processes, before this process initialises the GPU (rank 0 at N = 1 only)
    cpu_base = None
    if args.full and world == 1 and args.gpus == 1 and not args.no_cpu_baseline and args.device == "cuda":
        log(f"cpu baseline (oracle, {args.cpu_sample} molecules, limit {args.cpu_limit:.0f} s) ...")
        cpu_base = cpu_baseline(workload, args.cpu_sample, 5, 2, args.cpu_limit)
        log(f"cpu baseline: {cpu_base}")
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} does not match WORLD_SIZE={world}")
    on_gpu = args.device == "cuda"
    if not on_gpu and not args.tiny_model:
        raise SystemExit("--device cpu is a host-logic test mode: it needs --tiny-model")
    if args.dist_backend == "gloo":          # test mode: all ranks share the visible device(s)
        local_rank = local_rank % max(torch.cuda.device_count(), 1)
    if on_gpu:
        torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank) if on_gpu else torch.device("cpu")

    def sync():
        if on_gpu:
            torch.cuda.synchronize()
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend=args.dist_backend)

    from grappa_amd import Energy, MolwiseLoss, get_default_model_config, model_from_config, ops
    from grappa_amd.backend import get_backend
    from grappa_amd.datasets import WORKLOADS, WORKLOAD_DESCRIPTIONS, build_batch_from_pool, pool_atom_counts, select_molecules, workload_molecule_ids
    from grappa_amd.dist import BucketedGradReducer, shard_indices
    from grappa_amd.optim import FlatParams, FusedAdam

    log("imports done; building model")
    be = get_backend()
    if args.act_dtype == "bf16":
        ops.set_activation_dtype("bf16")
        be.set_gemm_precision("bf16")
    if args.gemm_precision:
        be.set_gemm_precision(args.gemm_precision)
    model_cfg = get_default_model_config()
    if args.tiny_model:
        model_cfg.update(graph_node_features=16, gnn_width=32, gnn_attentional_layers=1, gnn_attention_heads=2,
                         **{f"{h}_{k}": v for h in ("bond", "angle", "proper", "improper")
                            for k, v in (("transformer_depth", 1), ("n_heads", 2), ("transformer_width", 32), ("symmetriser_depth", 2), ("symmetriser_width", 16))})
    model = model_from_config(model_cfg)
    keyed_init(model)
    model = model.to(dev).train()
    flat = FlatParams(model)
    opt = FusedAdam(flat, lr=1.5e-5, max_grad_norm=10.0)
    reducer = BucketedGradReducer(model, flat)
    energy = Energy()
    ops.manual_seed(1234 + rank)
    counts = pool_atom_counts()

    class Job:
        """one configuration on this rank: its molecules in chunks resident in HBM, and the train step over them"""

        def __init__(self, name, global_batch, ids, seed):
            self.name, self.global_batch, self.n_local = name, int(global_batch), len(ids)
            self.loss_fn = MolwiseLoss(**LOSS_KW)
            self.loss_fn.global_batch_size = int(global_batch)
            self.graphs = [build_batch_from_pool(ids[i:i + args.chunk], n_confs=WORKLOADS[name][3], seed=seed).to(dev)
                           for i in range(0, len(ids), args.chunk)]
            self.atoms = sum(g.plan().N for g in self.graphs)
            self.tuples = {k: sum(int(g.plan().T[k]) for g in self.graphs) for k in self.graphs[0].plan().T}
            self.allreduce_events = None
            self.solo = False          # True: this rank alone (the single-GPU reference of the strong-scaling curve): no collective

        def step(self):
            opt.zero_grad()
            # the overlapped all-reduce bucket leaves with the LAST chunk's backward pass (never from a rank that runs alone)
            reducer.begin_step(10 ** 9 if self.solo else len(self.graphs))
            for g in self.graphs:                                      # gradients accumulate in the flat buffer over the chunks
                for lvl in ("n2", "n3", "n4", "n4_improper"):         # drop last step's outputs
                    for k in ("k", "eq"):
                        g.nodes[lvl].data.pop(k, None)
                loss = self.loss_fn(energy(model(g)))
                loss.backward()
            if self.solo:
                reducer._flush_queued_wgrads()
            elif self.allreduce_events is not None and on_gpu:
                # HIP events around the collectives of BOTH buckets: the reducer records one where the heads' bucket leaves
                # (only with the overlap on) and a pair around what finish() sends and waits for
                reducer.time_events = []
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                reducer.finish()
                e1.record()
                self.allreduce_events.append((e0, e1, reducer.time_events))
                reducer.time_events = None
            elif self.allreduce_events is not None:
                t_ar = time.perf_counter()
                reducer.finish()
                self.allreduce_events.append(1e3 * (time.perf_counter() - t_ar))
            else:
                reducer.finish()       # all-reduce of what the backward pass has not sent yet (the GNN bucket), wait for both
            opt.step()
            return loss

        def timed(self, steps, warmup):
            """-> (seconds for `steps` steps as the MAX over ranks, last loss)"""
            multi = world > 1 and not self.solo
            for _ in range(warmup):
                loss = self.step()
            sync()
            if multi:
                dist.barrier()
            sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = self.step()
            sync()
            if multi:
                dist.barrier()
            sync()
            dt = time.perf_counter() - t0
            if multi:
                t = torch.tensor([dt], device=dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt = float(t)
            return dt, finite_loss(self.name, loss.detach())

        def describe(self):
            mdl = "TINY TEST MODEL (not a measurement)" if args.tiny_model else "production GrappaModel 40.8M params"
            return {"workload": f"{self.name}: {WORKLOAD_DESCRIPTIONS[self.name]}, {WORKLOADS[self.name][3]} conformations, {mdl} "
                                f"(keyed init), train mode (dropout on), Adam + clip 10"
                                + (f"; this rank: {self.n_local} molecules in {len(self.graphs)} chunks of <= {args.chunk}, gradients accumulated, one optimiser step"
                                   if len(self.graphs) > 1 else ""),
                    "global_batch": self.global_batch, "molecules_rank0": self.n_local, "conformations": WORKLOADS[self.name][3],
                    "atoms_rank0": self.atoms, "tuples_rank0": self.tuples, "chunks_rank0": len(self.graphs)}

    def strong_job(name, total):
        _, lo, hi, _ = WORKLOADS[name]
        all_ids = workload_molecule_ids(name, seed=0) if total == WORKLOADS[name][0] else select_molecules(total, seed=0, min_atoms=lo, max_atoms=hi)
        sizes = [int(counts[i]) for i in all_ids]
        mine = [all_ids[j] for j in shard_indices(sizes, world, rank)]
        return Job(name, total, mine, seed=0)

    log("model ready; building workload")
    if strong:
        job = strong_job(workload, args.strong_global_batch or WORKLOADS[workload][0])
    else:
        job = Job(workload, WORKLOADS[workload][0] * world, workload_molecule_ids(workload, seed=rank), seed=rank)
    log(f"workload {job.name} ready: molecules {job.n_local} atoms {job.atoms} tuples {job.tuples}; warmup")
    def recorded_step(j, steps):
        """the train step of job `j` (one chunk) as ONE hipGraph replay on its resident batch (grappa_amd/capture.py CapturedTrainStep: zero_grad ->
        forward -> Energy -> loss -> backward -> clip + Adam, the four writer heads as branches of the graph): `steps` replays between two
        synchronisations.  The recording trains (3 warm-up steps); training state is put back afterwards so that later measurements start
        from the same weights."""
        from grappa_amd.capture import CapturedTrainStep
        if len(j.graphs) != 1:
            raise RuntimeError("recorded_step: one resident chunk only")
        cap = CapturedTrainStep(model, energy, j.loss_fn, opt, j.graphs[0], warmup=3, preserve_state=True)
        try:
            for _ in range(2):
                cap()
            sync()
            t0_ = time.perf_counter()
            for _ in range(steps):
                cap()
            sync()
            d_ = time.perf_counter() - t0_
            return {"value": j.global_batch * steps / d_, "unit": "molecules/s", "ms_per_step": 1e3 * d_ / steps, "steps": steps, "warmup": 2,
                    "mode": "hipGraph replay of the whole train step on the resident batch (CapturedTrainStep), dropout masks fresh per replay",
                    "final_loss": finite_loss(f"recorded {j.name}", cap.loss), "gemm_precision": be.gemm_precision_name,
                    "activation_storage": "bf16" if ops.act_dtype() is not None else "f32"}
        finally:
            del cap
            torch.cuda.empty_cache()

    dt, final_loss = job.timed(args.steps, args.warmup)
    log(f"timed region done: {1e3 * dt / args.steps:.1f} ms/step")
    dumped = None
    if args.dump_outputs and rank == 0:
        # before anything below moves the weights or overwrites the graphs' outputs
        dumped = dump_outputs(args.dump_outputs, job.graphs, flat, final_loss)
        log(f"outputs of the last timed step written to {args.dump_outputs}: {dumped}")

    GEMM_PEAK_NOTE = ("achieved = algorithmic 2MNK FLOPs / HIP-event time of the calls; peak = bf16 dense MFMA peak (16 x 157.3 TFLOP/s, "
                      "MI355X_MICROARCH.md; the fp16 one is the same) / partial products issued per fp32 product; the time of the operands' "
                      "maxima passes (f32_f16x3) is charged to the products; `achieved` counts the products LAUNCHED (`tflop_per_step_launched`); SURVEY "
                      "8(d)'s per-token count (`tflop_per_step`) is ~5 % larger because the first layer of the proper and angle writers runs its "
                      "LayerNorm + QKV product on (atom, position) rows (`achieved_with_algorithmic_credit` = that count over the same time)")

    def write_shape_table(path, title, details, steps):
        """per-shape account of the products of an instrumented pass (one queue: a launch's HIP-event time is its kernel's own).  A grouped
        launch's time is shared among its products by their FLOPs."""
        import collections
        acc = collections.OrderedDict()
        total_ms = 0.0
        for fam, det, ms, fl, _by in details:
            if fam != "gemm_f32" or not det:
                continue
            total_ms += ms
            fsum = sum(2.0 * d["M"] * d["N"] * d["K"] for d in det) or 1.0
            for d in det:
                f = 2.0 * d["M"] * d["N"] * d["K"]
                key = (d["layout"], d["M"], d["N"], d["K"], d["fmt"], d["epi"], len(det) > 1)
                a = acc.setdefault(key, [0, 0.0, 0.0])
                a[0] += 1
                a[1] += ms * f / fsum
                a[2] += f
        kname, nprod = GEMM_KERNELS[getattr(be, "gemm_precision_name", "f32")]
        peak = (PEAK_F32_MFMA_TFLOPS if nprod == 0 else PEAK_BF16_MFMA_TFLOPS / nprod) if ops.act_dtype() is None else PEAK_BF16_MFMA_TFLOPS
        with open(path, "a") as fh:
            fh.write(f"# {title}: dense products of {steps} instrumented step(s) on ONE queue, HIP events around every launch; ceiling {peak:.1f} TFLOP/s; "
                     f"products {total_ms / steps:.2f} ms per step\n")
            fh.write("# layout      M      N      K  operands epilogue grouped  launches/step  us/launch   ms/step  TFLOP/s   frac  share  tiles(256x128)/256 CUs\n")
            for (lay, M, N, K, fmt, epi, grouped), (n, ms, fl) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
                tf = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
                tiles = ((M + 255) // 256) * ((N + 127) // 128)
                fh.write(f"  {lay:6s} {M:6d} {N:6d} {K:6d}  {fmt:7s}  {epi:7s} {'yes' if grouped else 'no ':3s}   {n / steps:10.1f}  {1e3 * ms / n:9.1f}  {ms / steps:8.3f}  {tf:7.1f}  {tf / peak:5.3f}  "
                         f"{100 * ms / total_ms:5.1f}  {tiles / 256:6.2f}\n")

    def instrument(j, steps):
        """instrumented repetition of a job's steps: HIP events around every GEMM / GAT launch on the launch stream (ONE stream:
        GRAPPA_HEAD_STREAMS=1 and GRAPPA_WGRADS_ASIDE=0 semantics; profiles/ rocprof runs use the same settings) and around the gradient all-reduce
        -> (gemm roofline dict, gat roofline dict, ms per instrumented step, all-reduce ms per step)"""
        hs = model.parameter_writer.head_streams
        model.parameter_writer.head_streams = 1
        aside = getattr(be, "wgrads_aside", False)
        pinned = False
        if on_gpu:
            be.wgrads_aside = False           # one queue: a launch's HIP-event time is the kernel's own, not its share of a busy chip
            if getattr(be, "_tails", None) is not None and not be._tails_pinned:
                be.pin_tail_launches(be._tails)      # the products keep the plans of the measured configuration (split-K tails off under four streams)
                pinned = True
        j.step()
        sync()
        j.allreduce_events = []
        if on_gpu:
            be.start_profile()
        t1 = time.perf_counter()
        for _ in range(steps):
            j.step()
        prof = be.stop_profile() if on_gpu else {}
        dtp = time.perf_counter() - t1
        if on_gpu and args.shape_table:
            write_shape_table(args.shape_table, j.name + (" bf16 storage" if ops.act_dtype() is not None else ""), be.last_profile_details, steps)
        ar_ms = sum((ev[0].elapsed_time(ev[1]) if on_gpu else ev) for ev in j.allreduce_events) / max(len(j.allreduce_events), 1)
        # with the overlap on: how long before finish() the heads' bucket left (the collective had that long to run beside the GNN's backward pass)
        leads = [te[1].elapsed_time(ev[0]) for ev in j.allreduce_events if on_gpu for te in ev[2] if te[0] == "heads_sent"]
        j.heads_bucket_lead_ms = sum(leads) / len(leads) if leads else None
        j.allreduce_events = None
        model.parameter_writer.head_streams = hs
        if on_gpu:
            be.wgrads_aside = aside
            if pinned:
                be.pin_tail_launches(None)
        n, ms, fl, by = prof.get("gemm_f32", (0, 0.0, 0.0, 0.0))
        # the passes that find the operands' row / column maxima (precision f32_f16x3) are part of that arithmetic's price: their time
        # is charged to the products (the launch count and the bytes stay those of the products)
        n_amax, ms_amax = prof.get("amax", (0, 0.0, 0.0, 0.0))[:2]
        ms_products = ms
        ms += ms_amax
        # algorithmic FLOPs = SURVEY 8(d)'s per-token count: those of the products launched plus those the (atom, position)-row
        # formulation of the first writer layer did not have to launch (ops.ProjFirstLayerFn); both rates are reported
        fl_launched = fl
        fl += prof.get("gemm_saved", (0, 0.0, 0.0, 0.0))[2]
        # `achieved` / `frac`: the FLOPs of the products actually launched over their time; the rate with the un-launched
        # first-layer products credited (SURVEY 8(d)'s per-token count) is the secondary field
        achieved = (fl_launched / (ms * 1e-3)) / 1e12 if ms > 0 else 0.0
        achieved_credit = (fl / (ms * 1e-3)) / 1e12 if ms > 0 else 0.0
        kname, nprod = GEMM_KERNELS[getattr(be, "gemm_precision_name", "f32")]
        if ops.act_dtype() is not None:
            kname = "gemm_planes_kernel<1,*> (bf16 operands by LDS-DMA, v_mfma_f32_32x32x16_bf16, fp32 accumulate) + gemm_bf16x_kernel<1,*> for the fp32-operand products"
        # `achieved` counts the ALGORITHMIC FLOPs (2MNK); the split kernels issue `nprod` bf16 MFMAs per fp32 product, so the
        # ceiling in the same unit is the bf16 dense peak / nprod
        peak = PEAK_F32_MFMA_TFLOPS if nprod == 0 else PEAK_BF16_MFMA_TFLOPS / nprod
        roof = {"bound": "mfma", "kernel": kname, "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                "frac_of_native_f32_mfma_peak": achieved / PEAK_F32_MFMA_TFLOPS, "frac_of_bf16x6_ceiling": achieved / (PEAK_BF16_MFMA_TFLOPS / 6),
                "gemm_precision": getattr(be, "gemm_precision_name", None),
                "traffic": None, "traffic_source": None, "algorithmic_bytes_per_launch": by / max(n, 1),
                "launches_per_step": n / steps, "avg_launch_us": 1e3 * ms / max(n, 1), "gflop_per_launch": fl / max(n, 1) / 1e9,
                "kernel_ms_per_step": ms / steps, "tflop_per_step": fl / steps / 1e12, "tflop_per_step_launched": fl_launched / steps / 1e12,
                "achieved_with_algorithmic_credit": achieved_credit, "frac_with_algorithmic_credit": achieved_credit / peak, "note": GEMM_PEAK_NOTE}
        if n_amax:
            roof.update({"maxima_pass_ms_per_step": ms_amax / steps, "maxima_pass_launches_per_step": n_amax / steps,
                         "products_only_ms_per_step": ms_products / steps,
                         "products_only_tflops": (fl_launched / (ms_products * 1e-3)) / 1e12 if ms_products > 0 else 0.0})
        # round 6: the fused writer-head layer (grappa_writer_head_fwd / _bwd, bf16 storage) is a kernel family of its own: its products are NOT in
        # `achieved` above (which stays the dense products' launches), so it carries its own line -- 12 * 512^2 FLOP per token row and launch
        nw, msw, flw, byw = prof.get("writer_layer", (0, 0.0, 0.0, 0.0))
        if nw:
            aw = (flw / (msw * 1e-3)) / 1e12 if msw > 0 else 0.0
            roof["writer_layer"] = {"bound": "mfma", "kernel": "writer_layer_fwd/bwd_bf16_kernel (v_mfma_f32_16x16x32_bf16, one launch per transformer layer and pass)",
                                    "achieved": aw, "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": aw / PEAK_BF16_MFMA_TFLOPS,
                                    "launches_per_step": nw / steps, "kernel_ms_per_step": msw / steps, "tflop_per_step": flw / steps / 1e12,
                                    "algorithmic_bytes_per_launch": byw / max(nw, 1),
                                    "all_products_achieved": ((fl_launched + flw) / ((ms + msw) * 1e-3)) / 1e12 if (ms + msw) > 0 else 0.0}
            roof["writer_layer"]["all_products_frac"] = roof["writer_layer"]["all_products_achieved"] / peak
        gat = {}
        for fam in ("gat_fwd", "gat_bwd"):
            n_, ms_, fl_, by_ = prof.get(fam, (0, 0.0, 0.0, 0.0))
            a_ = (by_ / (ms_ * 1e-3)) / 1e9 if ms_ > 0 else 0.0
            gat[fam] = {"bound": "hbm", "achieved": a_, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": a_ / PEAK_HBM_GBS,
                        "avg_launch_us": 1e3 * ms_ / max(n_, 1), "mb_per_launch": by_ / max(n_, 1) / 1e6}
        return roof, gat, 1e3 * dtp / steps, ar_ms

    head_streams = model.parameter_writer.head_streams
    roof = gat = ms_instr = allreduce_ms = None
    if args.full:
        roof, gat, ms_instr, allreduce_ms = instrument(job, args.steps)
        log("instrumented pass done")

    def alt_run(setter, restore):
        setter()
        d, _ = job.timed(args.steps, 1)
        restore()
        return {"value": job.global_batch * args.steps / d, "ms_per_step": 1e3 * d / args.steps}

    # the same K steps with the dense products on the native fp32 matrix instruction, for reference next to the default
    alt = {}
    for name in [a for a in args.alt_precision.split(",") if args.full and on_gpu and a and a != be.gemm_precision_name]:
        default_precision = be.gemm_precision_name
        alt[name] = alt_run(lambda: be.set_gemm_precision(name), lambda: be.set_gemm_precision(default_precision))
        alt[name]["gemm_precision"] = name
        log(f"alt precision {name}: {alt[name]['ms_per_step']:.1f} ms/step")
    bwd = None
    if args.bwd_precision:
        bwd = alt_run(lambda: be.set_gemm_precision_bwd(args.bwd_precision), lambda: be.set_gemm_precision_bwd(None))
        bwd.update({"backward_gemm_precision": args.bwd_precision,
                    "note": "NOT the headline configuration: forward products as in `default`, dgrad/wgrad products in the named arithmetic "
                            "(GRAPPA_GEMM_PRECISION_BWD); parameters / energies / forces / loss are bit-identical to the default"})
        log(f"backward precision {args.bwd_precision}: {bwd['ms_per_step']:.1f} ms/step")

    # opt-in kernel (GRAPPA_WEIGHT_PLANES): the same steps with the weights read from their pre-split bf16 planes by LDS-DMA
    wpl = None
    if args.full and on_gpu and world == 1 and not args.no_extras and not be.weight_planes and args.act_dtype == "f32":
        default_precision = be.gemm_precision_name
        be.set_gemm_precision("f32_bf16x6")            # the plane format is a bf16 split: it rides on the bf16x6 arithmetic
        be.weight_planes = True
        d_w, _ = job.timed(args.steps, 1)
        be.weight_planes = False
        be.set_gemm_precision(default_precision)
        wpl = {"value": job.global_batch * args.steps / d_w, "ms_per_step": 1e3 * d_w / args.steps, "gemm_precision": "f32_bf16x6",
               "note": "GRAPPA_WEIGHT_PLANES=1 with GRAPPA_GEMM_PRECISION=f32_bf16x6: forward / dgrad products read the weight from bf16 planes "
                       "split once per optimiser step (csrc/gemm_planes.hip gemm_wplanes_kernel); results equal f32_bf16x6 to rounding; not the default"}
        log(f"weight planes: {wpl['ms_per_step']:.1f} ms/step")

    # the other stream setting of the writer heads beside the default (four HIP streams since round 3), never `value`
    heads_alt = None
    if args.full and on_gpu and world == 1 and not args.no_extras and args.act_dtype == "f32":
        default_streams = model.parameter_writer.head_streams
        other = 1 if default_streams > 1 else 4
        model.parameter_writer.head_streams = other
        d_h, _ = job.timed(args.steps, 2)
        model.parameter_writer.head_streams = default_streams
        heads_alt = {"value": job.global_batch * args.steps / d_h, "ms_per_step": 1e3 * d_h / args.steps, "writer_head_streams": other,
                     "note": f"GRAPPA_HEAD_STREAMS={other} (the default is {default_streams}): bond / angle / proper / improper writers on "
                             f"{'one HIP stream' if other == 1 else 'four HIP streams'}; bit-identical gradients with grouped launches off "
                             "(tests/test_gpu_e2e.py, tools/head_streams_soak.py)"}
        log(f"writer heads on {other} stream(s): {heads_alt['ms_per_step']:.1f} ms/step")

    # N = 1: the other single-GPU configurations, timed right after the headline measurement: C3 in the headline arithmetic, C3 in the
    # bf16 STORAGE configuration BASELINE configs[2] names (never `value`), and the 4096-molecule batch of C4 on one GPU
    extras = {}
    if args.full and on_gpu and world == 1 and not args.no_extras and not strong and workload == "C2-pubchem-b256" and args.act_dtype == "f32":
        headline_graphs = job.graphs
        default_precision = be.gemm_precision_name
        for key, name, steps, bf16 in (("c3", "C3-espaloma-b1024", 5, False), ("c3_bf16", "C3-espaloma-b1024", 5, True),
                                       ("scale_n1", "C4-espaloma-b4096", 5, False)):
            try:
                if bf16:
                    ops.set_activation_dtype("bf16")
                    be.set_gemm_precision("bf16")
                j2 = Job(name, WORKLOADS[name][0], workload_molecule_ids(name, seed=0), seed=0)
                d2, l2 = j2.timed(steps, 2)
                extras[key] = {"value": j2.global_batch * steps / d2, "unit": "molecules/s", "ms_per_step": 1e3 * d2 / steps, "steps": steps, "warmup": 2,
                               "scaling": None, "n_gpus": 1, "gemm_precision": be.gemm_precision_name,
                               "activation_storage": "bf16" if bf16 else "f32", "final_loss": l2, "config": j2.describe()}
                r2, g2, _, _ = instrument(j2, 2 if key != "scale_n1" else 1)
                # PMC counters cannot be read in-process: a committed rocprofv3 --pmc summary of the same workload and storage is reported while the
                # kernel sources it was measured on are the ones running (profiles/pmc_traffic_c3.json, pmc_traffic_c3_bf16.json: tools/pmc_only.sh)
                tp2 = os.path.join(ROOT, "profiles", {"c3": "pmc_traffic_c3.json", "c3_bf16": "pmc_traffic_c3_bf16.json"}.get(key, "-"))
                if os.path.exists(tp2):
                    try:
                        tj2 = json.load(open(tp2))
                        if tj2.get("kernel_source_hash") == kernel_source_hash():
                            r2["traffic"] = tj2["families"]["dense_products"]["hbm_bytes_per_step"] / max(r2["launches_per_step"], 1.0)
                            r2["traffic_source"] = f"profiles/{os.path.basename(tp2)} (as the headline's)"
                    except Exception:
                        pass
                for k_ in ("traffic", "traffic_source"):
                    if r2.get(k_) is None:
                        r2.pop(k_, None)
                extras[key]["roofline"], extras[key]["roofline_gat"] = r2, g2
                if key == "scale_n1":
                    extras[key]["note"] = ("BASELINE configs[3]'s 4096-molecule global batch on ONE GPU (4 chunks of 1024, gradients accumulated, one optimiser "
                                           "step): the N = 1 point of the strong-scaling curve the driver measures at N = 2, 4, 8")
                if bf16:
                    extras[key]["note"] = ("bf16 STORAGE configuration (BASELINE configs[2]): activations and activation gradients in HBM as bf16, dense "
                                           "products straight from bf16 operands (fp32 accumulate), LayerNorm statistics / softmax / energies / forces / "
                                           "weights / weight gradients fp32; parameters within 2e-2 of the oracle (tests/test_gpu_bf16.py); reported "
                                           "beside, never as, the fp32-grade headline")
                log(f"{key}: {extras[key]['ms_per_step']:.1f} ms/step = {extras[key]['value']:.0f} molecules/s")
                if key in ("c3", "c3_bf16"):
                    # the same step as ONE recorded hipGraph on the resident batch: what is left when the host's enqueue is gone
                    try:
                        extras[key + "_recorded"] = recorded_step(j2, 5)
                        log(f"{key}_recorded: {extras[key + '_recorded']['ms_per_step']:.1f} ms/step")
                    except Exception as e:  # noqa: BLE001
                        extras[key + "_recorded"] = {"value": None, "error": repr(e)[:300]}
                del j2
            except Exception as e:  # noqa: BLE001  (an extra must never take the headline line down)
                extras[key] = {"value": None, "error": repr(e)[:300]}
            finally:
                ops.set_activation_dtype("f32")
                be.set_gemm_precision(default_precision)
                torch.cuda.empty_cache()
        job.graphs = headline_graphs
        try:
            extras["c2_recorded"] = recorded_step(job, args.steps)
            log(f"c2_recorded: {extras['c2_recorded']['ms_per_step']:.2f} ms/step (eager headline {1e3 * dt / args.steps:.2f})")
        except Exception as e:  # noqa: BLE001
            extras["c2_recorded"] = {"value": None, "error": repr(e)[:300]}
        finally:
            torch.cuda.empty_cache()
        # ---- launch counts and host enqueue time of one headline step: the library counts its own launches; the host time is
        # taken with an empty queue in front of every step, so it is the time Python + the C ABI need to ISSUE the step, not to run it
        try:
            host_ms, launches = [], []
            for _ in range(5):
                sync()
                be.lib.grappa_launch_count(1)
                t_h = time.perf_counter()
                job.step()
                host_ms.append(1e3 * (time.perf_counter() - t_h))
                sync()
                launches.append(int(be.lib.grappa_launch_count(1)))
            host_ms.sort()
            extras["launches"] = {"library_kernel_launches_per_step": sorted(launches)[len(launches) // 2], "host_enqueue_ms_per_step": host_ms[len(host_ms) // 2],
                                  "workload": job.name, "writer_head_streams": model.parameter_writer.head_streams,
                                  "note": "kernels launched by libgrappa_hip.so per C2 train step (its own counter; torch adds ~1 fill / copy per "
                                          "output tensor) and the wall time the host needs to issue one step into an empty queue"}
            log(f"launches per step {extras['launches']['library_kernel_launches_per_step']}, host enqueue {extras['launches']['host_enqueue_ms_per_step']:.1f} ms")
        except Exception as e:  # noqa: BLE001
            extras["launches"] = {"error": repr(e)[:300]}
        # ---- the reference's own operating point: batch 32 x 32 conformations (training/config.py:49-52), eager and as a recorded hipGraph
        try:
            from grappa_amd.capture import CapturedTrainStep
            ids32 = workload_molecule_ids("C2-pubchem-b256", seed=0)[:32]
            j32 = Job("C2-pubchem-b256", 32, ids32, seed=0)
            d32, _ = j32.timed(20, 5)
            sync()
            be.lib.grappa_launch_count(1)
            j32.step()
            sync()
            n32 = int(be.lib.grappa_launch_count(1))
            cap = CapturedTrainStep(model, energy, j32.loss_fn, opt, j32.graphs[0], warmup=3)
            for _ in range(5):
                cap()
            sync()
            t_c = time.perf_counter()
            n_rep = 50
            for _ in range(n_rep):
                cap()
            sync()
            d_c = time.perf_counter() - t_c
            extras["b32_train"] = {"value": 32 * n_rep / d_c, "unit": "molecules/s", "ms_per_step": 1e3 * d_c / n_rep, "steps": n_rep, "warmup": 5,
                                   "mode": "hipGraph replay (grappa_amd/capture.py CapturedTrainStep): one graph launch per train step",
                                   "eager": {"value": 32 * 20 / d32, "ms_per_step": 1e3 * d32 / 20, "steps": 20, "warmup": 5,
                                             "library_kernel_launches_per_step": n32},
                                   "final_loss": finite_loss("recorded b32_train", cap.loss), "config": j32.describe(),
                                   "note": "32 molecules x 32 conformations of the C2 molecule range, production model, train mode (dropout on: the "
                                           "recorded step draws fresh masks per replay through the device-side salt), Adam + clip 10; the SAME resident "
                                           "batch every step (shapes are part of a recorded graph: a loader must deliver batches of one shape to use it)"}
            log(f"b32_train: eager {extras['b32_train']['eager']['ms_per_step']:.1f} ms/step, recorded {extras['b32_train']['ms_per_step']:.1f} ms/step "
                f"= {extras['b32_train']['value']:.0f} molecules/s")
            del cap, j32
        except Exception as e:  # noqa: BLE001
            extras["b32_train"] = {"value": None, "error": repr(e)[:400]}
        finally:
            torch.cuda.empty_cache()
        # ---- recorded training on REAL epochs at batch 32: a resident dataset, shuffled batches padded to a handful of shapes, one hipGraph
        # per shape (grappa_amd/trainer.py Trainer(recorded=True), device_dataset.ShapeBuckets) -- every batch different
        try:
            from grappa_amd.datasets import graph_from_pool
            from grappa_amd.device_dataset import DeviceDataset
            from grappa_amd.trainer import Trainer
            n_mols, n_epochs = 1024, 8
            pool_ids = select_molecules(n_mols, seed=11, min_atoms=WORKLOADS["C2-pubchem-b256"][1], max_atoms=WORKLOADS["C2-pubchem-b256"][2])
            t_b = time.perf_counter()
            items = [(graph_from_pool(int(i), n_confs=32, seed=0), "pool") for i in pool_ids]
            ds = DeviceDataset(items, device=dev)
            t_build = time.perf_counter() - t_b
            res = {}
            for mode in ("eager", "recorded"):
                m2 = model_from_config(model_cfg).to(dev)          # (a model object holds its head streams: not copyable; same weights through the state dict)
                m2.load_state_dict(model.state_dict())
                m2.train()
                tr = Trainer(m2, ds, None, batch_size=32, conf_strategy=32, lr=1e-5, gradient_clip_val=10.0, start_qm_epochs=0, warmup_steps=2,
                             energy_weight=1.0, gradient_weight=0.8, param_weight=0.0, recorded=(mode == "recorded"), shape_buckets=4, seed=3)
                ep = []
                for e in range(n_epochs if mode == "recorded" else 3):
                    sync()
                    t_e = time.perf_counter()
                    loss_e = tr.train_epoch(e)
                    sync()
                    ep.append((time.perf_counter() - t_e, loss_e))
                steady = ep[1:]
                n_b = (n_mols // 32) * len(steady)
                res[mode] = {"value": n_mols * len(steady) / sum(t for t, _ in steady), "ms_per_step": 1e3 * sum(t for t, _ in steady) / n_b,
                             "batches": n_b, "epochs_timed": len(steady), "first_epoch_s": ep[0][0], "last_epoch_loss": ep[-1][1]}
                if mode == "recorded":
                    st = tr.recorded_stats
                    res[mode].update({"graphs_recorded": st["graphs_recorded"], "replayed_steps": st["replayed"], "eager_fallback_steps": st["eager"],
                                      "padding_rows_over_real_rows": st["padding_rows"] / max(st["real_rows"], 1),
                                      "bucket_caps": [dict(c) for c in tr._buckets.caps]})
                del tr, m2
                torch.cuda.empty_cache()
            extras["b32_train_epochs"] = dict(res["recorded"], unit="molecules/s", eager=res["eager"], dataset_molecules=n_mols, dataset_build_s=t_build,
                                              mode="Trainer(recorded=True): shuffled epochs over a resident dataset, every batch padded to one of a handful of "
                                                   "shapes by a padding molecule the loss skips, one recorded hipGraph per shape, batches copied into its inputs",
                                              note="the first epoch (bucket calibration + recording the graphs) is reported apart (first_epoch_s); every "
                                                   "timed step is a DIFFERENT batch of 32 molecules x 32 conformations incl. device collate, padding and the copy-in; "
                                                   "production model, train mode, Adam + clip 10")
            log(f"b32_train_epochs: eager {res['eager']['ms_per_step']:.1f} ms/step ({res['eager']['value']:.0f} mol/s), recorded "
                f"{res['recorded']['ms_per_step']:.1f} ms/step = {res['recorded']['value']:.0f} mol/s over {res['recorded']['batches']} batches, "
                f"{res['recorded']['graphs_recorded']} graphs, padding {100 * res['recorded']['padding_rows_over_real_rows']:.1f}%")
            del ds, items
        except Exception as e:  # noqa: BLE001
            import traceback
            extras["b32_train_epochs"] = {"value": None, "error": repr(e)[:400], "trace": traceback.format_exc()[-1200:]}
        finally:
            torch.cuda.empty_cache()
        # ---- Grappa.predict on ONE ~40-atom molecule (grappa.py:36-57): eager and through the cache of recorded forwards
        try:
            import numpy as np
            from grappa_amd import Grappa
            from grappa_amd.datasets import molecule_from_pool
            mol = molecule_from_pool(int(np.argmin(np.abs(pool_atom_counts() - 40))))
            gr = Grappa(model, device="cuda")
            lat = {}
            for mode in ("eager", "recorded"):
                keep_graphs = gr._graphs
                if mode == "eager":
                    gr._graphs = None
                for _ in range(4):
                    gr.predict(mol)
                ts = []
                for _ in range(30):
                    sync()
                    t_p = time.perf_counter()
                    gr.predict(mol)
                    ts.append(1e3 * (time.perf_counter() - t_p))
                ts.sort()
                lat[mode] = {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "p90_ms": ts[int(0.9 * len(ts))]}
                gr._graphs = keep_graphs
            extras["predict_latency_ms"] = {"value": lat["recorded"]["median_ms"], "unit": "ms per Grappa.predict call (median of 30)", "higher_is_better": False,
                                            "recorded": lat["recorded"], "eager": lat["eager"], "atoms": int(mol.to_dgl().num_nodes("n1")),
                                            "note": "host-side graph preparation + copy to the device + forward + copy back + Parameters.from_dgl; "
                                                    "`recorded`: the shape's forward replayed from the cache of hipGraphs (second and later calls on a shape)"}
            log(f"predict: eager {lat['eager']['median_ms']:.2f} ms, recorded {lat['recorded']['median_ms']:.2f} ms")
        except Exception as e:  # noqa: BLE001
            extras["predict_latency_ms"] = {"value": None, "error": repr(e)[:400]}
        finally:
            model.train()
        # BASELINE configs[4] / SURVEY 8(d): single-graph inference latency, ONE 50,046-atom protein graph (19 x T4 lysozyme), eval mode
        try:
            from grappa_amd.datasets import protein_graph_t4
            g5 = protein_graph_t4(19).to(dev)
            model.eval()
            lat = []
            with torch.no_grad():
                for i in range(2 + 5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    model(g5)
                    e1.record()
                    torch.cuda.synchronize()
                    if i >= 2:
                        lat.append(e0.elapsed_time(e1))
            lat.sort()
            extras["c5_inference"] = {"value": lat[len(lat) // 2], "unit": "ms per forward (median of 5 after 2 warm-up)", "higher_is_better": False,
                                      "min_ms": lat[0], "max_ms": lat[-1], "atoms": int(g5.num_nodes("n1")),
                                      "tuples": {lv: int(g5.num_nodes(lv)) for lv in ("n2", "n3", "n4", "n4_improper")},
                                      "atoms_per_s": 1e3 * g5.num_nodes("n1") / lat[len(lat) // 2], "gemm_precision": be.gemm_precision_name,
                                      "config": "C5: ONE graph of 19 disjoint all-atom T4 lysozymes, production GrappaModel (keyed init), eval mode, no_grad; "
                                                "parameters vs the oracle: tests/test_gpu_e2e.py::test_c5_protein_size_inference_matches_oracle"}
            log(f"c5_inference: {extras['c5_inference']['value']:.1f} ms per forward")
            del g5
        except Exception as e:  # noqa: BLE001
            extras["c5_inference"] = {"value": None, "error": repr(e)[:300]}
        finally:
            model.train()
            torch.cuda.empty_cache()

    # N > 1: what the collective layer actually saw, so that the first real multi-GPU run checks itself
    dist_info = None
    if args.full and world > 1:
        me = {"rank": rank, "local_rank": local_rank, "device_index": torch.cuda.current_device() if on_gpu else None, "pid": os.getpid(),
              "device_name": torch.cuda.get_device_name() if on_gpu else "cpu",
              "device_uuid": str(getattr(torch.cuda.get_device_properties(dev), "uuid", "")) if on_gpu else None}
        everyone = [None] * world
        dist.all_gather_object(everyone, me)
        distinct = distinct_devices(everyone, world, enforce=on_gpu and args.dist_backend == "nccl")
        # overlapped vs post-backward reduction of the SAME gradients, bit for bit: the same batch and dropout seeds through both
        # orders, no optimiser step in between; the two orders cut the buffer alike (dist.BucketedGradReducer.finish)
        n_check = min(args.steps, 10)
        mism, t_modes = 0, {}
        for mode in (False, True):
            red2 = BucketedGradReducer(model, flat, overlap=mode)
            grads = []
            sync()
            dist.barrier()
            t_m = time.perf_counter()
            for s_ in range(n_check):
                ops.manual_seed(777 + 13 * s_ + rank)
                flat.zero_grad()
                red2.begin_step(len(job.graphs))
                for g_ in job.graphs:
                    for lvl in ("n2", "n3", "n4", "n4_improper"):
                        for k_ in ("k", "eq"):
                            g_.nodes[lvl].data.pop(k_, None)
                    job.loss_fn(energy(model(g_))).backward()
                red2.finish()
                if s_ < 3:
                    grads.append(flat.grad.clone())
            sync()
            t_modes[mode] = 1e3 * (time.perf_counter() - t_m) / n_check
            if mode:
                mism = sum(int(not torch.equal(a_, b_)) for a_, b_ in zip(grads, kept))
            kept = grads
        model.on_heads_backward_done = reducer._on_heads_done if reducer.overlap else None
        mm = torch.tensor([mism], device=dev)
        dist.all_reduce(mm, op=dist.ReduceOp.SUM)
        dist_info = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "ranks": everyone, "distinct_devices": distinct,
                     "rccl_version": (".".join(map(str, torch.cuda.nccl.version())) if on_gpu and hasattr(torch.cuda, "nccl") else None),
                     "env": {k_: v_ for k_, v_ in os.environ.items() if k_.startswith(("NCCL_", "RCCL_", "HSA_ENABLE_IPC"))},
                     "allreduce_overlap_default": reducer.overlap,
                     "allreduce_bit_check": {"steps_compared": 3, "mismatching_steps_summed_over_ranks": int(mm),
                                             "ms_per_step_post_backward": t_modes[False], "ms_per_step_overlapped": t_modes[True],
                                             "note": "gradient buffers after the all-reduce, heads' bucket sent from inside the backward pass vs both "
                                                     "buckets after it, same batch and dropout seeds, torch.equal; untimed forward+backward+all-reduce "
                                                     "loops of both orders beside it (no optimiser step)"}}
        log(f"dist self-check: {dist_info['backend']} world {dist_info['world_size']}, {distinct} distinct devices, overlap bit check mismatches {int(mm)}, "
            f"post-backward {t_modes[False]:.1f} ms vs overlapped {t_modes[True]:.1f} ms per forward+backward+all-reduce")

    # N > 1, strong scaling: the same-workload N = 1 point.  Rank 0 alone runs the WHOLE global batch (chunks of --chunk molecules, gradients
    # accumulated, one optimiser step, no collective) while the other ranks wait at the barrier that follows; last, so that nothing
    # measured above sees rank 0's parameters drift from the others'
    scaling_ref = None
    if args.full and world > 1 and strong and not args.no_scaling_reference:
        if rank == 0:
            try:
                total = job.global_batch
                _, lo_, hi_, _ = WORKLOADS[job.name]
                all_ids = workload_molecule_ids(job.name, seed=0) if total == WORKLOADS[job.name][0] else select_molecules(total, seed=0, min_atoms=lo_, max_atoms=hi_)
                jr = Job(job.name, total, all_ids, seed=0)
                jr.solo = True
                ref_steps = 3 if total > 2048 else 5
                d_r, _ = jr.timed(ref_steps, 1)
                scaling_ref = {"value": total * ref_steps / d_r, "unit": "molecules/s", "ms_per_step": 1e3 * d_r / ref_steps, "steps": ref_steps, "warmup": 1,
                               "n_gpus": 1, "config": jr.describe(),
                               "note": "the same global batch on rank 0's GPU alone, measured in this run right after the N-rank measurement"}
                log(f"single-GPU reference of the same global batch: {scaling_ref['ms_per_step']:.1f} ms/step = {scaling_ref['value']:.0f} molecules/s")
                del jr
            except Exception as e:  # noqa: BLE001
                scaling_ref = {"value": None, "error": repr(e)[:300]}
        dist.barrier()

    if rank == 0:
        # HBM traffic per launch of the dominant kernel: PMC counters cannot be read from inside the process; the committed
        # rocprofv3 --pmc summary of this same command (tools/pmc_traffic.py -> profiles/pmc_traffic_c2.json) is reported -- only
        # while the kernel sources it was measured on are the ones running
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic_c2.json")
        if roof is not None and job.name == "C2-pubchem-b256" and os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                if tj.get("kernel_source_hash") == kernel_source_hash():
                    # per product call, like `achieved`: the bytes of every kernel the products launch (main, grouped, split-K reduce,
                    # row-maxima passes) per step, over the product calls per step
                    roof["traffic"] = tj["families"]["dense_products"]["hbm_bytes_per_step"] / max(roof["launches_per_step"], 1.0)
                    roof["traffic_source"] = ("profiles/pmc_traffic_c2.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, "
                                              "gfx950 corrections of MI355X_MICROARCH.md; HBM bytes of all kernels of the dense products per "
                                              "step / product calls per step; same kernel sources)")
                else:
                    roof["traffic_source"] = "profiles/pmc_traffic_c2.json was measured on other kernel sources: not reported"
            except Exception:
                pass
        cfg = job.describe()
        cfg.update({"parallelism": f"dp{world}", "world_size": dist.get_world_size() if world > 1 else 1, "dist_backend": dist.get_backend() if world > 1 else None,
                    "allreduce_ms_per_step": allreduce_ms if world > 1 else None, "allreduce_bytes": 4 * flat.numel if world > 1 else None,
                    "allreduce_overlap": reducer.overlap if world > 1 else None,
                    "heads_bucket_lead_ms": getattr(job, "heads_bucket_lead_ms", None) if world > 1 else None,
                    "writer_head_streams": head_streams})
        out = {
            "metric": "molecules/sec (train step, energy+force loss)", "value": job.global_batch * args.steps / dt, "unit": "molecules/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
            "scaling": ("strong" if strong else "weak") if world > 1 else None, "vs_baseline": None, "dtype": "bf16" if args.act_dtype == "bf16" else "f32", "data": "synthetic",
            "config": cfg,
            "gemm_arithmetic": {"default": getattr(be, "gemm_precision_name", None),
                                "note": "inputs, outputs, accumulation and every non-GEMM kernel are fp32; f32_f16x3 scales every row of an "
                                        "fp32 operand by a power of two (largest magnitude -> [2^14, 2^15)), splits it into 2 fp16 pieces "
                                        "(24 significant bits) and sums the 3 largest partial products on the fp16 matrix cores; f32_bf16x6 "
                                        "(the previous default) = 3 bf16 pieces, 6 products.  Error vs a float64 product <= that of the native "
                                        "fp32 MFMA for both (tests/test_gpu_ops.py::test_gemm_precision_modes, tests/test_gpu_f16x3.py); "
                                        "end-to-end parity: tests/test_gpu_e2e.py, tests/test_gpu_configs.py",
                                "native_f32_mfma": alt.get("f32"), "f32_bf16x6": alt.get("f32_bf16x6"), "backward_reduced": bwd, "weight_planes": wpl},
            "roofline": roof, "roofline_gat": gat, "ms_per_step_instrumented": ms_instr, "final_loss": final_loss,
            "writer_heads_other_stream_setting": heads_alt,
        }
        out.update(extras)
        # where ONE recorded hipGraph replay per step (same kernels, same optimiser step, fresh dropout masks per replay;
        # grappa_amd/capture.py CapturedTrainStep, replay == eager step in tests/test_gpu_capture.py) is at least 3 % faster than the eager
        # step, IT is the headline's mode -- K replays between two synchronisations after the eager warm-up and timing above -- and the
        # eager figure stays beside it
        rec = extras.get("c2_recorded") if (world == 1 and workload == "C2-pubchem-b256" and args.act_dtype == "f32") else None
        out["step_mode"] = "eager (one Python-issued launch sequence per step)"
        if isinstance(rec, dict) and rec.get("value") and rec.get("steps") == args.steps and rec["ms_per_step"] <= 0.97 * out["ms_per_step"]:
            out["eager"] = {"value": out["value"], "ms_per_step": out["ms_per_step"], "steps": args.steps, "warmup": args.warmup}
            out["value"], out["ms_per_step"] = rec["value"], rec["ms_per_step"]
            out["step_mode"] = rec["mode"]
        # the driver's record keeps `config` verbatim and only the NAMES of other top-level keys: the numbers the extras stand for travel in
        # config.extras too (value, unit, ms per step, the products' roofline fraction) -- VERDICT r4 item 7
        def _brief(e):
            if not isinstance(e, dict):
                return e
            b = {k: e[k] for k in ("value", "unit", "ms_per_step", "steps", "error", "library_kernel_launches_per_step", "host_enqueue_ms_per_step") if k in e}
            r = e.get("roofline")
            if isinstance(r, dict):
                b["roofline_frac"], b["roofline_achieved"], b["roofline_peak"], b["roofline_traffic"] = r.get("frac"), r.get("achieved"), r.get("peak"), r.get("traffic")
            if isinstance(e.get("eager"), dict):
                b["eager_ms_per_step"] = e["eager"].get("ms_per_step")
            return b
        out["config"]["extras"] = {k: _brief(v) for k, v in extras.items()}
        if dist_info is not None:
            out["dist"] = dist_info
        if scaling_ref is not None:
            out["strong_scaling_reference"] = scaling_ref
            out["scaling_factor"] = (out["value"] / scaling_ref["value"]) if scaling_ref.get("value") else None
        out["cpu_baseline"] = cpu_base
        out["full"] = args.full
        if not args.full:
            # a plain run measures the headline alone: the fields that only --full measures are left out of its line
            for k in ("roofline", "roofline_gat", "ms_per_step_instrumented", "writer_heads_other_stream_setting", "cpu_baseline"):
                out.pop(k)
            for k in ("native_f32_mfma", "f32_bf16x6", "backward_reduced", "weight_planes"):
                out["gemm_arithmetic"].pop(k)
            out["config"].pop("extras")
        if dumped is not None:
            out["dumped_outputs"] = {"dir": args.dump_outputs, "shapes": dumped}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
