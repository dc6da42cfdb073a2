"""Times `Evaluator.pool(n_bootstrap)` over a synthetic store on one GPU: `--datasets` datasets x `--mols` molecules, stepped in batches of
256 molecules x 32 conformations of seeded random numbers (the evaluator never looks at where its inputs come from).

    python tools/evaluator_pool_bench.py [--datasets 8 --mols 2000 --n-bootstrap 1000 --repeats 5] > profiles/evaluator_pool_bootstrap.txt

Prints one JSON line: the whole `pool()` call by HIP events (host draw of the index table, uploads, kernels, the read-back), the host
draw alone by the host clock, and the two launches per index chunk alone by HIP events over tables that are already on the device.
A measurement path: without a GPU it fails."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--datasets", type=int, default=8)
    ap.add_argument("--mols", type=int, default=2000)
    ap.add_argument("--n-bootstrap", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from grappa_amd import _lib
    from grappa_amd.backend import get_backend
    from grappa_amd.evaluation import Evaluator, bootstrap_indices
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    ev = Evaluator()
    M, B, C = a.datasets * a.mols, 256, 32
    t0 = time.perf_counter()
    for first in range(0, M, B):
        nb = min(B, M - first)
        counts = torch.randint(10, 60, (nb,), generator=g)
        N = int(counts.sum())
        ptr = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).int().to(dev)
        e_ref, g_ref = torch.randn(nb, C, generator=g) * 5, torch.randn(N, C, 3, generator=g) * 20
        data_g = {"energy_ref": e_ref.to(dev), "energy": (e_ref + torch.randn(nb, C, generator=g)).to(dev),
                  "is_dummy": (torch.arange(C)[None, :] >= torch.randint(8, C + 1, (nb, 1), generator=g)).float().to(dev)}
        data_n1 = {"gradient_ref": g_ref.to(dev), "gradient": (g_ref + torch.randn(N, C, 3, generator=g) * 3).to(dev)}
        graph = types.SimpleNamespace(plan=lambda p=types.SimpleNamespace(B=nb, N=N, atom_molptr=ptr): p,
                                      nodes={"g": types.SimpleNamespace(data=data_g), "n1": types.SimpleNamespace(data=data_n1)})
        ev.step(graph, [f"ds{(first + j) % a.datasets}" for j in range(nb)])
    torch.cuda.synchronize()
    t_steps = time.perf_counter() - t0

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e), out

    ev.pool(n_bootstrap=8)                                                  # code objects loaded, allocator warm
    pool_ms = [timed(lambda: ev.pool(n_bootstrap=a.n_bootstrap, seed=0))[0] for _ in range(a.repeats)]
    names, counts, tables = ev._table()
    draw_ms = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        idx = bootstrap_indices(counts, a.n_bootstrap, 0)
        draw_ms.append(1e3 * (time.perf_counter() - t0))
    be = get_backend()
    idx_dev = torch.from_numpy(idx).to(dev)
    ds_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev)
    out = [torch.zeros((a.n_bootstrap, len(names), len(_lib.EVAL_METRICS)), dtype=torch.float64, device=dev)] + \
          [torch.zeros((len(names), len(_lib.EVAL_METRICS)), dtype=torch.float64, device=dev) for _ in range(2)]
    launch = lambda: be.eval_bootstrap(tables[0], ds_ptr, idx_dev, a.n_bootstrap, 0, a.n_bootstrap, *out)      # noqa: E731
    launch()
    kernel_ms = [timed(launch)[0] for _ in range(a.repeats)]
    med = lambda v: float(np.median(v))                                     # noqa: E731
    print(json.dumps({"what": "Evaluator.pool", "device": torch.cuda.get_device_name(0), "datasets": a.datasets, "molecules": M,
                      "conformations_per_batch_row": C, "n_bootstrap": a.n_bootstrap, "repeats": a.repeats,
                      "pool_ms_hip_events": {"median": med(pool_ms), "all": [round(x, 3) for x in pool_ms]},
                      "of_which_host_index_draw_ms_host_clock": {"median": med(draw_ms), "all": [round(x, 3) for x in draw_ms]},
                      "bootstrap_and_spread_launches_ms_hip_events": {"median": med(kernel_ms), "all": [round(x, 4) for x in kernel_ms]},
                      "index_table_bytes": int(idx.nbytes), "moment_table_bytes": int(tables[0].numel() * 8),
                      "steps_s_host_clock_incl_input_generation": round(t_steps, 3)}))


if __name__ == "__main__":
    main()
