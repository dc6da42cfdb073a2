"""GPU: the grouped weight-gradient launch (grappa_gemm_f32_grouped: header, product grid, reduction) timed through the C ABI with HIP
events on one queue, on groups shaped like those of a C2 step: the weight gradients of one transformer layer of the four writer heads
(C2 token counts; 16 products of 1536 x 512 and 512 x 512) with the operands as fp32 rows, A / B / both in the pair format and all four
mixed in one launch, and the GNN's fp32 group (8,233 atom rows).  Random normal operands (zeros or constants flatter the clock).

    python tools/wgrad_group_bench.py [--rounds 3] [--iters 10] [--libs name=path,name=path,...] [--out FILE]

Prints, per group and library, the time of one call in every round and the FLOP rate of the best.  --libs adds other builds of
libgrappa_hip.so (the -D legs of an A/B, the parent commit's library) to the loaded one: all of them run in ONE process on the same
operands, a round of each in turn, which is what makes their difference readable beside the run-to-run spread.
"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from grappa_amd import _lib  # noqa: E402

TOKENS = (17158, 44325, 83328, 28248)
LAYER = ((1536, 512), (512, 512), (512, 512), (512, 512))
GNN = ((512, 2048), (2048, 512), (512, 512), (512, 512), (512, 512), (512, 512))
ATOMS = 8233


def _bits(t):
    return t.float().abs().contiguous().view(torch.int32)


def build(lib, shapes, fmts, gen):
    """shapes: (T, M, N) per member; fmts: "f32" | "pa" | "pb" | "pab" per member -> (descriptor array, workspace, FLOPs, what stays alive)"""
    st = torch.cuda.current_stream().cuda_stream
    arr = (_lib.GemmDesc * len(shapes))()
    keep, flops = [], 0.0
    for d, (T, M, N), fmt in zip(arr, shapes, fmts):
        dz, x = torch.randn((T, M), generator=gen, device="cuda"), torch.randn((T, N), generator=gen, device="cuda")
        dw, db = torch.zeros((M, N), device="cuda"), torch.zeros((M,), device="cuda")
        d.M, d.N, d.K, d.accumulate, d.precision, d.amax_bcast = M, N, T, 1, _lib.GEMM_PRECISIONS["f32_f16x3"], 3
        ptrs = {}
        for which, t, cols in (("a", dz, M), ("b", x, N)):
            tmax = _bits(t.abs().amax().reshape(1))
            keep += [t, tmax]
            if which in fmt[1:]:
                rowmax = _bits(t.abs().amax(1))
                pairs = torch.zeros((T, 2 * cols), dtype=torch.float16, device="cuda")
                assert lib.grappa_split_pairs_f32(st, T, cols, t.data_ptr(), t.stride(0), rowmax.data_ptr(), pairs.data_ptr(), pairs.stride(0), 0) == 0
                keep += [rowmax, pairs]
                ptrs[which] = (pairs.data_ptr(), pairs.stride(0), 1, rowmax.data_ptr(), tmax.data_ptr())
            else:
                ptrs[which] = (t.data_ptr(), t.stride(0), 0, None, tmax.data_ptr())
        d.A, d.lda, d.a_planes, d.a_rowmax, d.a_amax = ptrs["a"]
        d.B, d.ldb, d.b_planes, d.b_rowmax, d.b_amax = ptrs["b"]
        d.C, d.ldc, d.a_colsum = dw.data_ptr(), dw.stride(0), db.data_ptr()
        keep += [dw, db]
        flops += 2.0 * T * M * N
    ws = torch.empty(int(lib.grappa_gemm_f32_grouped_workspace_bytes(arr, len(shapes))) + 256, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return arr, ws, flops, keep


def groups():
    heads = [(T, M, N) for T in TOKENS for M, N in LAYER]
    cyc = ("f32", "pa", "pb", "pab")
    yield "heads16 f32", heads, ["f32"] * 16
    yield "heads16 pa", heads, ["pa"] * 16
    yield "heads16 pb", heads, ["pb"] * 16
    yield "heads16 pab", heads, ["pab"] * 16
    yield "heads16 mixed", heads, [cyc[i % 4] for i in range(16)]
    yield "heads16 pb+pab", heads, [("pb", "pab")[i % 2] for i in range(16)]
    yield "gnn6 f32", [(ATOMS, M, N) for M, N in GNN], ["f32"] * len(GNN)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--libs", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wgrad_group_bench: needs a GPU")
    lib = _lib.load()
    legs = [("loaded", lib)]
    for item in filter(None, args.libs.split(",")):
        name, path = item.split("=", 1)
        other = C.CDLL(os.path.abspath(path))
        for fn in ("grappa_gemm_f32_grouped", "grappa_gemm_f32_grouped_workspace_bytes"):
            getattr(other, fn).restype, getattr(other, fn).argtypes = _lib.SIGNATURES[fn]
        legs.append((name, other))
    gen = torch.Generator(device="cuda").manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    lines = [f"# ms per grouped call (header + product + reduction), {args.rounds} rounds of {args.iters} calls, the libraries in turn; loaded = {_lib.LIB_PATH}"]
    for name, shapes, fmts in groups():
        arr, ws, flops, keep = build(lib, shapes, fmts, gen)
        ms = {leg: [] for leg, _ in legs}
        for leg, l in legs:
            for _ in range(3):
                assert l.grappa_gemm_f32_grouped(st, arr, len(shapes), ws.data_ptr(), ws.numel() - 256) == 0, leg
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for leg, l in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    l.grappa_gemm_f32_grouped(st, arr, len(shapes), ws.data_ptr(), ws.numel() - 256)
                e1.record()
                torch.cuda.synchronize()
                ms[leg].append(e0.elapsed_time(e1) / args.iters)
        for leg, _ in legs:
            m = ms[leg]
            lines.append(f"{name:16s} {leg:12s} " + " ".join(f"{v:8.4f}" for v in m) + f"   best {min(m):8.4f} spread {max(m) - min(m):7.4f} ms  {flops / min(m) / 1e9:6.1f} TFLOP/s")
            print(lines[-1], flush=True)
        del arr, ws, keep
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
