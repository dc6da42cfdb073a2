"""Data parallelism by molecule: one process per GPU, one RCCL all-reduce of the flat gradient buffer.

The reference is single-device.  Molecules never interact (block-diagonal graph,
loss = mean over molecules), so the batch is dealt to the ranks after sorting by size (round-robin,
balances tuples per GPU), every rank runs the same kernels on its shard with the loss scaled by
1/B_global, and the gradients are summed over xGMI: one collective of the flat buffer (`all_reduce_gradients`), or two
buckets, the first optionally overlapped with the rest of the backward pass (`BucketedGradReducer`).
"""
import os
from typing import List, Sequence

import torch
import torch.distributed as dist

from . import settings


def init_process_group_from_env(backend: str = None) -> int:
    """torchrun-style env (RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT, LOCAL_RANK) -> world size."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and not dist.is_initialized():
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"      # "nccl" is RCCL on ROCm
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend=backend)
    return world


def shard_indices(sizes: Sequence[int], world_size: int, rank: int) -> List[int]:
    """indices of the molecules of `rank`: sort by size (descending, stable) and deal round-robin."""
    order = sorted(range(len(sizes)), key=lambda i: (-int(sizes[i]), i))
    return sorted(order[rank::world_size])


def all_reduce_gradients(flat_grad: torch.Tensor) -> None:
    """sum over ranks; each rank's loss is already scaled by 1/B_global (MolwiseLoss.global_batch_size)."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(flat_grad, op=dist.ReduceOp.SUM)


class BucketedGradReducer:
    """Gradient all-reduce in two buckets of the flat buffer, the first optionally overlapped with the backward pass.

    The backward pass finishes the writer heads (55 % of the parameters: 22.2 M of 40.8 M in the production model) before it enters
    the GNN (18.6 M).  The moment the gradient of the atom embedding `h` is complete (`GrappaModel.on_heads_backward_done`) every writer
    gradient is final, so its slice of the flat buffer is handed to an ASYNCHRONOUS all-reduce (RCCL runs it on its own stream,
    ordered after the compute stream's work so far) while the GNN backward keeps the matrix cores busy; `finish()` reduces the
    GNN slice and waits for both.  Same sums as `all_reduce_gradients`, so results are identical."""

    def __init__(self, model, flat, overlap=None):
        self.flat = flat
        self.model = model
        self.head_range = flat.range_of(model.parameter_writer)
        self._work = []
        self._heads_sent = False
        self._passes_left = 1          # backward passes still to come before the step's gradients are final (begin_step)
        self.time_events = None        # bench.py sets a list: HIP events around the collectives of both buckets
        # overlap (OPT-IN: GRAPPA_OVERLAP_ALLREDUCE=1 or overlap=True; default: both buckets after backward()): the writer-head bucket is
        # sent from inside the backward pass, the moment the gradient of h is complete -- ops.SplitHeadsFn, which runs on the caller's
        # stream behind every head's stream, so the collective (RCCL orders its own stream behind the caller's at the call) sees final
        # values.  Same sums either way on gloo (tests/test_host_train.py holds the two bit-equal).  Why opt-in: RCCL's
        # reduction kernels would then run on their own queue BESIDE this library's MFMA products of the GNN's backward pass, and
        # DESIGN.md section 6 documents a platform hazard for exactly that pairing -- a packed-fp32 instruction returning wrong dwords
        # while MFMA wavefronts of another queue share the SIMD.  This library is compiled without packed fp32; librccl is not ours to
        # compile, and no run on two or more GPUs has compared overlapped and post-backward reductions bit for bit yet
        # (bench.py --gpus N reports `allreduce_bit_check` when both orders are run: see there).
        self.overlap = settings.read("overlap") if overlap is None else bool(overlap)
        model.on_heads_backward_done = self._on_heads_done if self.overlap else None

    @staticmethod
    def _active() -> bool:
        return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1

    @staticmethod
    def _flush_queued_wgrads() -> None:
        from .backend import get_backend
        be = get_backend()
        if hasattr(be, "flush_wgrads"):
            be.flush_wgrads()                      # weight gradients still queued for a grouped launch belong in the buffer first

    def begin_step(self, backward_passes: int = 1) -> None:
        """declare how many backward passes accumulate into the gradient buffer before `finish()` (a batch processed in chunks): the
        writer-head bucket is sent from inside the LAST of them only.  Without this call every step is one backward pass."""
        self._passes_left = int(backward_passes)

    def _on_heads_done(self) -> None:
        self._passes_left -= 1
        if self._passes_left > 0:
            return
        if self._active() and not self._heads_sent:
            self._flush_queued_wgrads()
            a, b = self.head_range
            if self.time_events is not None and self.flat.grad.is_cuda:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record()
                self.time_events.append(("heads_sent", e0, None))        # (bench.py: when the overlapped bucket left, relative to finish())
            self._work.append(dist.all_reduce(self.flat.grad[a:b], op=dist.ReduceOp.SUM, async_op=True))
            self._heads_sent = True

    def finish(self) -> None:
        """call after loss.backward(): reduces what is left and waits for every bucket"""
        self._flush_queued_wgrads()
        if self._active():
            a, b = self.head_range
            # the SAME buckets whether the heads' one left from inside the backward pass or leaves here: a collective's summation order
            # depends on how the buffer is cut, so only equal cuts make the two orders comparable bit for bit (bench.py's N > 1 check)
            todo = [(0, a), (b, self.flat.numel)] if self._heads_sent else [(a, b), (0, a), (b, self.flat.numel)]
            t0 = self.time_events is not None and self.flat.grad.is_cuda
            if t0:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            for lo, hi in todo:
                if hi > lo:
                    self._work.append(dist.all_reduce(self.flat.grad[lo:hi], op=dist.ReduceOp.SUM, async_op=True))
            for w in self._work:
                w.wait()
            if t0:
                e1.record()
                self.time_events.append(("finish", e0, e1))
        self._work = []
        self._heads_sent = False
        self._passes_left = 1
