"""Every setting of the engine, as one table: where it lives, which environment variable sets it, its default and why.

libgrappa_hip.so reads no environment; the Python package reads it HERE only (`read`).  Each owner fills its plain attributes from the table at
the time it always did -- `HipBackend.__init__` and the parameter writer at construction, `ops` and `_lib` at import, the `host` entries
where they are used -- and the hot path reads those attributes.  `launch_stamp` is the value of every setting that a recorded hipGraph has
baked into its launches: the stamps of capture.CapturedForward and trainer.Trainer are derived from it, so a setting added to the table is in
both.  `python -m grappa_amd.settings` prints the table.
"""
import os
from typing import Callable, NamedTuple, Optional, Union


class Setting(NamedTuple):
    name: str                        # the attribute of its owner
    owner: str                       # "backend" (HipBackend) | "ops" (module grappa_amd.ops) | "writer" (model.parameter_writer) | "host" (read where used)
    env: Optional[str]               # None: state without a variable that is baked into the launches all the same
    kind: Union[str, Callable]       # "flag" | "int" | "str" | a function of the variable's text
    default: object
    doc: str
    setter: Optional[str] = None     # method of the owner that takes the value instead of a plain assignment


def _or_none(s):
    return s or None


def _gb_to_bytes(s):
    return int(float(s) * 2 ** 30)


def _tail_pin(s):
    return None if s == "" else s != "0"


def _native_plan(s):
    return s not in ("numpy", "0", "")


TABLE = (
    Setting("gemm_precision_name", "backend", "GRAPPA_GEMM_PRECISION", "str", "f32_f16x3",
            "arithmetic of the dense products (include/grappa_hip.h GRAPPA_GEMM_*): \"f32_f16x3\" = fp32 operands, every row scaled by a "
            "power of two, split into two fp16 pieces (3 partial products on the fp16 matrix cores, fp32 accumulation); \"f32_bf16x6\" = "
            "three bf16 pieces, 6 products (the default until round 2).  Both are at least as close to the exact product as the native "
            "fp32 MFMA (tests/test_gpu_ops.py::test_gemm_precision_modes) at ~2.3x / ~1.7x its speed; \"f32\" = native fp32 MFMA",
            "set_gemm_precision"),
    Setting("gemm_precision_bwd_name", "backend", "GRAPPA_GEMM_PRECISION_BWD", _or_none, None,
            "optional, OFF by default: a separate arithmetic for the products of the BACKWARD pass (dgrad / wgrad layouts), e.g. "
            "\"bf16x3\" (two bf16 pieces per operand, 2^-16 per product).  The forward pass -- parameters, energies, forces, loss -- is "
            "untouched by it; the reference itself trains with torch.set_float32_matmul_precision('medium') (training/trainrun.py:3).",
            "set_gemm_precision_bwd"),
    Setting("defer_wgrads", "backend", "GRAPPA_DEFER_WGRADS", "flag", True,
            "weight-gradient products of a backward pass are queued and launched together (grappa_gemm_f32_grouped): alone, each must "
            "cut its K (= tokens) 10 - 32 ways to fill the chip and pays for that many partial tiles per output tile"),
    Setting("defer_ln", "backend", "GRAPPA_DEFER_LN_REDUCTIONS", "flag", True,
            "tuning: 0 = reduce every LayerNorm's parameter gradients at once"),
    Setting("wgrad_queue_bytes", "backend", "GRAPPA_WGRAD_QUEUE_GB", _gb_to_bytes, 12 * 2 ** 30,
            "bytes of operands the queue of deferred weight-gradient products may keep alive (the variable is in GB)"),
    Setting("inference_pairs", "backend", "GRAPPA_INFERENCE_PAIRS", "flag", True,
            "inference (no gradient asked for): LayerNorm and the tuple attention write the A operand of the product behind them in the pair "
            "format and the product reads operands split once (csrc/gemm_pairs.hip) -- same bits as the fp32-operand product of the same K cuts"),
    Setting("training_pairs", "backend", "GRAPPA_TRAINING_PAIRS", "flag", True,
            "training (round 4): the same producers write pairs ONLY, the dropout backward too, and the weight-gradient products read pairs "
            "(C ABI 8: token rows moved onto the tensor's scale inside the kernel) -- no fp32 copy of a normalised activation exists any more"),
    Setting("group_launches", "backend", "GRAPPA_GROUP_LAUNCHES", "flag", True,
            "the same product of the four writer heads as ONE launch (gemm_group); GRAPPA_GROUP_LAUNCHES=0: one by one"),
    Setting("amax_parts", "backend", "GRAPPA_AMAX_PARTS", "flag", False,
            "opt-in (GRAPPA_AMAX_PARTS=1): the row maxima of a product's output stay the per-segment partials its epilogue writes and the "
            "products that read the tensor combine them (C ABI 8 out_amax_parts / a_amax_nseg: 62 combine launches per C2 step gone).  Measured "
            "SLOWER: 37.4 against 35.9 ms per C2 step -- every workgroup of the consumer re-reads 16 partials per row in its prologue and "
            "epilogue, which costs more than the one small launch it replaces (profiles/r4_amax_parts_ab.txt) -- hence not the default"),
    Setting("fuse_ln_drop", "backend", "GRAPPA_FUSE_LN_DROP", "flag", True,
            "the dropout backward of a layer's two dropouts written by the LayerNorm backward that produces their input (C ABI 9): 30 of the "
            "40 act_dropout_bwd launches of a C2 step gone with the read of the gradient they made.  GRAPPA_FUSE_LN_DROP=0: launches of their own"),
    Setting("pairs_min_rows", "backend", "GRAPPA_PAIRS_MIN_ROWS", "int", 12288,
            "training_pairs: tables with fewer rows stay fp32 (the GNN's 8,233 atom rows at C2: the two-workgroup pair kernel gains nothing there; "
            "HipBackend.training_pairs_ok)"),
    Setting("backward_pairs", "backend", "GRAPPA_BACKWARD_PAIRS", "flag", False,
            "the dropout backward writing ITS rows (gradients) as pairs too: the input-gradient products behind gain (pair kernel), the weight-"
            "gradient products lose a little (a pair-format A operand costs 3 - 5 %, a pair-format B operand gains 9 %: tools/wgrad_pairs_bench.py) "
            "Measured on the C2 step: 34.9 ms with the forward producers' pairs only, 35.0 - 35.1 with the backward producers' too, 35.35 without "
            "pairs (profiles/r4_backward_pairs_ab.txt) -- hence off by default"),
    Setting("weight_pairs_min_rows", "backend", "GRAPPA_WPAIRS_MIN_ROWS", "int", 24000,
            "round 5: forward / input-gradient products whose A operand reaches them as fp32 rows (the second product of a feed-forward, every "
            "input-gradient product) read the WEIGHT from its pairs and split A's fragments in registers (csrc/gemm_wpairs_il.hip: the pinned "
            "pipeline, two workgroups per CU) where that beats the fp32-operand kernel: tables of at least `wpairs_min_rows` rows (on the C2 shapes "
            "1.08 - 1.12 x at >= 28 k rows, slower than the 512-thread kernel on one round of tiles: profiles/r5_pairs_lab_v4.txt)"),
    Setting("_tails", "backend", None, "flag", None,
            "tail launches of the products: True / False, None = the library's default (grappa_gemm_desc.plan_tail)"),
    Setting("plan_override", "backend", None, "str", None,
            "tuning / tests: (cfg or -1, nsplit or 0, tail: -1 model, 0 never, 1 forced) applied to every product"),
    Setting("splitk_reduce", "backend", None, "int", 0,
            "tests: 0 library default, 1 a reduction launch, 2 inside the product's launch"),
    Setting("_tails_pinned", "backend", "GRAPPA_PLAN_TAILS", _tail_pin, None,
            "the value is the pin: True / False = tail launches on / off whatever the model asks for (GRAPPA_PLAN_TAILS=1 / 0), None (unset or "
            "empty) = the model's choice; the attribute says whether a pin holds", "pin_tail_launches"),
    Setting("gnn_tails", "backend", "GRAPPA_GNN_TAILS", "flag", False,
            "tuning: tail launches for the GNN's products while the heads run without"),
    Setting("wgrads_aside", "backend", "GRAPPA_WGRADS_ASIDE", "flag", True,
            "tuning: 0 = every queued product waits for the end of the pass"),
    Setting("weight_planes", "backend", "GRAPPA_WEIGHT_PLANES", "flag", False,
            "opt-in (GRAPPA_WEIGHT_PLANES=1): forward and dgrad products read the weight matrix from its bf16 planes (split once per "
            "optimiser step, both orientations) through LDS-DMA instead of re-splitting it in every workgroup of every launch "
            "(csrc/gemm_planes.hip gemm_wplanes_kernel).  Results are bit-identical to the default; measured speed is the same within "
            "+-3 % (DESIGN.md section 6), which is why it is not the default."),
    Setting("fused_writer_layer", "backend", "GRAPPA_FUSED_WRITER_LAYER", "flag", True,
            "round 6: a transformer layer of a writer head as ONE kernel (csrc/writer_layer.hip, grappa_writer_head_fwd) where its shape allows: "
            "bf16 storage configuration, 512 features, 8 heads.  GRAPPA_FUSED_WRITER_LAYER=0: the unfused sequence (A/B, tests)"),
    Setting("fused_writer_layer_bwd", "backend", "GRAPPA_FUSED_WRITER_LAYER_BWD", "flag", True,
            "... and its backward pass: the input-gradient chain as one kernel (grappa_writer_head_bwd); 0: the unfused backward over the tensors "
            "the fused forward saved"),
    Setting("fused_first_layer", "backend", "GRAPPA_FUSED_FIRST_LAYER", "flag", True,
            "... and the first layer of the angle / proper heads (ops.ProjFirstLayerFn: LayerNorm + q | k | v on (atom, position) rows) through the same "
            "kernels in their gather mode; 0: the unfused sequence behind the table-level products"),
    Setting("first_layer_indexed", "backend", "GRAPPA_FIRST_LAYER_INDEXED", "flag", True,
            "the unfused fp32 first layer (ops.ProjFirstLayerFn) keeps q | k | v on the table: the attention kernels read a token's row through the "
            "table index (grappa_seqattn_*_idx_f32), and the token sums of the backward pass run with several rows in flight and write the row maxima "
            "of what they sum (grappa_tuple_gather_bwd2_f32).  GRAPPA_FIRST_LAYER_INDEXED=0: the token-level copy of q | k | v and the one-row-at-a-time "
            "sums -- the reference of the equality tests and the other leg of tools/first_layer_ab.sh"),
    Setting("wgrad_column_maxima", "backend", "GRAPPA_WGRAD_COLUMN_MAXIMA", "flag", False,
            "weight-gradient products reduce over the tokens, so each operand gets ONE scale (its largest magnitude): columns more than "
            "2^16 below it lose relative precision gradually.  GRAPPA_WGRAD_COLUMN_MAXIMA=1 gives every column its own scale instead, "
            "at the price of one extra pass over both operands of every weight-gradient product (rigorous, ~15 % slower steps)"),

    Setting("FIRST_LAYER_ON_ATOM_ROWS", "ops", "GRAPPA_FIRST_LAYER_ROWS", "flag", True,
            "the first transformer layer of a writer on (atom, position) rows instead of tokens where those are far fewer (ProjFirstLayerFn); "
            "GRAPPA_FIRST_LAYER_ROWS=0: always the token formulation (ProjGatherFn + TransformerLayerFn)"),
    Setting("act_dtype", "ops", "GRAPPA_ACT_DTYPE", "str", "f32",
            "\"f32\" or \"bf16\", the bf16 STORAGE configuration (ops.set_activation_dtype, which sets it afterwards; ops.act_dtype() gives the "
            "element type, None = float32)"),

    Setting("head_streams", "writer", "GRAPPA_HEAD_STREAMS", "int", 4,
            "The four writers read the same atom embedding and write disjoint tuple levels: on the GPU each runs on its own HIP stream "
            "(largest first), so that the tail rounds and launch gaps of one head's kernels are filled by another head's; autograd replays "
            "every backward node on the stream of its forward, which gives the same overlap in the backward pass (-1.7 .. -2.0 ms of a 38 ms "
            "C2 step).  Default since round 3 (GRAPPA_HEAD_STREAMS=1 puts everything back on one stream).  History (DESIGN.md section 6): a "
            "since-removed LayerNorm kernel computed deviating rows beside MFMA wavefronts of another queue; the trigger -- packed fp32 "
            "instructions -- is compiled out of this library, and the gradients of h are joined by the library's own kernel "
            "(ops.SplitHeadsFn), so no torch arithmetic kernel runs on a side stream."),
    Setting("merged_heads", "writer", "GRAPPA_MERGED_HEADS", "str", "0",
            "round 4: the heads LAYER-LOCKED on one stream -- every product of a transformer / symmetriser layer is ONE grouped launch over the "
            "heads (ops.MultiTransformerLayerFn, backend.gemm_group): what the four streams approximated, without their launch count. "
            "GRAPPA_MERGED_HEADS: \"0\" (default) never, \"1\" always, \"auto\" = when a head's tokens would not fill the chip by themselves (fewer "
            "than `merged_heads_max_tokens` tokens in the largest head).  Measured (round 4, DESIGN.md section 6): the layer-locked heads cut "
            "the launches per batch-32 step from 681 to 487 and the products' time on one queue by 6 %, but lose to four streams on the wall "
            "clock in every regime tried -- C2 37.2 against 35.8 ms, batch 32 eager 18.4 against 16.4 ms (the Python that builds the grouped "
            "calls costs more than the launches it saves), recorded 9.5 against 9.0 ms, recorded predict 3.5 against 3.0 ms -- hence opt-in"),
    Setting("merged_heads_max_tokens", "writer", "GRAPPA_MERGED_HEADS_MAX_TOKENS", "int", 40000,
            "merged_heads \"auto\": the largest head's token count below which the heads are merged"),

    Setting("LIB_PATH", "host", "GRAPPA_HIP_LIB", "str", None,
            "_lib, at import: another libgrappa_hip.so than the one beside the package (kernel A/B builds, tools/)"),
    Setting("models_dir", "host", "GRAPPA_MODELS_DIR", "str", None,
            "loading.models_dir, per call: where release files are looked up before `<repository>/models`"),
    Setting("trust_checkpoints", "host", "GRAPPA_TRUST_CHECKPOINTS", "flag", False,
            "loading._torch_load, per call: unpickle in full a file that does not load with weights_only=True (the caller vouches for it)"),
    Setting("overlap", "host", "GRAPPA_OVERLAP_ALLREDUCE", "flag", False,
            "dist.BucketedGradReducer, at construction (see there for why it is opt-in): the writer-head bucket is all-reduced from inside the backward pass"),
    Setting("predict_graphs", "host", "GRAPPA_PREDICT_GRAPHS", "flag", True,
            "grappa.Grappa, at construction: repeated shapes replay a recorded hipGraph instead of issuing ~450 launches from Python "
            "(grappa_amd/capture.py; GRAPPA_PREDICT_GRAPHS=0: never)"),
    Setting("host_plan", "host", "GRAPPA_HOST_PLAN", _native_plan, True,
            "batch, per call: the batch plan's index structures and position tables from libgrappa_host.so; \"numpy\", \"0\" or empty: the numpy "
            "builders, the definition the native ones are tested against"),
)

BY_NAME = {e.name: e for e in TABLE}
_NAMES = {owner: tuple(e.name for e in TABLE if e.owner == owner) for owner in ("backend", "ops", "writer", "host")}


def of(owner: str) -> tuple:
    return tuple(BY_NAME[n] for n in _NAMES[owner])


def read(name: str):
    """the value of setting `name` under the current environment: unset gives the default; a flag is `not in ("0", "")`"""
    e = BY_NAME[name]
    raw = None if e.env is None else os.environ.get(e.env)
    if raw is None:
        return e.default
    if e.kind == "flag":
        return raw not in ("0", "")
    if e.kind == "int":
        return int(raw)
    return raw if e.kind == "str" else e.kind(raw)


def launch_stamp(be, model=None) -> tuple:
    """the current value of every `backend`, `ops` and `writer` setting: what a recorded hipGraph has baked into its launches besides shapes and
    weights.  A setting changed in the middle of a run means new graphs, not stale ones.  (All of them, not a chosen subset; values are read, never cached:
    tests and tools assign the attributes directly.  A backend or model that lacks an attribute gives None.)"""
    from . import ops
    pw = getattr(model, "parameter_writer", None)
    ops_values = (getattr(ops, n) for n in _NAMES["ops"])
    return (tuple(getattr(be, n, None) for n in _NAMES["backend"]) + tuple(v() if callable(v) else v for v in ops_values)
            + tuple(getattr(pw, n, None) for n in _NAMES["writer"]))


if __name__ == "__main__":
    for e in TABLE:
        kind = e.kind if isinstance(e.kind, str) else e.kind.__name__.strip("_")
        print(f"{e.owner + '.' + e.name:36s} {e.env or '-':32s} {kind:12s} default {e.default!r}, now {read(e.name)!r}\n    {e.doc}\n")
