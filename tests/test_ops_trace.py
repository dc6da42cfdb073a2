"""What the autograd Functions of grappa_amd/ops.py hand to the library, pinned call by call.

The writer heads' Functions (`TransformerLayerFn`, `ProjFirstLayerFn`, `SymmetriserFn`, their layer-locked forms `MultiTransformerLayerFn` and
`MultiSymmetriserFn`) and `AttBlockFn` are hand-sequenced kernel calls: which launch comes when, with which operand, record and seed, is the
whole content of that file.  None of it needs a GPU once the library is replaced by the recorder of tests/trace_recorder.py (a real
`HipBackend` over a stub whose every symbol records its call, on CPU tensors of zeros): every scenario of `SCENARIOS` runs a Function forward
and backward through it, and its trace is compared with the committed fixture tests/golden/ops_trace.json.

A trace is the ordered list of library calls with every descriptor field, in the text form test_dense_front_end_trace.py describes, and
after the calls of a step one `{step=...}` line with the element type and shape of every tensor the Function returned and of the gradient
every leaf received (`-` for none), the profile's figures and, for error cases, the exception.  The fixture holds these lines for the
scenarios of `IN_FULL` and, for the others, the number of lines and a SHA-256 digest of them; `--show SCENARIO` prints a scenario's lines from
whatever ops.py is first on the import path.

HOW THE FIXTURE WAS MADE: once, by this module's own write entry point run against grappa_amd/ops.py of commit 3246fcf ("Test output maps,
statistics gradients and parameter loss vs float64"), the commit BEFORE the feed-forward, the dropout backward, the attention layer body and
the symmetriser were each stated once for the head-by-head and the layer-locked path (a checkout of that commit in a scratch directory put
first on the import path):

    PYTHONPATH=<checkout of the parent commit> python tests/test_ops_trace.py --write

It is never regenerated from later code: the test's value is that it fails on any change to what these Functions emit.
"""
import itertools
import json
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.append(ROOT)          # (appended: the write entry point imports the package from whatever PYTHONPATH names first)

from grappa_amd import backend, ops          # noqa: E402
import trace_recorder                        # noqa: E402
from trace_recorder import F32, BF16, I32    # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "ops_trace.json")


def _desc(t):
    return None if t is None else f"{str(t.dtype).replace('torch.', '')}{list(t.shape)}"


class _Cx(trace_recorder._Cx):
    """the recorder's scenario with what the scenarios of ops.py need: the recorder as THE backend, named leaves, one step = forward + backward"""

    def __init__(self, mp):
        super().__init__(mp)
        mp.setattr(backend, "_BACKEND", self.be)
        mp.setitem(ops._INFERENCE, "on", False)
        mp.setitem(ops._ACT, "dtype", None)
        mp.setattr(torch.Tensor, "contiguous", self._noting(torch.Tensor.contiguous), raising=False)          # (the copies the Functions make)
        self.leaves = {}

    def t(self, name, shape, dtype=F32, grad=False):
        """a named tensor of zeros; grad: a leaf whose gradient the step reports"""
        self.naming = name
        t = torch.zeros(shape, dtype=dtype)
        self.naming = None
        if grad:
            self.leaves[name] = t.requires_grad_()
        return t

    def run(self, label, fn, no_grad=False, strided_grad=False):
        """fn() -> the Function's output(s); backward from named gradients of zeros where an output asks for one (strided_grad: from every
        second column of a table twice as wide, which the Functions have to copy)"""
        def body():
            with torch.no_grad() if no_grad else torch.enable_grad():
                ops.mark_mode()
                outs = fn()
            outs = outs if isinstance(outs, (tuple, list)) else (outs,)
            r = {"out": [_desc(o) for o in outs]}
            live = [o for o in outs if o.requires_grad]
            if live:
                gs = [self.t(f"{label}_g{i}", (o.shape[0], o.shape[1] * (2 if strided_grad else 1)), o.dtype) for i, o in enumerate(live)]
                torch.autograd.backward(live, [g[:, ::2] for g in gs] if strided_grad else gs)
                r["grad"] = {n: _desc(l.grad) for n, l in self.leaves.items()}
            return r
        self.step(label, body)


# ---------------------------------------------------------------------------------------------------- modes and parameters
def _mode(cx, mode):
    """-> no_grad?  infer: torch.no_grad() behind ops.mark_mode(); train: training_pairs off; pairs: on, with the row threshold lowered so
    that these tables qualify; +bwd: backward_pairs on; -ip: inference_pairs off; -fuse: the LayerNorm backward does not write the dropout's"""
    base, *flags = mode.replace("+", " +").replace("-", " -").split()
    cx.set(training_pairs=base == "pairs", pairs_min_rows=1, backward_pairs="+bwd" in flags, inference_pairs="-ip" not in flags,
           fuse_ln_drop="-fuse" not in flags)
    assert base in ("infer", "train", "pairs"), mode
    return base == "infer"


_LAYER = ("n1_w", "n1_b", "w_in", "b_in", "w_o", "b_o", "nf_w", "nf_b", "w1", "b1", "w2", "b2")


def _layer(cx, p, Fd, ln=True, frozen=()):
    """the twelve parameters of a transformer layer of width Fd, in the Functions' order"""
    shapes = dict(n1_w=(Fd,), n1_b=(Fd,), w_in=(3 * Fd, Fd), b_in=(3 * Fd,), w_o=(Fd, Fd), b_o=(Fd,), nf_w=(Fd,), nf_b=(Fd,), w1=(Fd, Fd), b1=(Fd,),
                  w2=(Fd, Fd), b2=(Fd,))
    return [None if (not ln and n[:2] in ("n1", "nf")) else cx.t(p + n, shapes[n], grad=n not in frozen) for n in _LAYER]


def _ff(cx, p, n_in, hid, n_out, ln=True, frozen=()):
    """norm_w, norm_b, w1, b1, w2, b2 of one FeedForward"""
    shapes = dict(nw=(n_in,), nb=(n_in,), w1=(hid, n_in), b1=(hid,), w2=(n_out, hid), b2=(n_out,))
    return [None if (not ln and n in ("nw", "nb")) else cx.t(p + n, shapes[n], grad=n not in frozen) for n in shapes]


def _sym_layers(cx, p, s, Fd, n_layers, n_out, ln=True, frozen=()):
    """a symmetriser's stack: s*Fd -> 64 (-> 64 with a skip)* -> n_out"""
    widths = [s * Fd] + [64] * (n_layers - 1) + [n_out]
    return [t for i in range(n_layers) for t in _ff(cx, f"{p}l{i}_", widths[i], 64, widths[i + 1], ln, frozen)]


def _perms(s):
    return [tuple(range(s)), tuple(reversed(range(s)))]


def _act(cx, bf16):
    if bf16:
        cx.mp.setitem(ops._ACT, "dtype", torch.bfloat16)
    return BF16 if bf16 else F32


# ---------------------------------------------------------------------------------------------------- the Functions
class _SecondConsumer(torch.autograd.Function):
    """a tensor as it is, in a graph where it has a second consumer: the backward pass adds that consumer's gradient (nothing) IN PLACE to the
    one that came first -- what autograd's accumulation does with a buffer it holds the only reference to, and so what the version check of
    `ops._masked_grad` is there for.  (The recorder keeps a reference to every tensor, so autograd itself would add out of place here.)"""

    @staticmethod
    def forward(ctx, x):
        y = x.view_as(x)
        if hasattr(x, "_grappa_drop"):
            y._grappa_drop = x._grappa_drop
        return y

    @staticmethod
    def backward(ctx, g):
        return g.add_(0.0)


def transformer(cx, s=3, T=40, mode="train", drop=0.0, Fd=64, nheads=4, bf16=False, ln=True, frozen=(), x_grad=None, layers=1, second_consumer=False, strided_grad=False, **be):
    no_grad = _mode(cx, mode)
    cx.set(**be)
    dt = _act(cx, bf16)
    x = cx.t("x", (s * T, Fd), dt, grad=x_grad if x_grad is not None else not no_grad)
    P = [_layer(cx, f"L{i}_", Fd, ln, frozen) for i in range(layers)]

    def fn():
        cur = x
        for i, p in enumerate(P):
            if i and second_consumer:
                cur = _SecondConsumer.apply(cur)
            cur = ops.TransformerLayerFn.apply(cur, s, T, nheads, drop, 11 + 2 * i, 12 + 2 * i, *p)
        return cur
    cx.run("layer", fn, no_grad, strided_grad)


def proj_first(cx, s=3, T=40, mode="train", drop=0.0, N=12, R=64, Fd=64, nheads=4, pe=True, bf16=False, ln=True, frozen=(), h_grad=None, strided_grad=False, **be):
    no_grad = _mode(cx, mode)
    cx.set(**be)
    dt = _act(cx, bf16)
    Wp = Fd - (1 if pe else 0)
    h = cx.t("h", (N, R), F32, grad=h_grad if h_grad is not None else not no_grad)
    w, b = cx.t("w", (Wp, R), grad="w" not in frozen), cx.t("b", (Wp,), grad="b" not in frozen)
    tabs = (cx.t("idx_id", (N, s), I32), cx.t("invid_ptr", (N + 1,), I32), cx.t("invid_rows", (s * N,), I32), cx.t("idx_tab", (T, s), I32),
            cx.t("invtab_ptr", (s * N + 1,), I32), cx.t("invtab_rows", (s * T,), I32))
    pev = cx.t("pe", (s,)) if pe else None
    P = _layer(cx, "", Fd, ln, frozen)
    cx.run("first", lambda: ops.ProjFirstLayerFn.apply(h, w, b, tabs, s, T, pev, None if dt == F32 else dt, nheads, drop, 21, 22, *P), no_grad, strided_grad)


def symmetriser(cx, s=3, T=40, mode="train", Fd=64, n_layers=3, n_out=8, bf16=False, ln=True, frozen=(), x_grad=None, strided_grad=False, **be):
    no_grad = _mode(cx, mode)
    cx.set(**be)
    x = cx.t("x", (s * T, Fd), _act(cx, bf16), grad=x_grad if x_grad is not None else not no_grad)
    flat = _sym_layers(cx, "", s, Fd, n_layers, n_out, ln, frozen)
    cx.run("sym", lambda: ops.SymmetriserFn.apply(x, s, T, _perms(s), n_layers, *flat), no_grad, strided_grad)


def multi_transformer(cx, heads=((2, 40), (3, 40)), mode="train", drop=0.0, Fd=64, nheads=4, ln=True, frozen=(), frozen_head=0, no_grad_x=(), strided_grad=False, **be):
    """heads: (s, T) per head; frozen: parameters of head `frozen_head` that take no gradient; no_grad_x: heads whose x takes none"""
    no_grad = _mode(cx, mode)
    cx.set(**be)
    cfgs, flat = [], []
    for i, (s, T) in enumerate(heads):
        cfgs.append((s, T, nheads, drop, 31 + 2 * i, 32 + 2 * i))
        flat += [cx.t(f"x{i}", (s * T, Fd), grad=not no_grad and i not in no_grad_x)] + _layer(cx, f"h{i}_", Fd, ln, frozen if i == frozen_head else ())
    cx.run("layers", lambda: ops.MultiTransformerLayerFn.apply(tuple(cfgs), *flat), no_grad, strided_grad)


def multi_symmetriser(cx, heads=((2, 40, 3, 8), (3, 40, 2, 8)), mode="train", Fd=64, ln=True, frozen=(), frozen_head=0, no_grad_x=(), **be):
    """heads: (s, T, n_layers, n_out) per head"""
    no_grad = _mode(cx, mode)
    cx.set(**be)
    cfgs, flat = [], []
    for i, (s, T, nl, n_out) in enumerate(heads):
        cfgs.append((s, T, _perms(s), nl))
        flat += [cx.t(f"x{i}", (s * T, Fd), grad=not no_grad and i not in no_grad_x)] + _sym_layers(cx, f"h{i}_", s, Fd, nl, n_out, ln, frozen if i == frozen_head else ())
    cx.run("syms", lambda: ops.MultiSymmetriserFn.apply(tuple(cfgs), *flat), no_grad)


def att_block(cx, N=40, E=90, mode="train", drop=0.0, Fd=64, heads=4, ff=True, ln=True, frozen=(), **be):
    no_grad = _mode(cx, mode)
    cx.set(**be)
    plan = types.SimpleNamespace(N=N, E=E, indptr=cx.t("indptr", (N + 1,), I32), indices=cx.t("indices", (E,), I32), rev=cx.t("rev", (E,), I32))
    h = cx.t("h", (N, Fd), grad=not no_grad)
    g = lambda n, shape: cx.t(n, shape, grad=n not in frozen)          # noqa: E731
    ln1 = [g("ln_w", (Fd,)), g("ln_b", (Fd,))] if ln else [None, None]
    ln2 = [g("ln2_w", (Fd,)), g("ln2_b", (Fd,))] if ln else [None, None]
    tail = ln2 + [g("w1", (Fd, Fd)), g("b1", (Fd,)), g("w2", (Fd, Fd)), g("b2", (Fd,))] if ff else [None] * 6
    P = ln1 + [g("w_fc", (Fd, Fd)), g("w_r", (Fd, Fd)), g("b_r", (Fd,))] + tail
    cx.run("block", lambda: ops.AttBlockFn.apply(h, plan, heads, drop, 41, 42, *P), no_grad)


# ---------------------------------------------------------------------------------------------------- the table
SCENARIOS = {}


def _add(name, f, **kw):
    assert name not in SCENARIOS, name
    SCENARIOS[name] = lambda cx: f(cx, **kw)


def _tag(**kw):
    return "_".join(f"{k}{'-'.join(map(str, v)) if isinstance(v, (tuple, list)) else v}" for k, v in kw.items())


_MODES = ("infer", "infer-ip", "train", "train-fuse", "pairs", "pairs+bwd")
_FROZEN = {"w2": ("w2",), "wo": ("w_o",), "win": ("w_in",), "ln1": ("n1_w", "n1_b"), "lnf": ("nf_w", "nf_b"), "b2": ("b2",), "bo": ("b_o",), "w1": ("w1",)}

# ---- TransformerLayerFn, fp32: every tuple size, both sides of the row thresholds, an empty level, every mode, dropout off and on
for _s, _T, _m, _p in itertools.product((2, 3, 4), (0, 5, 40), _MODES, (0.0, 0.1)):
    _add("tl_" + _tag(s=_s, T=_T, m=_m, p=_p), transformer, s=_s, T=_T, mode=_m, drop=_p)
for _m, _p in itertools.product(("infer", "train", "pairs", "pairs+bwd"), (0.0, 0.1)):
    _add("tl_noln_" + _tag(m=_m, p=_p), transformer, mode=_m, drop=_p, ln=False)
    _add("tl_xnograd_" + _tag(m=_m, p=_p), transformer, mode=_m, drop=_p, x_grad=False)
for (_n, _f), _m in itertools.product(_FROZEN.items(), ("train", "pairs+bwd")):
    _add(f"tl_frozen_{_n}_" + _tag(m=_m), transformer, mode=_m, drop=0.1, frozen=_f)
# ---- two layers in one graph: the dropout of the layer in front, written by the LayerNorm backward of the layer behind
for _m, _p, _c in itertools.product(("train", "train-fuse", "pairs", "pairs+bwd"), (0.0, 0.1), (False, True)):
    _add("tl_stack_" + _tag(m=_m, p=_p, second=int(_c)), transformer, mode=_m, drop=_p, layers=2, second_consumer=_c)
for _m, _p in itertools.product(("train", "pairs+bwd"), (0.0, 0.1)):
    _add("tl_strided_grad_" + _tag(m=_m, p=_p), transformer, mode=_m, drop=_p, strided_grad=True)
    _add("pf_strided_grad_" + _tag(m=_m, p=_p), proj_first, mode=_m, drop=_p, strided_grad=True)
    _add("mt_strided_grad_" + _tag(m=_m, p=_p), multi_transformer, mode=_m, drop=_p, strided_grad=True)
    _add("sy_strided_grad_" + _tag(m=_m), symmetriser, mode=_m, strided_grad=True) if _p == 0.0 else None
    _add("tl_xgrad_infer_" + _tag(m=_m, p=_p), transformer, mode="infer", drop=_p, x_grad=True) if _m == "train" else None
_add("tl_stack_noln", transformer, drop=0.1, layers=2, ln=False)
_add("tl_stack_frozen_ln1", transformer, drop=0.1, layers=2, frozen=("n1_w", "n1_b"))
_add("tl_stack_infer", transformer, mode="infer", drop=0.1, layers=2)
# ---- bf16 storage: the fused layer and its switches
for _s, _T, _m, _p, _fw, _fb in itertools.product((2, 3, 4), (5, 40), ("infer", "train"), (0.0, 0.1), (True, False), (True, False)):
    if _m == "infer" and not _fb:
        continue
    _add("tl_bf16_" + _tag(s=_s, T=_T, m=_m, p=_p, fused=int(_fw), fbwd=int(_fb)), transformer, s=_s, T=_T, mode=_m, drop=_p, Fd=512, nheads=8, bf16=True,
         fused_writer_layer=_fw, fused_writer_layer_bwd=_fb)
_add("tl_bf16_T0", transformer, T=0, Fd=512, nheads=8, bf16=True)
_add("tl_bf16_noln", transformer, Fd=512, nheads=8, bf16=True, ln=False, drop=0.1)
_add("tl_bf16_narrow", transformer, Fd=64, nheads=4, bf16=True, drop=0.1)
_add("tl_bf16_stack", transformer, Fd=512, nheads=8, bf16=True, drop=0.1, layers=2)
_add("tl_bf16_frozen_w2", transformer, Fd=512, nheads=8, bf16=True, drop=0.1, frozen=("w2", "nf_w", "nf_b", "b_o"))

# ---- ProjFirstLayerFn
for _s, _T, _m, _p, _ix in itertools.product((2, 3, 4), (0, 5, 40), ("infer", "train", "pairs", "pairs+bwd"), (0.0, 0.1), (True, False)):
    _add("pf_" + _tag(s=_s, T=_T, m=_m, p=_p, idx=int(_ix)), proj_first, s=_s, T=_T, mode=_m, drop=_p, first_layer_indexed=_ix)
for _ix in (True, False):
    _add(f"pf_noln_idx{int(_ix)}", proj_first, drop=0.1, ln=False, first_layer_indexed=_ix)
    _add(f"pf_nope_idx{int(_ix)}", proj_first, drop=0.1, pe=False, first_layer_indexed=_ix)
    _add(f"pf_hnograd_idx{int(_ix)}", proj_first, drop=0.1, h_grad=False, first_layer_indexed=_ix)
    _add(f"pf_infer-ip_idx{int(_ix)}", proj_first, mode="infer-ip", first_layer_indexed=_ix)
    _add(f"pf_train-fuse_idx{int(_ix)}", proj_first, mode="train-fuse", drop=0.1, first_layer_indexed=_ix)
    for _n, _f in dict(_FROZEN, w=("w",), b=("b",)).items():
        _add(f"pf_frozen_{_n}_idx{int(_ix)}", proj_first, mode="pairs+bwd", drop=0.1, frozen=_f, first_layer_indexed=_ix)
for _s, _T, _m, _p, _f1, _fb in itertools.product((2, 3, 4), (5, 40), ("infer", "train"), (0.0, 0.1), (True, False), (True, False)):
    if _m == "infer" and not _fb:
        continue
    _add("pf_bf16_" + _tag(s=_s, T=_T, m=_m, p=_p, ffirst=int(_f1), fbwd=int(_fb)), proj_first, s=_s, T=_T, mode=_m, drop=_p, Fd=512, nheads=8, bf16=True,
         fused_first_layer=_f1, fused_writer_layer_bwd=_fb)
_add("pf_bf16_unfused", proj_first, Fd=512, nheads=8, bf16=True, drop=0.1, fused_writer_layer=False)
_add("pf_bf16_T0", proj_first, T=0, Fd=512, nheads=8, bf16=True)
_add("pf_bf16_frozen", proj_first, Fd=512, nheads=8, bf16=True, drop=0.1, frozen=("w_o", "b1", "nf_w", "nf_b"))

# ---- SymmetriserFn
for _s, _T, _m, _nl, _no in itertools.product((2, 3, 4), (0, 5, 40), _MODES, (1, 2, 3), (8, 64)):
    if _m in ("infer-ip", "train-fuse") and _nl != 3:
        continue
    _add("sy_" + _tag(s=_s, T=_T, m=_m, layers=_nl, out=_no), symmetriser, s=_s, T=_T, mode=_m, n_layers=_nl, n_out=_no)
for _m in ("infer", "train", "pairs+bwd"):
    _add("sy_noln_" + _tag(m=_m), symmetriser, mode=_m, ln=False)
    _add("sy_xnograd_" + _tag(m=_m), symmetriser, mode=_m, x_grad=False)
    _add("sy_bf16_" + _tag(m=_m), symmetriser, mode=_m, bf16=True)
    for _n, _f in dict(w2=("w2",), w1=("w1",), ln=("nw", "nb"), b2=("b2",), b1=("b1",)).items():
        _add(f"sy_frozen_{_n}_" + _tag(m=_m), symmetriser, mode=_m, frozen=_f)

# ---- MultiTransformerLayerFn: 1, 2 and 4 heads with different s
_HEADS = {"1": ((3, 40),), "2": ((2, 40), (3, 40)), "4": ((2, 40), (3, 40), (4, 40), (4, 5)), "4small": ((2, 5), (3, 5), (4, 5), (4, 3)),
          "2mixed": ((3, 5), (4, 40))}
for (_n, _h), _m, _p in itertools.product(_HEADS.items(), _MODES, (0.0, 0.1)):
    _add(f"mt_{_n}_" + _tag(m=_m, p=_p), multi_transformer, heads=_h, mode=_m, drop=_p)
for _m, _p in itertools.product(("infer", "train", "pairs+bwd"), (0.0, 0.1)):
    _add("mt_noln_" + _tag(m=_m, p=_p), multi_transformer, mode=_m, drop=_p, ln=False)
    _add("mt_xnograd_" + _tag(m=_m, p=_p), multi_transformer, mode=_m, drop=_p, no_grad_x=(1,))
    _add("mt_xnograd_all_" + _tag(m=_m, p=_p), multi_transformer, mode=_m, drop=_p, no_grad_x=(0, 1))
for (_n, _f), _m, _fh in itertools.product(_FROZEN.items(), ("train", "pairs+bwd"), (0, 1)):
    _add(f"mt_frozen_{_n}_" + _tag(m=_m, head=_fh), multi_transformer, mode=_m, drop=0.1, frozen=_f, frozen_head=_fh)
_add("mt_group_launches_off", multi_transformer, drop=0.1, group_launches=False)
_add("mt_defer_ln_off", multi_transformer, drop=0.1, defer_ln=False)

# ---- MultiSymmetriserFn: heads of different depth (a layer with fewer active heads), narrow and wide outputs
_SHEADS = {"1": ((3, 40, 3, 8),), "2": ((2, 40, 3, 8), (3, 40, 2, 8)), "4": ((2, 40, 3, 8), (3, 40, 2, 64), (4, 40, 3, 8), (4, 5, 1, 8)),
           "4wide": ((2, 40, 3, 64), (3, 40, 3, 64), (4, 40, 2, 64), (4, 40, 3, 64)), "2small": ((2, 5, 2, 8), (3, 5, 3, 64))}
for (_n, _h), _m in itertools.product(_SHEADS.items(), _MODES):
    _add(f"ms_{_n}_" + _tag(m=_m), multi_symmetriser, heads=_h, mode=_m)
for _m in ("infer", "train", "pairs+bwd"):
    _add("ms_noln_" + _tag(m=_m), multi_symmetriser, mode=_m, ln=False)
    _add("ms_xnograd_" + _tag(m=_m), multi_symmetriser, mode=_m, no_grad_x=(0,))
    _add("ms_xnograd_all_" + _tag(m=_m), multi_symmetriser, mode=_m, no_grad_x=(0, 1))
    for (_n, _f), _fh in itertools.product(dict(w2=("w2",), w1=("w1",), ln=("nw", "nb"), b2=("b2",)).items(), (0, 1)):
        _add(f"ms_frozen_{_n}_" + _tag(m=_m, head=_fh), multi_symmetriser, mode=_m, frozen=_f, frozen_head=_fh)

# ---- AttBlockFn: with and without its feed-forward part (the one caller of the feed-forward with an activation behind the second product)
for _N, _m, _p, _ffp in itertools.product((20, 40), _MODES, (0.0, 0.1), (True, False)):
    _add("ab_" + _tag(N=_N, m=_m, p=_p, ff=int(_ffp)), att_block, N=_N, mode=_m, drop=_p, ff=_ffp)
for _m in ("train", "pairs+bwd"):
    _add("ab_noln_" + _tag(m=_m), att_block, mode=_m, drop=0.1, ln=False)
    for _n, _f in dict(w2=("w2",), wr=("w_r",), ln2=("ln2_w", "ln2_b"), b2=("b2",), w1=("w1",)).items():
        _add(f"ab_frozen_{_n}_" + _tag(m=_m), att_block, mode=_m, drop=0.1, frozen=_f)

# the scenarios whose trace the fixture holds line by line; of the others it holds a digest of the same lines
IN_FULL = {"tl_s3_T40_mtrain_p0.1", "tl_s3_T40_mpairs+bwd_p0.1", "tl_s3_T40_minfer_p0.0", "tl_stack_mtrain_p0.1_second0", "tl_stack_mtrain_p0.1_second1",
           "tl_bf16_s3_T40_mtrain_p0.1_fused1_fbwd1", "pf_s3_T40_mtrain_p0.1_idx1", "pf_bf16_s3_T40_mtrain_p0.1_ffirst1_fbwd1",
           "sy_s3_T40_mtrain_layers3_out8", "mt_4_mtrain_p0.1", "mt_4_mtrain_p0.0", "ms_4_mtrain", "ab_N40_mtrain_p0.1_ff1"}


# ---------------------------------------------------------------------------------------------------- driver
def run_scenario(name, mp):
    cx = _Cx(mp)
    SCENARIOS[name](cx)
    out = trace_recorder.lines(cx)
    assert not any("?" in e for e in out if not e.startswith("{step=")), f"{name}: a pointer into memory the recorder does not know"
    return out


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_table_and_fixture_hold_the_same_scenarios():
    fx = _fixture()
    assert sorted(fx) == sorted(SCENARIOS)
    assert {n for n, v in fx.items() if isinstance(v, list)} == IN_FULL


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_ops_trace(name, monkeypatch):
    want = _fixture()[name]
    got = run_scenario(name, monkeypatch)
    if isinstance(want, str):
        assert trace_recorder.digest(got) == want, \
            f"{name}: the trace changed; `--show {name}` prints it (for the pinned one: with the parent commit first on PYTHONPATH):\n" + "\n".join(got)
        return
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: entry {i} differs"
    assert len(got) == len(want)


def _write():
    out = []
    for name in sorted(SCENARIOS):
        with pytest.MonkeyPatch.context() as mp:
            entries = run_scenario(name, mp)
        if name in IN_FULL:
            out.append(f" {json.dumps(name)}: [\n" + ",\n".join("  " + json.dumps(e) for e in entries) + "\n ]")
        else:
            out.append(f" {json.dumps(name)}: {json.dumps(trace_recorder.digest(entries))}")
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(out) + "\n}\n")
    print(f"{FIXTURE}: {len(SCENARIOS)} scenarios from {ops.__file__}")


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        _write()
    elif len(sys.argv) == 3 and sys.argv[1] == "--show" and sys.argv[2] in SCENARIOS:
        with pytest.MonkeyPatch.context() as mp:
            print("\n".join(run_scenario(sys.argv[2], mp)))
    else:
        sys.exit("usage: PYTHONPATH=<checkout of the parent commit> python tests/test_ops_trace.py --write | --show SCENARIO")
