"""What the Python front end of the dense products hands to the library, pinned call by call.

`HipBackend.gemm`, `gemm_group`, `gemm_wgrad` and the per-weight caches behind them decide which kernel family a product takes, which side
launches it triggers (weight maxima, pairs, planes, conversions) and what every field of its `grappa_gemm_desc` holds.  None of that needs a
GPU once the library is replaced by a recorder: this module builds a real `HipBackend` over a stub whose every symbol records its call and
returns 0 (a fixed byte count for the `*_workspace_bytes` queries), on CPU tensors, with `torch.cuda`'s stream / event entry points replaced
through pytest's `monkeypatch`.  Every scenario of `SCENARIOS` is driven through it and its trace compared with the committed fixture
tests/golden/dense_front_end_trace.json.

A trace is the ordered list of library calls, one line of text each: `symbol(arguments)` without the grappa_ prefix.  Every structure passed
(a `grappa_gemm_desc`, the array of a group or of a grouped launch, the LayerNorm reduction items, the device tables of the batched
refreshes) is dumped field by field as `{field=value ...}`, non-zero fields only.  Pointers are position-independent: `name+byte_offset`
into a tensor the scenario supplied, `new<k>+offset` into a tensor the front end allocated itself (numbered in order of first appearance),
`#<n>` for a stream handle, `-` for null.  After the calls of a step comes one `{step=...}` line with the shape of the return value, the
profile's family / launches / flops / bytes figures, the `last_profile_details` dicts and, for error cases, the exception type and message.
To keep the fixture small it holds these lines for the scenarios of `IN_FULL` (every route and entry point once) and, for the others, the
number of lines and a SHA-256 digest of them; `--show SCENARIO` prints a scenario's lines from whatever backend.py is first on the import path.

HOW THE FIXTURE WAS MADE: once, by this module's own write entry point run against grappa_amd/backend.py of the commit BEFORE the front end
was split into route, binding and launch (a checkout of that commit in a scratch directory put first on the import path):

    PYTHONPATH=<checkout of the parent commit> python tests/test_dense_front_end_trace.py --write

It is never regenerated from later code: the test's value is that it fails on any change to what the front end emits.
"""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.append(ROOT)          # (appended: the write entry point imports the package from whatever PYTHONPATH names first)

from grappa_amd import backend          # noqa: E402
from grappa_amd.backend import Amax           # noqa: E402
import trace_recorder                         # noqa: E402  (tests/trace_recorder.py: the stub library, its streams, the pointer naming)
from trace_recorder import F32, BF16, F16, I32, txt as _txt, digest as _digest          # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "dense_front_end_trace.json")


class _Cx(trace_recorder._Cx):
    """the recorder's scenario with what the scenarios of the dense products call: operands, records and the two entry points on fresh tensors"""

    def scales(self, p, kind, rows, cols):
        """an `Amax` record as a producer would hand it over"""
        if kind is None or isinstance(kind, Amax):
            return kind
        r = Amax()
        if kind in ("row", "pairs", "pairs_shape", "row_short"):
            r.row = self.vec(p + "_row", rows - (kind == "row_short"), I32)
        if kind in ("parts", "parts_other"):        # the partials of two segments; "parts_other": of another row count (combined into a row array)
            r.nseg = 2
            r.parts = self.vec(p + "_parts", 2 * rows + 2 * (kind == "parts_other"), I32)
        if kind in ("pairs", "pairs_shape"):
            r.pairs = self.mat(p + "_pairs", F16, (rows, 2 * cols + 64 * (kind == "pairs_shape")))
        if kind == "col":
            r.col = self.vec(p + "_col", cols, I32)
        if kind == "tmax":
            r.tmax = self.vec(p + "_tmax", 1, I32)
        self.records[p] = r
        return r

    def _epi(self, name, spec, shape):
        if spec is None or isinstance(spec, torch.Tensor):
            return spec
        if isinstance(spec, dict):
            return self.mat(name, spec.get("dtype", F32), spec.get("shape", shape), spec.get("ld"), spec.get("off", 0))
        return self.mat(name, spec, shape)

    def gemm(self, step="gemm", M=64, N=64, K=64, lay="fwd", a=F32, b=F32, out=F32, a_ld=None, a_off=0, b_ld=None, b_off=0, b_grad=True,
             out2=None, res=None, aux=None, pre=None, bias=None, res_ln=None, colsum=None, scales=None, b_scales=None,
             a_shape=None, b_shape=None, p="", defer=False, **kw):
        """one `gemm` call on fresh tensors named a, b, out, ... (prefix `p`); a tensor given for an operand is used as it is"""
        ak, bk = {"fwd": (True, True), "dgrad": (True, False), "wgrad": (False, False), "bad": (False, True)}[lay]
        ar, ac = (M, K) if ak else (K, M)
        br, bc = (N, K) if bk else (K, N)
        A = a if a is None or isinstance(a, torch.Tensor) else self.mat(p + "a", a, a_shape or (ar, ac), a_ld, a_off)
        B = b if isinstance(b, torch.Tensor) else self.mat(p + "b", b, b_shape or (br, bc), b_ld, b_off, grad=ak and b_grad)
        k = dict(M=M, N=N, K=K, a_kcontig=ak, b_kcontig=bk)
        for name, spec in (("out2", out2), ("res", res), ("aux", aux), ("pre", pre)):
            if spec is not None:
                k[name] = self._epi(p + name, spec, (M, N))
        if bias is not None:
            k["bias"] = bias if isinstance(bias, torch.Tensor) else self.vec(p + "bias", N if bias is True else bias[0], F32 if bias is True else bias[1])
        if res_ln is not None:
            lens = dict(mean=M, rstd=M, gamma=N, beta=N)
            lens.update({} if res_ln is True else res_ln)
            k["res_ln"] = tuple(self.vec(p + "ln_" + n, lens[n]) for n in ("mean", "rstd", "gamma", "beta"))
        if colsum is not None:
            k["a_colsum"] = self.vec(p + "colsum", M if colsum is True else colsum)
        if scales is not None:
            k["a_scales"] = self.scales(p + "sa", scales, ar, ac)
        if b_scales is not None:
            k["b_scales"] = self.scales(p + "sb", b_scales, br, bc)
        k.update(kw)
        args = (A, B, self._epi(p + "out", out, (M, N)))
        if defer:
            return args, k
        self.step(step, lambda: self.be.gemm(*args, **k))
        return args, k

    def wgrad(self, step="wgrad", T=64, Np=64, Kp=64, dz=F32, x=F32, dz_ld=None, x_ld=None, dz_off=0, db=False, zs=None, xs=None, dw=None, p="",
              dz_shape=None, run=True):
        """one `gemm_wgrad` call on fresh tensors dz, x, dw (, db)"""
        Z = dz if dz is None or isinstance(dz, torch.Tensor) else self.mat(p + "dz", dz, dz_shape or (T, Np), dz_ld, dz_off)
        X = x if x is None or isinstance(x, torch.Tensor) else self.mat(p + "x", x, (T, Kp), x_ld)
        W = dw if dw is not None else self.mat(p + "dw", F32, (Np, Kp))
        Bv = self.vec(p + "db", Np if db is True else db) if db else None
        call = lambda: self.be.gemm_wgrad(Z, X, W, Bv, dz_scales=self.scales(p + "sz", zs, T, Np), x_scales=self.scales(p + "sx", xs, T, Kp))      # noqa: E731
        if run:
            self.step(step, call)
        return call

    def backward(self, step, fn):
        """`fn` inside a backward pass of autograd (a graph task with its end-of-pass callbacks), as one step"""
        got = []

        class F(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x):
                return x.clone()

            @staticmethod
            def backward(ctx, g):
                got.append(fn())
                return g

        def run():
            F.apply(torch.ones(1, requires_grad=True)).sum().backward()
            return got[0]
        self.step(step, run)

    def touch(self, w):
        with torch.no_grad():
            w.add_(1.0)


# ---------------------------------------------------------------------------------------------------- the table
SCENARIOS = {}


def scenario(f):
    SCENARIOS[f.__name__] = f
    return f


def _simple(name, setup=None, **kw):
    def f(cx):
        if setup is not None:
            setup(cx)
        cx.gemm(**kw)
    SCENARIOS[name] = f


WP = lambda cx: cx.set(weight_pairs_min_rows=64)          # noqa: E731 -- (the threshold at a size a CPU test can afford)

# ---- every route in the forward and the input-gradient layout
for _lay in ("fwd", "dgrad"):
    _simple(f"split_{_lay}", lay=_lay, N=96, K=40)
    _simple(f"pairs_{_lay}", lay=_lay, a=None, scales="pairs", N=96)
    _simple(f"wpairs_{_lay}_at_threshold", WP, lay=_lay, N=96)
    _simple(f"bf16_a_planes_{_lay}", lay=_lay, a=BF16, N=96, out=BF16)
    _simple(f"bf16_a_converted_{_lay}", lay=_lay, a=BF16, a_off=1)
    _simple(f"weight_planes_{_lay}", lambda cx: cx.set(weight_planes=True), lay=_lay, precision="f32_bf16x6")
    _simple(f"native_small_m_{_lay}", lay=_lay, M=32)
    _simple(f"native_precision_{_lay}", lay=_lay, precision="f32", bias=True, res=F32)
    _simple(f"native_small_bf16_epilogue_{_lay}", lay=_lay, M=16, out=BF16, out2=BF16, res=BF16, aux=BF16, bias=True, act=1, drop_p=0.1, drop_seed=5, out_amax=True)
    _simple(f"native_precision_bf16_out_{_lay}", lay=_lay, precision="f32", out=BF16, res=F32, pre=F32)
    _simple(f"precision_bwd_{_lay}", lambda cx: cx.be.set_gemm_precision_bwd("bf16x3"), lay=_lay, scales="row")

# ---- what decides between the routes, and the source of A's maxima: each in one of the two layouts, alternating
_WPL = lambda cx: cx.set(weight_planes=True)          # noqa: E731
for _i, (_n, _su, _kw) in enumerate([
        ("split_row_given", None, dict(scales="row")),
        ("split_partials_taken", None, dict(scales="parts")),
        ("split_partials_combined", None, dict(scales="parts_other")),
        ("pairs_with_fp32_a", None, dict(scales="pairs")),
        ("wpairs_below_threshold", WP, dict(M=63)),
        ("wpairs_partials_taken", WP, dict(scales="parts")),
        ("wpairs_partials_combined", WP, dict(scales="parts_other")),
        ("wpairs_row_given", WP, dict(scales="row")),
        ("wpairs_unaligned_a", WP, dict(a_off=1)),
        ("wpairs_odd_k", WP, dict(K=48)),
        ("bf16_a_converted_ld", None, dict(a=BF16, a_ld=68)),
        ("bf16_a_converted_k", None, dict(a=BF16, K=48)),
        ("bf16_a_converted_wpairs", WP, dict(a=BF16, a_off=1, scales="row")),
        ("bf16_a_converted_wpairs_wide_ld", WP, dict(a=BF16, a_ld=66, M=96)),
        ("weight_planes_default_precision", _WPL, dict()),
        ("weight_planes_frozen_weight", _WPL, dict(precision="f32_bf16x6", b_grad=False)),
        ("weight_planes_bf16_a_converted", lambda cx: (_WPL(cx), cx.be.set_gemm_precision("bf16x3")), dict(a=BF16, a_off=1)),
        ("native_small_n", None, dict(N=16, scales="row")),
        ("native_precision_bf16_res", None, dict(precision="f32", res=BF16, aux=BF16, out2=F32)),
        ("native_bf16_a_small", None, dict(a=BF16, N=8, out=BF16)),
        ("precision_bwd_f32", lambda cx: cx.be.set_gemm_precision_bwd("f32"), dict()),
        ("precision_arg", None, dict(precision="f32_bf16x9")),
        ("backend_precision", lambda cx: cx.be.set_gemm_precision("f32_bf16x6"), dict(scales="pairs"))]):
    _simple(f"{_n}_{('fwd', 'dgrad')[_i % 2]}", _su, lay=("fwd", "dgrad")[_i % 2], **_kw)
    if _n == "precision_bwd_f32":
        _simple(f"{_n}_dgrad", _su, lay="dgrad", **_kw)          # (the forward product keeps the forward arithmetic: both sides)

# ---- each reason a pair-format A is refused: with the fp32 tensor (falls back) and without (raises)
_REFUSALS = {
    "small_m": dict(M=32), "small_n": dict(N=32), "k": dict(K=48), "precision_arg": dict(precision="f32_f16x3"), "shape": dict(scales="pairs_shape"),
    "weight_dtype": dict(b=BF16), "wgrad_layout": dict(lay="wgrad"), "colsum": dict(lay="wgrad", colsum=True),
    "precision_bwd": dict(setup=lambda cx: cx.be.set_gemm_precision_bwd("f32_f16x3")), "backend_precision": dict(setup=lambda cx: cx.be.set_gemm_precision("f32_bf16x6")),
}
for _n, _kw in _REFUSALS.items():
    _simple(f"pairs_refused_{_n}_fallback", **dict(dict(scales="pairs"), **_kw))
    _simple(f"pairs_refused_{_n}_raises", **dict(dict(scales="pairs", a=None), **_kw))

# ---- the weight-gradient layout through `gemm`
_simple("wgrad_f32", lay="wgrad", N=96, accumulate=True)
_simple("wgrad_f32_scales_given", lay="wgrad", scales="row", b_scales="tmax", accumulate=True)
_simple("wgrad_f32_partials_given", lay="wgrad", scales="parts", b_scales="parts", colsum=True, accumulate=True)
_simple("wgrad_column_maxima", lambda cx: cx.set(wgrad_column_maxima=True), lay="wgrad", b_scales="col", colsum=True)
_simple("wgrad_bf16_planes", lay="wgrad", a=BF16, b=BF16, colsum=True, accumulate=True)
_simple("wgrad_bf16_unaligned", lay="wgrad", a=BF16, b=BF16, b_ld=68)
_simple("wgrad_bf16_one_side", lay="wgrad", a=BF16, b=F32)
_simple("wgrad_bf16_small", lay="wgrad", a=BF16, b=BF16, M=16)
_simple("wgrad_precision_bwd", lambda cx: cx.be.set_gemm_precision_bwd("bf16x3"), lay="wgrad")
_simple("wgrad_native", lay="wgrad", precision="f32", colsum=True)

# ---- epilogue tensors in both element types, output maxima
_simple("epi_bias_act_drop", bias=True, act=1, drop_p=0.25, drop_seed=-3)
_simple("epi_res_f32", res=dict(ld=72), out=dict(ld=80, off=4))
_simple("epi_res_bf16", res=BF16, out=BF16)
_simple("epi_res_ln", res=F32, res_ln=True, bias=True)
_simple("epi_aux_f32", lay="dgrad", aux=F32)
_simple("epi_aux_bf16", lay="dgrad", aux=BF16, a=BF16, out=BF16)
_simple("epi_pre", pre=F32, res=F32)
_simple("epi_out2_c2", out2=F32, drop_p=0.1, drop_seed=2 ** 64 + 9)
_simple("epi_out2_c1p", out2=BF16, out=BF16, a=BF16)
_simple("epi_accumulate", lay="dgrad", accumulate=True, res=F32)
_simple("epi_pairs_everything", a=None, scales="pairs", bias=True, act=1, drop_p=0.1, drop_seed=1, res=F32, res_ln=True, out2=F32, pre=F32, out_amax=True)
_simple("epi_wpairs_everything", WP, scales="row", bias=True, res=BF16, aux=BF16, out=BF16, out_amax=True)
_simple("out_amax_split", out_amax=True)
_simple("out_amax_pair_only", out_amax="pair")
_simple("out_amax_out2", out2=F32, out_amax=True, scales="row")
_simple("out_amax_bf16_output", out=BF16, out_amax=True)
_simple("out_amax_native", M=16, out_amax=True)
_simple("out_amax_empty", M=0, out_amax=True)
_simple("empty_n", N=0)
for _n, _kw in {"split": {}, "pairs": dict(a=None, scales="pairs"), "wpairs": dict(setup=WP), "bf16_planes": dict(a=BF16), "native": dict(N=32),
                "weight_planes": dict(precision="f32_bf16x6"), "dgrad": dict(lay="dgrad", N=96)}.items():
    _su = _kw.pop("setup", None)
    _simple(f"amax_parts_{_n}", (lambda su: lambda cx: (cx.set(amax_parts=True, weight_planes=True), su and su(cx)))(_su), out_amax=True, **_kw)

# ---- per-call options
_simple("plan_override_cfg", lambda cx: cx.set(plan_override=(2, 3, -1)))
_simple("plan_override_no_tail", lambda cx: cx.set(plan_override=(-1, 0, 0)), a=None, scales="pairs")
_simple("plan_override_forced_tail", lambda cx: cx.set(plan_override=(0, -2, 1)), lay="dgrad")
_simple("tails_on", lambda cx: cx.be.set_tail_launches(True))
_simple("tails_off", lambda cx: cx.be.set_tail_launches(False))
_simple("tails_pinned", lambda cx: (cx.be.pin_tail_launches(False), cx.be.set_tail_launches(True)))
_simple("tails_unpinned", lambda cx: (cx.be.pin_tail_launches(True), cx.be.pin_tail_launches(None), cx.be.set_tail_launches(False)))
_simple("splitk_reduce_1", lambda cx: cx.set(splitk_reduce=1))
_simple("splitk_reduce_2", lambda cx: cx.set(splitk_reduce=2), lay="wgrad")
_simple("dropout_salt", lambda cx: cx.be.enable_dropout_salt(device="cpu"), drop_p=0.5, drop_seed=11)
_simple("dropout_salt_disabled", lambda cx: (cx.be.enable_dropout_salt(device="cpu"), cx.be.disable_dropout_salt()), drop_p=0.5, drop_seed=11)

# ---- every ValueError of `gemm` (the pair-only ones are above)
_simple("err_shape_a", a_shape=(64, 32))
_simple("err_shape_b", b_shape=(32, 64))
_simple("err_shape_out", out=dict(shape=(64, 32)))
_simple("err_k0", K=0)
_simple("err_weight_dtype", b=BF16)
_simple("err_layout", lay="bad")
_simple("err_maxima_split", scales="row_short")
_simple("err_maxima_wpairs", WP, scales="row_short")
_simple("err_bf16_out_alignment", out=dict(dtype=BF16, off=1))
_simple("err_bf16_res_ld", res=dict(dtype=BF16, ld=66))
_simple("err_out2_shape", out2=dict(shape=(64, 32)))
_simple("err_accumulate_bf16", out=BF16, accumulate=True)
_simple("err_out2_type_bf16", out=F32, out2=BF16)
_simple("err_out2_type_f32", out=BF16, out2=F32)
_simple("err_bias_length", bias=(63, F32))
_simple("err_bias_dtype", bias=(64, BF16))
_simple("err_res_shape", res=dict(shape=(64, 32)))
_simple("err_res_ln_without_res", res_ln=True)
_simple("err_res_ln_bf16_res", res=BF16, res_ln=True)
_simple("err_res_ln_native", res=F32, res_ln=True, precision="f32")
_simple("err_res_ln_small", res=F32, res_ln=True, M=32)
_simple("err_res_ln_length", res=F32, res_ln=dict(gamma=63))
_simple("err_aux_shape", aux=dict(shape=(32, 64)))
_simple("err_pre_shape", pre=dict(shape=(32, 64)))
_simple("err_pre_dtype", pre=BF16)
_simple("err_colsum_layout", colsum=True)
_simple("err_colsum_length", lay="wgrad", colsum=63)
_simple("err_out_rows_overlap", out=dict(ld=32))
_simple("err_precision_name", precision="f64")


@scenario
def err_a_inner_stride(cx):
    cx.naming = "a"
    a = torch.zeros(64, 128)[:, ::2]
    cx.naming = None
    cx.gemm(a=a)


# ---- gemm_group
def _group(cx, step, specs):
    calls = [cx.gemm(defer=True, p=f"g{i}_", **s) for i, s in enumerate(specs)]
    cx.step(step, lambda: cx.be.gemm_group(calls))


@scenario
def group_together(cx):
    _group(cx, "group", [dict(scales="row", bias=True, out_amax=True), dict(N=96), dict(K=96, res=F32), dict(M=96)])


@scenario
def group_of_five(cx):
    _group(cx, "group", [dict(a=None, scales="pairs")] * 5)


@scenario
def group_split_by_key(cx):
    WP(cx)
    _group(cx, "group", [dict(), dict(), dict(lay="dgrad"), dict(lay="dgrad"), dict(a=None, scales="pairs"), dict(a=None, scales="pairs"),
                         dict(precision="f32_bf16x6"), dict(precision="f32_bf16x6")])


@scenario
def group_wpairs(cx):
    WP(cx)
    _group(cx, "group", [dict(scales="parts"), dict(lay="fwd")])


@scenario
def group_pairs_both_layouts(cx):
    _group(cx, "group", [dict(a=None, scales="pairs"), dict(a=None, scales="pairs", lay="dgrad"), dict(), dict(lay="dgrad")])


@scenario
def group_wpairs_both_layouts(cx):
    WP(cx)
    _group(cx, "group", [dict(), dict(lay="dgrad"), dict(a=None, scales="pairs", lay="dgrad"), dict(M=63), dict(M=63)])


@scenario
def group_non_groupable_member(cx):
    _group(cx, "group", [dict(), dict(M=16), dict(), dict(out=BF16), dict(a=BF16), dict(lay="wgrad"), dict(), dict(M=0), dict()])


@scenario
def group_launches_off(cx):
    cx.set(group_launches=False)
    _group(cx, "group", [dict(), dict()])


@scenario
def group_refused_by_library(cx):
    cx.group_rc = -1
    _group(cx, "group", [dict(out_amax=True), dict(), dict()])


@scenario
def group_plan_override(cx):
    cx.set(plan_override=(1, 2, 0))
    _group(cx, "group", [dict(), dict(), dict(M=16)])


@scenario
def group_error_in_member(cx):
    _group(cx, "group", [dict(), dict(K=0)])


# ---- gemm_wgrad
@scenario
def wgrad_outside_a_pass(cx):
    cx.wgrad(db=True)
    cx.wgrad("rows_given", zs="row", xs="parts", p="b_")


@scenario
def wgrad_pairs_either_side(cx):
    cx.wgrad("pz", dz=None, zs="pairs", db=True)
    cx.wgrad("px", x=None, xs="pairs", p="b_")
    cx.wgrad("both", dz=None, x=None, zs="pairs", xs="pairs", p="c_")
    cx.wgrad("both_with_fp32", zs="pairs", xs="pairs", p="d_")


@scenario
def wgrad_pairs_refused(cx):
    cx.wgrad("width", Np=48, zs="pairs")
    cx.wgrad("width_raises", Np=48, dz=None, zs="pairs", p="b_")
    cx.wgrad("shape_raises", x=None, xs="pairs_shape", p="c_")
    cx.set(wgrad_column_maxima=True)
    cx.wgrad("column_maxima", zs="pairs", xs="pairs", p="d_")
    cx.wgrad("column_maxima_raises", dz=None, zs="pairs", p="e_")


@scenario
def wgrad_falls_through(cx):
    cx.wgrad("bf16_dz", dz=BF16, x=BF16, db=True)
    cx.wgrad("bf16_x", x=BF16, p="b_")
    cx.wgrad("narrow_n", Np=32, p="c_", zs="row")
    cx.wgrad("narrow_k", Kp=32, p="d_")
    cx.wgrad("no_tokens", T=0, p="e_")
    cx.set(defer_wgrads=False)
    cx.wgrad("switch_off", p="f_", db=True, xs="row")
    cx.set(defer_wgrads=True)
    cx.be.set_gemm_precision_bwd("f32")
    cx.wgrad("native_precision", p="g_")


@scenario
def wgrad_other_arithmetic(cx):
    cx.be.set_gemm_precision_bwd("bf16x3")
    cx.wgrad("bf16x3", db=True, zs="pairs")
    cx.be.set_gemm_precision_bwd(None)
    cx.set(wgrad_column_maxima=True)
    cx.wgrad("column_maxima", p="b_", zs="row")


@scenario
def wgrad_errors(cx):
    cx.wgrad("shape", dz_shape=(64, 48))
    cx.wgrad("db_length", db=63, p="b_")
    cx.wgrad("dz_rows_overlap", dz_ld=32, p="c_")


@scenario
def wgrad_options(cx):
    cx.be.enable_dropout_salt(device="cpu")
    cx.set(splitk_reduce=2, plan_override=(2, 3, 1))
    cx.be.set_tail_launches(False)
    cx.wgrad()


@scenario
def wgrad_queue_of_sixteen(cx):
    cx.backward("pass", lambda: [cx.wgrad(p=f"q{i}_", Np=64 + 32 * (i % 2), db=i % 3 == 0, zs="row", xs="parts", run=False)() for i in range(18)])


@scenario
def wgrad_queue_byte_budget(cx):
    cx.set(wgrad_queue_bytes=3 * 64 * 64 * 4)
    cx.backward("pass", lambda: [cx.wgrad(p=f"q{i}_", run=False, **kw)() for i, kw in enumerate([{}, {}, dict(dz=None, zs="pairs"), {}, {}])])


@scenario
def wgrad_load_partition(cx):
    specs = [{}, dict(Kp=513), dict(dz_off=1), dict(x=None, xs="pairs"), dict(x_ld=66), dict(Np=66, Kp=66), dict(dz=None, zs="pairs", Kp=513)]
    cx.backward("pass", lambda: [cx.wgrad(p=f"q{i}_", run=False, **kw)() for i, kw in enumerate(specs)])


@scenario
def wgrad_two_streams_and_aside(cx):
    def body():
        r = [cx.wgrad(p="m0_", run=False)()]
        with cx.on(9):
            r.append(cx.wgrad(p="h0_", run=False)())
            r.append(cx.wgrad(p="h1_", run=False)())
            cx.be.launch_wgrads_aside()
            r.append(cx.wgrad(p="h2_", run=False)())
        r.append(cx.wgrad(p="m1_", run=False)())
        cx.be.launch_wgrads_aside(all_streams=True)
        r.append(cx.wgrad(p="m2_", run=False)())
        with cx.on(9):
            r.append(cx.wgrad(p="h3_", run=False)())
        return r
    cx.backward("pass", body)
    cx.step("flush_outside", lambda: cx.be.flush_wgrads())


@scenario
def wgrad_flush_outside_discards_dead_pass(cx):
    def dies():
        cx.wgrad(p="q0_", run=False)()
        raise RuntimeError("the pass dies")
    cx.backward("dead_pass", dies)
    cx.step("flush_outside", lambda: cx.be.flush_wgrads())
    cx.wgrad("next", p="n_")


@scenario
def layernorm_reductions_deferred(cx):
    M, W = 48, 64
    g = [cx.vec(f"gamma{i}", W) for i in range(2)]
    dg, db = [cx.vec(f"dgamma{i}", W) for i in range(2)], [cx.vec(f"dbeta{i}", W) for i in range(2)]
    mean, rstd = cx.vec("mean", M), cx.vec("rstd", M)

    def body():
        r = []
        for i in (0, 1, 0):                      # (the third: a parameter whose reduction is queued already reduces at once)
            r.append(cx.be.layernorm_bwd(cx.mat(f"dy{len(r)}", F32, (M, W)), cx.mat(f"x{len(r)}", F32, (M, W)), mean, rstd, g[i], cx.mat(f"dx{len(r)}", F32, (M, W)),
                                         dg[i], db[i]))
        with cx.on(9):
            r.append(cx.wgrad(p="w_", run=False)())
        return r
    cx.backward("pass", body)
    cx.step("outside", lambda: cx.be.layernorm_bwd(cx.mat("dy_o", F32, (M, W)), cx.mat("x_o", F32, (M, W)), mean, rstd, g[0], cx.mat("dx_o", F32, (M, W)), dg[0], db[0]))


# ---- the per-weight caches
def _cache_states(cx, **kw):
    """one weight through: first use, hit, stale by version counter, stale by epoch (batched refresh with a second weight registered)"""
    (_, w, _), _ = cx.gemm("first", **kw)
    cx.gemm("hit", b=w, p="h_", **kw)
    cx.touch(w)
    cx.gemm("stale_by_version", b=w, p="v_", **kw)
    (_, w2, _), _ = cx.gemm("second_weight", p="w2_", **dict(kw, N=96))
    cx.be.invalidate_weights()
    cx.gemm("stale_by_epoch", b=w, p="e_", **kw)
    cx.gemm("second_weight_after_refresh", b=w2, p="e2_", **dict(kw, N=96))
    with cx.on(9):
        cx.gemm("other_stream_after_refresh", b=w2, p="s_", **dict(kw, N=96))
    return w, w2


SCENARIOS["cache_maxima_fwd"] = lambda cx: _cache_states(cx, lay="fwd")
SCENARIOS["cache_pairs_dgrad"] = lambda cx: _cache_states(cx, lay="dgrad", a=None, scales="pairs")
SCENARIOS["cache_wpairs_fwd"] = lambda cx: (WP(cx), _cache_states(cx, lay="fwd"))
SCENARIOS["cache_planes_dgrad"] = lambda cx: _cache_states(cx, lay="dgrad", a=BF16)


@scenario
def cache_entries_age_out(cx):
    (_, w, _), _ = cx.gemm("first", a=None, scales="pairs")
    (_, w2, _), _ = cx.gemm("second_weight", p="w2_", a=None, scales="pairs", N=96)
    cx.be.invalidate_weights()
    cx.gemm("w2_epoch_2", b=w2, p="a_", a=None, scales="pairs", N=96)
    cx.be.invalidate_weights()
    cx.gemm("w2_epoch_3", b=w2, p="b_", a=None, scales="pairs", N=96)          # w: unused since the step before last, leaves both tables
    cx.gemm("w_again", b=w, p="c_", a=None, scales="pairs")


@scenario
def cache_weight_replaced_in_place(cx):
    """a weight freed and another tensor object at the same address, with the same shape and version count"""
    for kw in (dict(), dict(a=None, scales="pairs"), dict(a=BF16)):
        tag = "split" if not kw else ("pairs" if "scales" in kw else "planes")
        base = cx.mat(tag + "_w", F32, (64, 64))
        w = base.detach().requires_grad_()
        cx.gemm(tag + "_first", b=w, p=tag + "1_", **kw)
        del w
        w = base.detach().requires_grad_()
        cx.gemm(tag + "_replaced", b=w, p=tag + "2_", **kw)


@scenario
def cache_odd_width_weight(cx):
    """a weight the batched maxima kernel cannot take refreshes by a pass of its own, into the arrays it has"""
    (_, w, _), _ = cx.gemm("first", K=34)
    (_, w2, _), _ = cx.gemm("batchable", p="w2_")
    cx.be.invalidate_weights()
    cx.gemm("stale_by_epoch", b=w, K=34, p="e_")
    cx.gemm("batchable_stale", b=w2, p="e2_")
    cx.touch(w)
    cx.gemm("stale_by_version", b=w, K=34, lay="fwd", p="v_")
    (_, w3, _), _ = cx.gemm("odd_stride", b_ld=66, p="w3_")
    cx.be.invalidate_weights()
    cx.gemm("odd_stride_stale", b=w3, p="e3_")


@scenario
def to_pairs_and_amax(cx):
    x = cx.mat("x", F32, (48, 40))
    cx.step("to_pairs", lambda: cx.be.to_pairs(x))
    cx.step("to_pairs_have_parts", lambda: cx.be.to_pairs(x, cx.scales("have", "parts", 48, 40)))
    cx.step("amax_all", lambda: cx.be.amax(x, None, rows=True, cols=True, tmax=True))
    cx.step("amax_tmax_from_parts", lambda: cx.be.amax(x, cx.scales("have2", "parts", 48, 40), tmax=True))
    cx.step("pairs_ok", lambda: [cx.be.pairs_ok(x, 64), cx.be.pairs_ok(x, 40), cx.be.pairs_ok(x, 64, training=True), cx.be.training_pairs_ok(12288, 64),
                                 cx.be.training_pairs_ok(12288, 32), cx.be.training_pairs_ok(100, 64)])


# ---------------------------------------------------------------------------------------------------- driver
def run_scenario(name, mp):
    """-> the trace as lines of text: `symbol(arguments)` per library call (without the grappa_ prefix), `{step=...}` after the calls of a step"""
    cx = _Cx(mp)
    SCENARIOS[name](cx)
    out = [_txt(e) if isinstance(e, dict) else f"{e[0].replace('grappa_', '')}({', '.join(_txt(v) for v in e[1:])})" for e in cx.out]
    assert not any("?" in e for e in out if not e.startswith("{step=")), f"{name}: a pointer into memory the recorder does not know"
    return out


# the scenarios whose trace the fixture holds line by line; of the others it holds a digest of the same lines
IN_FULL = {"split_fwd", "split_dgrad", "pairs_fwd", "pairs_dgrad", "wpairs_fwd_at_threshold", "wpairs_dgrad_at_threshold", "bf16_a_planes_fwd",
           "bf16_a_planes_dgrad", "weight_planes_fwd", "weight_planes_dgrad", "native_small_m_fwd", "native_precision_bf16_out_dgrad", "wgrad_f32",
           "wgrad_bf16_planes", "epi_pairs_everything", "plan_override_cfg", "group_together", "wgrad_pairs_either_side", "cache_pairs_dgrad"}


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_table_and_fixture_hold_the_same_scenarios():
    fx = _fixture()
    assert sorted(fx) == sorted(SCENARIOS)
    assert {n for n, v in fx.items() if isinstance(v, list)} == IN_FULL


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_front_end_trace(name, monkeypatch):
    want = _fixture()[name]
    got = run_scenario(name, monkeypatch)
    if isinstance(want, str):
        assert _digest(got) == want, f"{name}: the trace changed; `--show {name}` prints it (for the pinned one: with the parent commit first on PYTHONPATH):\n" + "\n".join(got)
        return
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: entry {i} differs"
    assert len(got) == len(want)


def _write():
    lines = []
    for name in sorted(SCENARIOS):
        with pytest.MonkeyPatch.context() as mp:
            entries = run_scenario(name, mp)
        if name in IN_FULL:
            lines.append(f" {json.dumps(name)}: [\n" + ",\n".join("  " + json.dumps(e) for e in entries) + "\n ]")
        else:
            lines.append(f" {json.dumps(name)}: {json.dumps(_digest(entries))}")
    with open(FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")
    print(f"{FIXTURE}: {len(SCENARIOS)} scenarios from {backend.__file__}")


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        _write()
    elif len(sys.argv) == 3 and sys.argv[1] == "--show" and sys.argv[2] in SCENARIOS:
        with pytest.MonkeyPatch.context() as mp:
            print("\n".join(run_scenario(sys.argv[2], mp)))
    else:
        sys.exit("usage: PYTHONPATH=<checkout of the parent commit> python tests/test_dense_front_end_trace.py --write | --show SCENARIO")
