"""The dense products' routes: one record per case of tests/test_gpu_gemm_routes.py, a Python restatement of the host-side routing
(route_of: which kernel family, tile, loads, way to finish the product and epilogue site a descriptor reaches), the CPU operand
generator of the sweep, and the calibration of the gate's only free constant.

A case's id spells its route: <kernel>-<tile>-<layout>-<loads>-<finish>-<epilogue site>-<epilogue form>, e.g.
`h3-256x128-dgrad-vec-splitk3-inkernel-inkernel-i` or `pairs_il-128x128-fwd-dma-tail2-tail_cls3-d`.
    kernel   native | x9 x6 x3 x1 h3 (gemm_bf16x_impl.h) | wplanes_<x> planes_<x> bf16_il (gemm_planes.hip, gemm_pairs_il.hip) |
             pairs_il pairs_loop (gemm_pairs_il.hip / gemm_pairs.hip) | wpairs_il wpairs_loop (gemm_wpairs_il.hip / gemm_pairs.hip)
    loads    vec (16-byte) | scalar | dma (plane and pair operands)
    finish   nosplit | splitk<n>-reduce | splitk<n>-inkernel | tail<n> (main launch + split-K tail launch)
    site     native native_reduce | cls1-5 cls9-12 (epilogue_band_fast) | walk (epilogue_band's vector walk) | ragged (N % 4 != 0: the last
             quad through epilogue_store) | misaligned (vec_io false: every element through epilogue_store) | reduce inkernel
             (splitk_reduce_quad) | tail_<site of the main launch> | g4_<site> (grappa_gemm_f32_group) | grouped grouped_reduce grouped_inkernel

Unreachable from the entry points (no case, by route_of):
  * grappa_launch_gemm_pairs' second reason for the round-3 loop, a split range that is not a multiple of 32: make_plan rounds the ranges
    of pair products to 32 (kround), so only a short last range (K < 64, or a forced split that leaves fewer than 64 columns) reaches it;
  * make_plan's rounding of k_per_split to 64 (bf16_il_tile): grappa_gemm_f32 always passes planes_tile = 0, the 256 x 256 and 128 x 128
    tiles of the bf16 pipeline are planned only for the workspace query; the bf16 pipeline's `(k_per_split & 63) == 0` falls back to the
    plane kernel instead (case planes_x1-...-K%64);
  * grappa_launch_gemm_pairs' refusal of a_amax_nseg > 1 on the round-3 weight-pairs loop: grappa_gemm_f32 refuses the descriptor first
    with the same predicate (REFUSALS: single-wpairs_nseg_on_loop).

Calibration of c_acc (kernel_refs.gemm_bound).  r = max |fp32 CPU product - float64| / (u32 S) over every product of the table, on the
sweep's own operands (tests/test_kernel_domain_refs.py::test_c_acc_is_twice_the_cpu_references_error measures it again):
    torch.matmul (fp32)                                    8.57   (the 17 M elements of the widest main + tail case; its blocking depends on the CPU: the test asserts the gate, not the figure)
    sequential fp32 chain over exact blocks of 8 columns   2.80   (deterministic)
c_acc = 2 * the larger = 17.1, one value for the whole sweep."""
import ctypes as C
import zlib
from dataclasses import dataclass, replace

import torch

import kernel_refs as kr

# measured by calibrate() on this table (max over all products): see the module docstring
R_MATMUL = 8.57
R_CHAIN = 2.80
C_ACC = 2.0 * max(R_MATMUL, R_CHAIN)

CFG_BM = [128, 64, 128, 32, 128, 128, 256, 256, 128]          # gemm_f32.hip CFG_BM / CFG_BN
CFG_BN = [128, 64, 32, 128, 64, 128, 128, 256, 128]
NCU = 256                                                       # gemm_f32.hip plan_cus()
KERNEL_OF = {"f32_bf16x9": "x9", "f32_bf16x6": "x6", "bf16x3": "x3", "bf16": "x1", "f32_f16x3": "h3"}


def _form(**kw):
    f = dict(pre=0, bias=0, act=0, aux=0, drop=0.0, res=0, res_ln=0, c2=0, acc=0, colsum=0, cp=0, resp=0, auxp=0, c1p=0)
    f.update(kw)
    return f


# section 4 of the issue; m5 (bf16 tensor + ELU) is added for fast class 10
FORMS = {
    "a": _form(), "b": _form(bias=1), "c": _form(bias=1, act=1), "d": _form(bias=1, drop=0.3, res=1), "e": _form(drop=0.5),
    "f": _form(aux=1), "g": _form(aux=1, res=1), "h": _form(bias=1, drop=0.25, res=1, res_ln=1),
    "i": _form(bias=1, act=1, drop=0.3, res=1, c2=1), "j": _form(pre=1, bias=1, act=1, res=1, c2=1), "k": _form(acc=1, bias=1),
    "l": _form(acc=1, colsum=1),
    "m1": _form(cp=1), "m2": _form(cp=1, resp=1), "m3": _form(cp=1, auxp=1, resp=1), "m4": _form(bias=1, drop=0.3, cp=1, c1p=1),
    "m5": _form(bias=1, act=1, cp=1),
    "n": _form(bias=1, cp=3, resp=3),
}
BF16_FORMS = ("m1", "m2", "m3", "m4", "m5", "n")


@dataclass(frozen=True)
class Case:
    route: str                   # declared: what the case is for (checked against route_of)
    site: str
    form: str
    M: int
    N: int
    K: int
    entry: str = "single"        # single | group4 | grouped
    fmt: str = "f32"             # f32 | wplanes | planes | pairs | wpairs (planes with arith bf16 = the one-plane bf16 product);
                                 # members of a grouped entry: f32 | pa | pb | pab (A, B or both as token-major pairs, C ABI 8)
    layout: str = "fwd"          # fwd | dgrad | wgrad
    arith: str = "f32_f16x3"
    cfg: int = 0                 # plan_cfg (tile index + 1; 0: the plan's own)
    nsplit: int = 0              # plan_nsplit
    tail: int = 2                # plan_tail
    reduce: int = 0              # splitk_reduce
    ld_extra: int = 0            # ldc = N + ld_extra (every fp32 epilogue tensor; bf16 tensors: ld = round_up(N, 4) + ld_extra)
    c_off: int = 0               # the fp32 epilogue tensors start c_off elements behind a 16-byte boundary
    op_extra: int = 0            # lda / ldb = round_up(row length, 4) + op_extra (fp32 operands)
    a_off: int = 0               # A starts a_off elements behind a 16-byte boundary (fp32 operands)
    amax: str = ""               # "" | out | parts
    a_nseg: int = 0              # a_amax given as this many per-segment partial arrays (a_amax_nseg)
    bcast: int = 0               # amax_bcast
    scaled: int = -1             # rows of A scaled by 2^U(-6, 6): 1 / 0; -1 = by the parity of the id's checksum
    members: tuple = ()          # group entries: the member products
    tag: str = ""

    @property
    def id(self):
        return "-".join(x for x in (self.route, self.site, self.form, self.amax and "amax_" + self.amax, self.tag) if x)

    @property
    def f(self):
        return FORMS[self.form]

    @property
    def planes(self):
        return self.fmt != "f32"

    @property
    def pairs(self):
        return self.fmt in ("pairs", "wpairs")

    @property
    def ldc(self):
        return self.N + self.ld_extra

    @property
    def rows_scaled(self):
        return bool(self.scaled) if self.scaled >= 0 else bool(zlib.crc32(self.id.encode()) & 1)

    def op_ld(self, which):
        """leading dimension of an fp32 operand as stored: A[M][K] / A[K][M] (wgrad); B[N][K] (fwd) / B[K][N]"""
        n = (self.K if self.layout != "wgrad" else self.M) if which == "a" else (self.K if self.layout == "fwd" else self.N)
        return (n + 3) // 4 * 4 + self.op_extra


# ------------------------------------------------------------------------------------------------------------------ the routing, restated
def plan_query(c):
    """grappa_gemm_f32_plan_desc (host only): -> (tile_m, tile_n, nsplit, tail_tiles, tail_nsplit) or None when refused"""
    from grappa_amd import _lib
    lib = _lib.load()
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.precision = c.M, c.N, c.K, _lib.GEMM_PRECISIONS[c.arith]
    d.plan_cfg, d.plan_nsplit, d.plan_tail, d.splitk_reduce = c.cfg, c.nsplit, c.tail, c.reduce
    out = [C.c_int() for _ in range(5)]
    rc = lib.grappa_gemm_f32_plan_desc(C.byref(d), *[C.byref(o) for o in out])
    return None if rc != 0 else tuple(o.value for o in out)


def use_bf16x(c):
    """gemm_f32.hip use_bf16x, and `planes ||` of grappa_gemm_f32 (bf16x = planes || use_bf16x)"""
    return c.planes or (c.arith != "f32" and c.M > 32 and c.N > 32)


def loads_vec(c):
    """gemm_f32.hip grappa_gemm_f32: vecA && vecB && padA && padB (fp32 operands; B always starts on a 16-byte boundary here)"""
    a_k, b_k = c.layout != "wgrad", c.layout == "fwd"
    lda, ldb = c.op_ld("a"), c.op_ld("b")
    vec_a = c.a_off % 4 == 0 and lda % 4 == 0 and (not a_k or c.K % 4 == 0)
    vec_b = ldb % 4 == 0 and (not b_k or c.K % 4 == 0)
    pad_a = a_k or (c.M + 3) // 4 * 4 <= lda
    pad_b = b_k or (c.N + 3) // 4 * 4 <= ldb
    return vec_a and vec_b and pad_a and pad_b


def vec_io(c):
    """gemm_f32.hip p.vec_io: al16 of C, C2, pre, res, aux (the sweep gives them one offset and one leading dimension)"""
    f = c.f
    has_f32 = not (f["cp"] and not f["c2"]) or f["pre"] or (f["res"] and not f["resp"]) or (f["aux"] and not f["auxp"])
    return (not has_f32) or (c.c_off % 4 == 0 and c.ldc % 4 == 0)


def epi_class(c):
    """gemm_f32.hip choose_epi_class"""
    f = c.f
    has_c = not f["cp"]                       # (the sweep's bf16-tensor forms pass C = NULL)
    if not (use_bf16x(c) and c.N % 4 == 0 and not f["c2"] and not f["c1p"] and not f["pre"] and not f["acc"]):
        return 0
    f32_only = vec_io(c) and has_c and not f["cp"] and not f["resp"] and not f["auxp"]
    bf16_only = f["cp"] == 1 and not has_c and not (f["res"] and not f["resp"]) and not (f["aux"] and not f["auxp"]) and f["resp"] in (0, 1) and f["auxp"] in (0, 1)
    if not (f32_only or bf16_only):
        return 0
    has_aux, has_res = bool(f["aux"] or f["auxp"]), bool(f["res"] or f["resp"])
    if has_aux:
        cls = 4 if (not f["bias"] and not f["act"] and f["drop"] == 0) else 0
    elif f["act"]:
        cls = 2 if (f["drop"] == 0 and not has_res) else 0
    else:
        cls = 3 if (f["drop"] > 0 or has_res) else 1
    if cls == 3 and f["res_ln"]:
        cls = 5 if f32_only else 0
    return 0 if cls == 0 else cls + (8 if bf16_only else 0)


def split_ladder(K, mk=1):
    """make_plan's candidate split factors: 1, 2, 3, 4, 5, 7, 9, 12, ... up to K / (mk * 32) (at most 64)"""
    max_split = K // (mk * 32) if K >= 2 * mk * 32 else 1
    ns, out = 1, []
    while ns <= min(max_split, 64):
        out.append(ns)
        ns = ns + 1 if ns < 4 else ns + (ns + 3) // 4
    return out


def forced_plan(c):
    """make_plan for plane / pair operands under a forced tile and a forced plan_nsplit (the records force both, so that the cost model
    has no say): -> (cfg index, nsplit, k_per_split, tail_tiles, tail_nsplit, tail_k_per_split) (a forced tile other than the pair kernels' three is ignored for these operands)"""
    assert c.planes and c.nsplit >= 1, c.id
    both_pairs = c.fmt == "pairs"
    cfg = 6                                                   # the plane kernels and fp32 A + weight pairs: 256 x 128 (pairs_cfg)
    if c.cfg:
        if both_pairs and c.cfg - 1 in (6, 7, 8):
            cfg = c.cfg - 1                                   # forced_pairs
        elif c.pairs and c.cfg - 1 in (6, 7, 8):
            cfg = c.cfg - 1                                   # (fp32 A + weight pairs: grappa_gemm_f32 then refuses cfg != 6)
    mk = 8 if not c.pairs else 1
    want = max(ns for ns in split_ladder(c.K, mk) if ns <= c.nsplit)
    rnd = lambda k: (k + 31) // 32 * 32                       # noqa: E731   (kround: 32 for pairs, BK = 32 otherwise)
    kps = rnd(-(-c.K // want))
    nsplit = -(-c.K // kps)
    tiles = -(-c.M // CFG_BM[cfg]) * -(-c.N // CFG_BN[cfg])
    rem = tiles % NCU
    if c.tail == 3 and nsplit == 1 and tiles > NCU and 0 < rem <= NCU * 5 // 8:
        max_tail = min(c.K // 128, 64) if c.K >= 256 else 1
        ts = min(NCU // rem, max_tail)
        tkps = rnd(-(-c.K // ts))
        tns = -(-c.K // tkps)
        if tns >= 2:
            return cfg, nsplit, kps, rem, tns, tkps
    return cfg, nsplit, kps, 0, 0, 0


def wpairs_il_takes(K, nsplit, kps):
    """gemm_common.h grappa_wpairs_il_takes"""
    return K % 32 == 0 and kps % 32 == 0 and K - (nsplit - 1) * kps >= 64


def pairs_il_takes(K, nsplit, kps):
    """gemm_pairs.hip grappa_launch_gemm_pairs: kk >= 4 * QSLAB && (nsplit == 1 || (k_per_split & 31) == 0)"""
    return K - (nsplit - 1) * kps >= 64 and (nsplit == 1 or kps % 32 == 0)


def bf16_il_takes(c, nsplit, kps):
    """gemm_planes.hip grappa_launch_gemm_planes, GRAPPA_GEMM_BF16 with both operands in planes (the tile is 256 x 128 by the plan)"""
    return c.layout == "fwd" and c.K % 64 == 0 and kps % 64 == 0 and c.K - (nsplit - 1) * kps >= 128


def site_of(c, nsplit, in_kernel):
    if not use_bf16x(c):
        return "native" if nsplit == 1 else "native_reduce"
    if nsplit > 1:
        return "inkernel" if in_kernel else "reduce"
    cls = epi_class(c)
    if cls:
        return f"cls{cls}"
    if not vec_io(c):
        return "misaligned"
    return "ragged" if c.N % 4 else "walk"


def group_psrc(members):
    """gemm_f32.hip grappa_gemm_f32_grouped: the operand-format specialisation of a group"""
    bits = [(1 if m.fmt in ("pa", "pab") else 0) | (2 if m.fmt in ("pb", "pab") else 0) for m in members]
    return bits[0] if all(b == bits[0] for b in bits) else 4


def group_plan(members):
    """gemm_f32.hip plan_group: one K chunk for the whole group -> (kps, [nsplit per member])"""
    tiles = [-(-m.M // 256) * -(-m.N // 128) for m in members]
    work = float(sum(t * m.K for t, m in zip(tiles, members)))
    kmax = (max(m.K for m in members) + 31) // 32 * 32
    best, best_kps = 1e300, kmax
    for R in range(1, 13):
        kps = (int(work / (256.0 * R)) + 31) // 32 * 32
        kps = min(max(kps, 1024), kmax)
        wgs, slab = 0, 0.0
        for t, m in zip(tiles, members):
            ns = -(-m.K // kps)
            wgs += t * ns
            if ns > 1:
                slab += ns * m.M * m.N / 200.0
        cost = float((wgs + 255) // 256) * 32768.0 * (kps + 160.0) / 307.0 + slab
        if cost < best:
            best, best_kps = cost, kps
    return best_kps, [-(-m.K // best_kps) for m in members]


def group_vec(members):
    """grappa_gemm_f32_grouped: 16-byte loads along the rows of both operands of every product"""
    return all(m.a_off % 4 == 0 and m.op_ld("a") % 4 == 0 and (m.M + 3) // 4 * 4 <= m.op_ld("a") and
               m.op_ld("b") % 4 == 0 and (m.N + 3) // 4 * 4 <= m.op_ld("b") for m in members if m.fmt == "f32")


def route_of(c):
    """-> (route, site) of a record, or ("refused", "") where the routing itself refuses it"""
    if c.entry == "grouped":
        psrc = group_psrc(c.members)
        _, ns = group_plan(c.members)
        vec = group_vec(c.members)
        chunks = (len(c.members) + 7) // 8
        split = "mixedsplit" if (max(ns) > 1 and min(ns) == 1) else ("split" if max(ns) > 1 else "nosplit")
        site = "grouped" if max(ns) == 1 else ("grouped_inkernel" if c.members[0].reduce == 2 else "grouped_reduce")
        return f"grouped_{KERNEL_OF[c.arith]}-psrc{psrc}-{'vec' if vec else 'scalar'}-n{len(c.members)}-chunk{chunks}-{split}", site
    if c.entry == "group4":
        kern = "pairs" if c.fmt == "pairs" else KERNEL_OF[c.arith]
        return f"group4_{kern}-256x128-{c.layout}-n{len(c.members)}", "+".join("g4_" + site_of(m, 1, False) for m in c.members)
    if c.fmt == "f32":
        q = plan_query(c)
        if q is None:
            return "refused", ""
        bm, bn, nsplit, tail_tiles, tns = q
        bf16x = use_bf16x(c)
        kern = KERNEL_OF[c.arith] if bf16x else "native"
        loads = "vec" if loads_vec(c) else "scalar"
        in_kernel = bf16x and c.reduce == 2                    # gemm_f32.hip launch: bf16x && !planes && splitk_in_kernel
    else:
        q = forced_plan(c)
        if q is None:
            return "refused", ""
        cfg, nsplit, kps, tail_tiles, tns, tkps = q
        bm, bn = CFG_BM[cfg], CFG_BN[cfg]
        loads, in_kernel = "dma", False
        x = KERNEL_OF[c.arith] if c.arith != "f32" else "x6"
        launches = [(nsplit, kps)] + ([(tns, tkps)] if tail_tiles else [])
        if c.fmt == "pairs":
            names = ["pairs_il" if pairs_il_takes(c.K, n, k) else "pairs_loop" for n, k in launches]
        elif c.fmt == "wpairs":
            names = ["wpairs_il" if wpairs_il_takes(c.K, n, k) else "wpairs_loop" for n, k in launches]
        elif c.fmt == "wplanes":
            names = [f"wplanes_{x}"]
        elif c.arith == "bf16":
            names = ["bf16_il" if bf16_il_takes(c, n, k) else "planes_x1" for n, k in launches]
        else:
            names = [f"planes_{x}"]
        kern = "+".join(dict.fromkeys(names))
    if tail_tiles:
        finish, site = f"tail{tns}", "tail_" + site_of(c, 1, False)
    elif nsplit > 1:
        finish = f"splitk{nsplit}-" + ("inkernel" if in_kernel else "reduce")
        site = site_of(c, nsplit, in_kernel)
    else:
        finish, site = "nosplit", site_of(c, 1, False)
    if c.a_nseg > 1:
        kern += "_nseg"
    return f"{kern}-{bm}x{bn}-{c.layout}-{loads}-{finish}", site


# ------------------------------------------------------------------------------------------------------------------ the table
# a tail launch needs more than 256 tiles: 257 rows of tiles, one column of tiles (the fewest elements that reach it), 100 rows in the tail
TAIL_ROWS, TAIL_N = 256, 36


def _tile(cfg):
    return f"{CFG_BM[cfg]}x{CFG_BN[cfg]}"


def _variants(kern, cfg, fmt, arith, in_kernel_too):
    """the form x site matrix on one carrier (forward layout): aligned, ragged N, misaligned output, split-K with the reduction launch,
    split-K finished in the launch, main + tail launch"""
    t, out = _tile(cfg), []
    loads = "vec" if fmt == "f32" else "dma"
    big_m = TAIL_ROWS * CFG_BM[cfg] + 100
    for i, form in enumerate(FORMS):
        if form in ("l", "n"):
            continue                                              # (wgrad layout only / the plane kernels only)
        base = dict(form=form, fmt=fmt, arith=arith, cfg=cfg + 1, K=160, tag="fx")
        pad = 8 * (i % 2)
        amax = ("out", "", "")[i % 3] if form not in BF16_FORMS else ""
        c0 = Case(f"{kern}-{t}-fwd-{loads}-nosplit", "", M=300, N=192, nsplit=1, ld_extra=pad, amax=amax, **base)
        out.append(replace(c0, site=site_of(c0, 1, False)))
        if form != "h":                                           # (res_ln_*: N % 4 == 0)
            c1 = replace(c0, N=190, ld_extra=2 + pad, amax="parts" if (i % 3 == 2 and form not in BF16_FORMS) else "")
            out.append(replace(c1, site=site_of(c1, 1, False)))
        if form not in BF16_FORMS:                                # (bf16 tensors must be 8-byte aligned: nothing to misalign)
            c2 = replace(c0, c_off=1, ld_extra=4 - pad // 2, amax="out" if i % 3 == 1 else "")
            out.append(replace(c2, site=site_of(c2, 1, False)))
        parts = "parts" if (i % 3 == 1 and form not in BF16_FORMS) else ""
        out.append(replace(c0, route=f"{kern}-{t}-fwd-{loads}-splitk3-reduce", site="reduce", K=400, nsplit=3, amax=parts or amax))
        if in_kernel_too:
            out.append(replace(c0, route=f"{kern}-{t}-fwd-{loads}-splitk3-inkernel", site="inkernel", K=400, nsplit=3, reduce=2, amax=parts))
        ct = replace(c0, route=f"{kern}-{t}-fwd-{loads}-tail2", M=big_m, N=TAIL_N, K=256, tail=3, amax=amax and "parts" if form not in BF16_FORMS else "")
        out.append(replace(ct, site="tail_" + site_of(ct, 1, False)))
    return out


def _native():
    out = []
    for cfg, (M, N) in ((0, (300, 200)), (1, (100, 72)), (4, (300, 100)), (2, (300, 24)), (3, (20, 300))):
        for layout in ("fwd", "dgrad", "wgrad"):
            form = "l" if layout == "wgrad" else "i"
            for split in (0, 1):
                ns = 3 if split else 1
                for vec in (1, 0):
                    if not vec and cfg in (0, 4):
                        continue                                  # (the scalar-load kernel is built for cfg 1-3 only)
                    # scalar loads: K % 4 != 0 on the K-contiguous layouts (31: one short slab), a base 4 bytes off and an odd ld on wgrad
                    K = (400 if split else 64) if (vec or layout == "wgrad") else (401 if split else 31)
                    sc = dict(a_off=1, op_extra=1) if (not vec and layout == "wgrad") else {}
                    fin = f"splitk{ns}-reduce" if split else "nosplit"
                    out.append(Case(f"native-{_tile(cfg)}-{layout}-{'vec' if vec else 'scalar'}-{fin}", "native_reduce" if split else "native", form,
                                    M, N, K, layout=layout, arith="f32", cfg=cfg + 1, nsplit=ns, ld_extra=4 * vec,
                                    amax="out" if (cfg + split) % 3 == 0 else "", **sc))
    # K = 1 and 6 on the scalar path; reached under F32_F16X3 by M <= 32 / N <= 32
    out.append(Case("native-64x64-fwd-scalar-nosplit", "native", "d", 65, 33, 1, arith="f32", cfg=2, nsplit=1, tag="K1"))
    out.append(Case("native-64x64-dgrad-scalar-nosplit", "native", "i", 64, 65, 6, layout="dgrad", arith="f32", cfg=2, nsplit=1, tag="K6"))
    out.append(Case("native-32x128-fwd-vec-nosplit", "native", "i", 32, 300, 64, arith="f32_f16x3", cfg=4, nsplit=1, tag="f16x3_M32"))
    out.append(Case("native-128x32-fwd-vec-splitk3-reduce", "native_reduce", "d", 300, 32, 400, arith="f32_f16x3", cfg=3, nsplit=3, tag="f16x3_N32"))
    # every form the native kernel takes, at its epilogue and behind its reduction
    for form in "abcdefgijk":
        am = "out" if form in "bdgj" else ""
        out.append(Case("native-128x128-fwd-vec-nosplit", "native", form, 129, 130, 64, arith="f32", cfg=1, nsplit=1, ld_extra=2, amax=am, tag="forms"))
        out.append(Case("native-128x128-fwd-vec-splitk2-reduce", "native_reduce", form, 129, 130, 64, arith="f32", cfg=1, nsplit=2, amax=am, tag="forms"))
    return out


def _split_in_kernel():
    out = []
    for arith in ("f32_bf16x9", "bf16x3", "bf16"):                  # every arithmetic on one layout and one tile (x6, h3: below)
        out.append(Case(f"{KERNEL_OF[arith]}-256x128-fwd-vec-nosplit", "walk", "i", 333, 192, 160, arith=arith, cfg=7, nsplit=1, ld_extra=8))
    for arith in ("f32_f16x3", "f32_bf16x6"):
        k = KERNEL_OF[arith]
        for cfg in (5, 6):
            bm = CFG_BM[cfg]
            for layout in ("fwd", "dgrad", "wgrad"):
                form = "l" if layout == "wgrad" else "i"
                for vec in (1, 0):
                    loads = "vec" if vec else "scalar"
                    # scalar loads: K % 4 != 0 on the K-contiguous layouts, a base 4 bytes off and an odd leading dimension on wgrad
                    sc = dict(a_off=1, op_extra=1) if (not vec and layout == "wgrad") else {}
                    kk = lambda K: K if (vec or layout == "wgrad") else K + 2          # noqa: E731
                    base = dict(form=form, layout=layout, arith=arith, cfg=cfg + 1, **sc)
                    r = f"{k}-{_tile(cfg)}-{layout}-{loads}"
                    site = "misaligned" if not vec else "walk"
                    out.append(Case(f"{r}-nosplit", site, M=bm + 1, N=132, K=kk(48), nsplit=1, c_off=0 if vec else 1, ld_extra=4 if vec else 3,
                                    amax="out" if vec else "", **base))
                    out.append(Case(f"{r}-splitk5-reduce", "reduce", M=2 * bm + 65, N=260, K=kk(1104), nsplit=5, ld_extra=4 * vec, amax="parts" if vec else "", **base))
                    out.append(Case(f"{r}-splitk6-inkernel", "inkernel", M=65, N=129, K=kk(512), nsplit=7, reduce=2, **base))      # (512 / 7 -> ranges of 96: 6 of them)
                    ct = Case(f"{r}-tail2", "", M=TAIL_ROWS * bm + 100, N=TAIL_N, K=kk(256), tail=3, **base)
                    out.append(replace(ct, site="tail_" + site_of(ct, 1, False)))
    return out


def _edges():
    """M and N at 33, 64, 65, one tile, one tile + 1 and several tiles with a ragged last one, on the families that take them"""
    out = []
    for M, N in ((33, 33), (64, 64), (65, 65), (128, 128), (129, 129), (300, 260)):
        tag, rag, pad = f"{M}x{N}", "ragged" if N % 4 else "walk", -N % 4 or 4
        out.append(Case("native-64x64-fwd-vec-nosplit", "native", "i", M, N, 64, arith="f32", cfg=2, nsplit=1, tag=tag))
        out.append(Case("h3-128x128-fwd-vec-nosplit", rag, "i", M, N, 64, cfg=6, nsplit=1, ld_extra=pad, tag=tag))
        out.append(Case("pairs_il-128x128-fwd-dma-nosplit", rag, "i", M, N, 64, fmt="pairs", cfg=9, nsplit=1, ld_extra=pad, tag=tag))
        out.append(Case("wpairs_il-256x128-fwd-dma-nosplit", rag, "i", M, N, 64, fmt="wpairs", nsplit=1, ld_extra=pad, tag=tag))
    for M, N in ((256, 128), (257, 129), (65, 65)):            # one tile and one tile + 1 of the 256-row tiles; the round-3 loops and the plane kernels
        tag, rag, pad = f"{M}x{N}", "ragged" if N % 4 else "walk", -N % 4 or 4
        out.append(Case("h3-256x128-fwd-vec-nosplit", rag, "i", M, N, 64, cfg=7, nsplit=1, ld_extra=pad, tag=tag))
        out.append(Case("x6-256x128-fwd-vec-nosplit", rag, "i", M, N, 64, arith="f32_bf16x6", cfg=7, nsplit=1, ld_extra=pad, tag=tag))
        out.append(Case("pairs_il-256x128-fwd-dma-nosplit", rag, "i", M, N, 64, fmt="pairs", cfg=7, nsplit=1, ld_extra=pad, tag=tag))
        out.append(Case("pairs_il-256x256-fwd-dma-nosplit", rag, "i", M, 2 * N, 64, fmt="pairs", cfg=8, nsplit=1, ld_extra=-2 * N % 4 or 4, tag=f"{M}x{2 * N}"))
        if M != 65:                                            # (65 x 65: above)
            out.append(Case("wpairs_il-256x128-fwd-dma-nosplit", rag, "i", M, N, 64, fmt="wpairs", nsplit=1, ld_extra=pad, tag=tag))
        out.append(Case("pairs_loop-256x128-fwd-dma-nosplit", rag, "i", M, N, 48, fmt="pairs", cfg=7, nsplit=1, ld_extra=pad, tag=tag))
        out.append(Case("wpairs_loop-256x128-fwd-dma-nosplit", rag, "i", M, N, 48, fmt="wpairs", nsplit=1, ld_extra=pad, tag=tag))
        out.append(Case("planes_x6-256x128-fwd-dma-nosplit", rag, "i", M, N, 64, fmt="planes", arith="f32_bf16x6", nsplit=1, ld_extra=pad, tag=tag))
        out.append(Case("wplanes_x6-256x128-fwd-dma-nosplit", rag, "i", M, N, 64, fmt="wplanes", arith="f32_bf16x6", nsplit=1, ld_extra=pad, tag=tag))
    for K in (1, 6, 31):                                       # less than one slab of K on the scalar-load path of the split kernels
        for arith in ("f32_f16x3", "f32_bf16x6"):
            for layout in ("fwd", "dgrad"):
                out.append(Case(f"{KERNEL_OF[arith]}-256x128-{layout}-scalar-nosplit", "walk", "i", 65, 132, K, layout=layout, arith=arith, cfg=7, nsplit=1,
                                ld_extra=4, tag=f"K{K}"))
        out.append(Case("h3-128x128-wgrad-scalar-nosplit", "walk", "l", 65, 132, K, layout="wgrad", cfg=6, nsplit=1, a_off=1, op_extra=1, tag=f"K{K}"))
    return out


def _wide_tails():
    """main + tail launches over several columns of tiles with several tiles in the tail (the other tail cases: one column, one tail tile):
    the tile -> (row, column) mapping from tile_begin and tail tiles that share the slab"""
    out = []
    for kern, cfg, fmt, arith, M, N in (("h3", 5, "f32", "f32_f16x3", 4204, 1024), ("h3", 6, "f32", "f32_f16x3", 8250, 1024), ("x6", 5, "f32", "f32_bf16x6", 4204, 1024),
                                        ("pairs_il", 8, "pairs", "f32_f16x3", 4204, 1024), ("pairs_il", 6, "pairs", "f32_f16x3", 8250, 1024),
                                        ("pairs_il", 7, "pairs", "f32_f16x3", 4312, 4000), ("wpairs_il", 6, "wpairs", "f32_f16x3", 8250, 1024)):
        loads = "vec" if fmt == "f32" else "dma"
        ct = Case(f"{kern}-{_tile(cfg)}-fwd-{loads}-tail2", "", "d", M, N, 256, fmt=fmt, arith=arith, cfg=0 if fmt == "wpairs" else cfg + 1, nsplit=1, tail=3,
                  amax="parts" if cfg == 5 else "", tag="wide")
        out.append(replace(ct, site="tail_" + site_of(ct, 1, False)))
    return out


def _planes():
    out = []
    for layout, tag in (("fwd", ""), ("fwd", "dgrad_planes_of_Wt")):         # weight planes: forward, and dgrad with the planes of W^T
        for arith in ("f32_bf16x9", "f32_bf16x6", "bf16x3", "bf16"):
            x = KERNEL_OF[arith]
            if tag and arith not in ("f32_bf16x6",):
                continue
            out.append(Case(f"wplanes_{x}-256x128-fwd-dma-nosplit", "walk", "i", 300, 200, 96, fmt="wplanes", arith=arith, nsplit=1, ld_extra=4, tag=tag))
    out.append(Case("wplanes_x6-256x128-fwd-dma-splitk2-reduce", "reduce", "d", 300, 200, 512, fmt="wplanes", arith="f32_bf16x6", nsplit=2, amax="out"))
    for arith in ("f32_bf16x9", "f32_bf16x6", "bf16x3"):
        x = KERNEL_OF[arith]
        out.append(Case(f"planes_{x}-256x128-fwd-dma-nosplit", "ragged", "i", 257, 129, 83, fmt="planes", arith=arith, nsplit=1, ld_extra=3))
        out.append(Case(f"planes_{x}-256x128-wgrad-dma-splitk3-reduce", "reduce", "l", 300, 200, 1000, fmt="planes", layout="wgrad", arith=arith, nsplit=3))
    out.append(Case("planes_x6-256x128-wgrad-dma-nosplit", "walk", "l", 96, 72, 300, fmt="planes", layout="wgrad", arith="f32_bf16x6", nsplit=1))
    out.append(Case("planes_x6-256x128-fwd-dma-nosplit", "walk", "n", 300, 200, 96, fmt="planes", arith="f32_bf16x6", nsplit=1, tag="3plane_Cp"))
    out.append(Case("planes_x6-256x128-fwd-dma-splitk2-reduce", "reduce", "n", 300, 200, 512, fmt="planes", arith="f32_bf16x6", nsplit=2, tag="3plane_Cp"))
    # the one-plane bf16 product: the pinned pipeline, and the plane kernel where K % 64 != 0 or the last K range is below 128 columns
    out.append(Case("bf16_il-256x128-fwd-dma-nosplit", "cls11", "m2", 300, 200, 128, fmt="planes", arith="bf16", nsplit=1))
    out.append(Case("bf16_il-256x128-fwd-dma-nosplit", "walk", "i", 513, 260, 192, fmt="planes", arith="bf16", nsplit=1, ld_extra=4))
    out.append(Case("bf16_il-256x128-fwd-dma-splitk2-reduce", "reduce", "d", 300, 200, 512, fmt="planes", arith="bf16", nsplit=2))
    out.append(Case("planes_x1-256x128-fwd-dma-nosplit", "walk", "i", 300, 200, 96, fmt="planes", arith="bf16", nsplit=1, tag="K%64"))
    out.append(Case("planes_x1-256x128-fwd-dma-splitk2-reduce", "reduce", "d", 300, 200, 544, fmt="planes", arith="bf16", nsplit=2, tag="K%64"))
    out.append(Case("planes_x1-256x128-fwd-dma-splitk3-reduce", "reduce", "d", 300, 200, 832, fmt="planes", arith="bf16", nsplit=3, tag="last_range_64"))
    out.append(Case("planes_x1-256x128-wgrad-dma-nosplit", "walk", "l", 96, 72, 300, fmt="planes", layout="wgrad", arith="bf16", nsplit=1))
    return out


def _pairs():
    out = []
    for cfg in (6, 7, 8):
        t, bm, bn = _tile(cfg), CFG_BM[cfg], CFG_BN[cfg]
        base = dict(fmt="pairs", cfg=cfg + 1)
        out.append(Case(f"pairs_il-{t}-fwd-dma-nosplit", "walk", "i", bm + 1, bn + 1 + 3, 64, nsplit=1, ld_extra=4, amax="out", **base))
        out.append(Case(f"pairs_il-{t}-fwd-dma-nosplit", "walk", "i", 3 * bm - 7, 2 * bn + 36, 400, nsplit=1, tag="K400", **base))
        out.append(Case(f"pairs_loop-{t}-fwd-dma-nosplit", "walk", "i", bm + 1, bn + 4, 48, nsplit=1, tag="K48", **base))
        out.append(Case(f"pairs_loop-{t}-fwd-dma-nosplit", "ragged", "d", 65, 33 + 4 * (cfg == 7), 16, nsplit=1, ld_extra=3, tag="K16", **base))
        for K, ns in ((400, 3), (1104, 5), (512, 7)):                # uneven forced cuts: ranges of 160, 224, 96 columns (rounded to 32)
            kern = "pairs_loop" if K == 512 else "pairs_il"          # (512 / 7 -> 5 ranges of 96 and one of 32: below the pipeline's 64)
            out.append(Case(f"{kern}-{t}-fwd-dma-splitk{-(-K // ((-(-K // ns) + 31) // 32 * 32))}-reduce", "reduce", "d", bm + 65, bn + 64, K, nsplit=ns,
                            amax="parts" if K == 400 else "", tag=f"K{K}", **base))
        # a forced split whose last range is short: 96 = 64 + 32 -> the round-3 loop
        out.append(Case(f"pairs_loop-{t}-fwd-dma-splitk2-reduce", "reduce", "d", 300, 200, 96, nsplit=2, tag="last_range_32", **base))
        ct = Case(f"pairs_il-{t}-fwd-dma-tail2", "", "i", TAIL_ROWS * bm + 100, TAIL_N, 256, tail=3, nsplit=0, **base)
        out.append(replace(ct, site="tail_" + site_of(ct, 1, False), nsplit=1))
    return out


def _wpairs():
    b = dict(fmt="wpairs")
    return [
        Case("wpairs_il-256x128-fwd-dma-nosplit", "walk", "i", 300, 200, 64, nsplit=1, ld_extra=4, amax="out", **b),
        Case("wpairs_il-256x128-fwd-dma-nosplit", "cls3", "d", 513, 260, 512, nsplit=1, tag="K512", **b),
        Case("wpairs_loop-256x128-fwd-dma-nosplit", "walk", "i", 300, 200, 48, nsplit=1, tag="K48", **b),
        Case("wpairs_loop-256x128-fwd-dma-nosplit", "ragged", "d", 257, 131, 16, nsplit=1, ld_extra=1, tag="K16", **b),
        Case("wpairs_il-256x128-fwd-dma-splitk3-reduce", "reduce", "d", 300, 200, 416, nsplit=3, amax="parts", **b),
        Case("wpairs_loop-256x128-fwd-dma-splitk2-reduce", "reduce", "d", 300, 200, 96, nsplit=2, tag="last_range_32", **b),
        Case("wpairs_il_nseg-256x128-fwd-dma-nosplit", "cls1", "b", 300, 200, 128, nsplit=1, a_nseg=4, **b),
        Case("wpairs_il_nseg-256x128-fwd-dma-splitk2-reduce", "reduce", "i", 300, 200, 256, nsplit=2, a_nseg=3, **b),
        Case("wpairs_il-256x128-fwd-dma-tail2", "tail_walk", "i", TAIL_ROWS * 256 + 100, TAIL_N, 256, nsplit=1, tail=3, **b),
    ]


def _group4():
    out = []
    ms = [(300, 200, "d"), (65, 132, "i"), (513, 64, "c"), (40, 36, "h")]
    shapes = [(300, 200), (65, 132), (513, 64), (40, 36)]
    for fmt, layout, arith in (("f32", "fwd", "f32_f16x3"), ("f32", "dgrad", "f32_f16x3"), ("pairs", "fwd", "f32_f16x3"), ("f32", "fwd", "f32_bf16x6")):
        for n in (1, 2, 3, 4):
            if arith == "f32_bf16x6" and n != 4:
                continue
            mem = tuple(Case("", "", form, M, N, 96 + 32 * j, fmt=fmt, layout=layout, arith=arith, ld_extra=4 * (j % 2), amax=("out", "", "parts", "")[j],
                             tag=f"m{j}") for j, (M, N, form) in enumerate(ms[:n]))
            kern = "pairs" if fmt == "pairs" else KERNEL_OF[arith]
            out.append(Case(f"group4_{kern}-256x128-{layout}-n{n}", "+".join("g4_" + site_of(m, 1, False) for m in mem), "", 0, 0, 0, entry="group4",
                            fmt=fmt, layout=layout, arith=arith, members=mem))
    # every other form a group member takes (group4_desc_ok: aux, pre, accumulate, bias alone, no epilogue), rotated over the four members
    for fmt, layout in (("f32", "fwd"), ("f32", "dgrad"), ("pairs", "fwd")):
        for forms in ("abef", "gjka", "fkbe"):
            mem = tuple(Case("", "", form, M, N, 96 + 32 * j, fmt=fmt, layout=layout, ld_extra=4 * ((j + 1) % 2), amax=("", "out", "", "parts")[j], tag=f"m{j}")
                        for j, (form, (M, N)) in enumerate(zip(forms, shapes)))
            kern = "pairs" if fmt == "pairs" else "h3"
            out.append(Case(f"group4_{kern}-256x128-{layout}-n4", "+".join("g4_" + site_of(m, 1, False) for m in mem), "", 0, 0, 0, entry="group4",
                            fmt=fmt, layout=layout, members=mem, tag="forms_" + forms))
    return out


def _grouped():
    out = []

    def group(route, site, mem, arith="f32_f16x3", tag=""):
        out.append(Case(route, site, "", 0, 0, 0, entry="grouped", layout="wgrad", arith=arith, members=tuple(mem), tag=tag))

    def member(j, M, N, K, fmt="f32", form=None, **kw):
        return Case("", "", form or ("k", "l")[j % 2], M, N, K, fmt=fmt, layout="wgrad", bcast=(1 if fmt in ("pa", "pab") else 0) | (2 if fmt in ("pb", "pab") else 0),
                    tag=f"m{j}", **kw)

    for n in (1, 8, 9, 16):                  # one shape for all products (the deliberate fault of the second upload chunk needs that)
        group(f"grouped_h3-psrc0-vec-n{n}-chunk{(n + 7) // 8}-nosplit", "grouped", [member(j, 64, 96, 100) for j in range(n)])
    group("grouped_h3-psrc0-scalar-n2-chunk1-nosplit", "grouped", [member(0, 65, 40, 70, op_extra=1), member(1, 64, 48, 33)])
    group("grouped_h3-psrc0-vec-n9-chunk2-mixedsplit", "grouped_reduce", [member(j, 64 + 32 * (j % 3), 96, 2100 if j in (0, 8) else 100 + j) for j in range(9)], tag="ragged")
    group("grouped_h3-psrc0-vec-n3-chunk1-mixedsplit", "grouped_reduce", [member(0, 300, 200, 3000, reduce=1), member(1, 64, 96, 200), member(2, 257, 129, 2049)], tag="reduce1")
    group("grouped_h3-psrc0-vec-n3-chunk1-mixedsplit", "grouped_inkernel", [member(0, 300, 200, 3000, reduce=2), member(1, 64, 96, 200), member(2, 257, 129, 2049)], tag="reduce2")
    group("grouped_x6-psrc0-vec-n2-chunk1-mixedsplit", "grouped_reduce", [member(0, 300, 200, 2100, arith="f32_bf16x6"), member(1, 64, 96, 200, arith="f32_bf16x6")], arith="f32_bf16x6")
    for psrc, fmts in ((1, ("pa", "pa")), (2, ("pb", "pb")), (3, ("pab", "pab")), (4, ("pa", "f32", "pab"))):
        mem = [member(j, 64 + 32 * j, 96, 300 + 2000 * (j == 1), fmt=f) for j, f in enumerate(fmts)]
        group(f"grouped_h3-psrc{psrc}-vec-n{len(mem)}-chunk1-mixedsplit", "grouped_reduce", mem)
    return out


def build_cases():
    cases = _native() + _split_in_kernel() + _variants("h3", 6, "f32", "f32_f16x3", True) + _variants("pairs_il", 8, "pairs", "f32_f16x3", False)
    cases += _edges() + _wide_tails() + _planes() + _pairs() + _wpairs() + _group4() + _grouped()
    return cases


CASES = build_cases()
BY_ID = {c.id: c for c in CASES}


# ------------------------------------------------------------------------------------------------------------------ operands
def _seed(text):
    return zlib.crc32(text.encode())


def operands(c, key=None):
    """the CPU tensors of one product, seeded by the case's id: A and B as stored for the layout (fwd A[M,K] B[N,K]; dgrad A[M,K] B[K,N];
    wgrad A[K,M] B[K,N]), rows of A (of the PRODUCT: columns of the stored wgrad operand) scaled by 2^U(-6, 6) in half of the cases, and the
    epilogue tensors with magnitudes of their own (res 1, aux 3, pre 0.3, old 0.5) so that an addend from the wrong tensor cannot hide"""
    gen = torch.Generator().manual_seed(_seed(key or c.id))
    rnd = lambda *s: torch.randn(*s, generator=gen)            # noqa: E731
    M, N, K, f = c.M, c.N, c.K, c.f
    a = rnd(M, K)
    if c.rows_scaled if key is None else bool(_seed(key) & 1):
        a = a * torch.exp2(torch.rand(M, 1, generator=gen) * 12 - 6)
    b = rnd(N, K) * 0.05
    o = dict(A=a if c.layout != "wgrad" else a.t().contiguous(), B=b if c.layout == "fwd" else b.t().contiguous())
    o["bias"] = rnd(N) if f["bias"] else None
    o["res"] = rnd(M, N) if (f["res"] or f["resp"]) else None
    o["aux"] = torch.nn.functional.elu(3.0 * rnd(M, N)) if (f["aux"] or f["auxp"]) else None
    o["pre"] = 0.3 * rnd(M, N) if f["pre"] else None
    o["old"] = 0.5 * rnd(M, N) if f["acc"] else None
    o["colsum_old"] = 0.5 * rnd(M) if f["colsum"] else None
    if f["res_ln"]:
        o["res"] = 3.0 * o["res"] + 1.0
        x = o["res"].double()
        o["ln"] = (x.mean(1).float(), (1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5)).float(), rnd(N), rnd(N))
    else:
        o["ln"] = None
    if f["resp"]:
        o["res"] = o["res"].to(torch.bfloat16).float() if f["resp"] == 1 else o["res"]
    if f["auxp"]:
        o["aux"] = o["aux"].to(torch.bfloat16).float()
    if c.arith == "bf16" and c.fmt == "planes":              # the one-plane product is GIVEN bf16 operands
        o["A"], o["B"] = o["A"].to(torch.bfloat16).float(), o["B"].to(torch.bfloat16).float()
    return o


def reference(c, o, seed, salt=0):
    """-> (C64, OUT64, colsum64, terms) of one product by kernel_refs.gemm_ref64 / gemm_terms"""
    f = c.f
    kw = dict(pre=o["pre"], bias=o["bias"], drop_p=f["drop"], drop_seed=seed, drop_salt=salt, res=o["res"], res_ln=o["ln"], old=o["old"])
    C64, OUT64, cs = kr.gemm_ref64(o["A"], o["B"], c.layout, act=f["act"], aux=o["aux"], two_outputs=bool(f["c2"] or f["c1p"]), a_colsum_old=o["colsum_old"], **kw)
    return C64, OUT64, cs, kr.gemm_terms(o["A"], o["B"], c.layout, amax_bcast=c.bcast, **kw)


def products(cases=None):
    """every single product of the table (group members one by one) with the key that seeds its operands"""
    for c in cases or CASES:
        if c.members:
            for m in c.members:
                yield m, f"{c.id}/{m.tag}"
        else:
            yield c, None


def calibrate(cases=None, verbose=False):
    """-> (r of torch.matmul, r of the block-of-8 chain): max |fp32 CPU - float64| / (u32 S) over the products of the table"""
    r_mm = r_ch = 0.0
    for c, key in products(cases):
        o = operands(c, key)
        a, b = kr.gemm_operands64(o["A"], o["B"], c.layout)
        want, S = a @ b.t(), (a.abs() @ b.abs().t()).clamp_min(1e-300)
        mm = float(((a.float() @ b.float().t()).double() - want).abs().div(kr.U32 * S).max())
        ch = float((kr.matmul_chain32(a.float(), b.float()).double() - want).abs().div(kr.U32 * S).max())
        if verbose:
            print(f"{c.id if key is None else key}: matmul {mm:.2f} chain {ch:.2f}", flush=True)
        r_mm, r_ch = max(r_mm, mm), max(r_ch, ch)
    return r_mm, r_ch


# ------------------------------------------------------------------------------------------------------------------ refusals
def _first(pred):
    return next(c.id for c in CASES if pred(c))


def _set(i=0, **kw):
    def mutate(prods):
        for k, v in kw.items():
            setattr(prods[i].d, k, v(prods[i].d) if callable(v) else v)
    return mutate


def _all(**kw):
    def mutate(prods):
        for p in prods:
            for k, v in kw.items():
                setattr(p.d, k, v(p.d) if callable(v) else v)
    return mutate


_H3 = _first(lambda c: c.route == "h3-256x128-fwd-vec-nosplit" and c.form == "d" and c.site == "cls3")
_H3_AMAX = _first(lambda c: c.route == "h3-256x128-fwd-vec-nosplit" and c.amax == "out")
_H3_LN = _first(lambda c: c.route == "h3-256x128-fwd-vec-nosplit" and c.form == "h")
_H3_WGRAD = _first(lambda c: c.route == "h3-256x128-wgrad-vec-nosplit")
_M1 = _first(lambda c: c.route == "h3-256x128-fwd-vec-nosplit" and c.form == "m1" and c.site == "cls9")
_M4 = _first(lambda c: c.route == "h3-256x128-fwd-vec-nosplit" and c.form == "m4" and c.N % 4 == 0)
_NATIVE = _first(lambda c: c.route == "native-128x128-fwd-vec-nosplit" and c.form == "d")
_NATIVE_AMAX = _first(lambda c: c.route.startswith("native-128x128-fwd-vec-nosplit") and c.amax == "out")
_PAIRS = _first(lambda c: c.route == "pairs_il-256x128-fwd-dma-nosplit")
_WPAIRS = _first(lambda c: c.route == "wpairs_il-256x128-fwd-dma-nosplit")
_WPAIRS_LOOP = _first(lambda c: c.route == "wpairs_loop-256x128-fwd-dma-nosplit")
_WPLANES = _first(lambda c: c.route == "wplanes_x6-256x128-fwd-dma-nosplit")
_PLANES = _first(lambda c: c.route == "planes_x6-256x128-fwd-dma-nosplit")
_G4 = _first(lambda c: c.route == "group4_h3-256x128-fwd-n2")
_G4_4 = _first(lambda c: c.route == "group4_h3-256x128-fwd-n4")
_G4_PAIRS = _first(lambda c: c.route == "group4_pairs-256x128-fwd-n1")
_GROUPED = _first(lambda c: c.route == "grouped_h3-psrc0-vec-n1-chunk1-nosplit")
_GROUPED_8 = _first(lambda c: c.route == "grouped_h3-psrc0-vec-n8-chunk1-nosplit")
_GROUPED_PA = _first(lambda c: c.route.startswith("grouped_h3-psrc1-"))

# name -> (the valid record it starts from, the change that makes the library refuse it); the comment names the line of gemm_f32.hip
REFUSALS = {
    # grappa_gemm_f32
    "single-null_A": (_H3, _set(A=None)),                                               # !d->A
    "single-no_output": (_H3, _set(C=None)),                                            # !C && !Cp && !C1p
    "single-c2_without_c": (_M1, _set(C2=lambda d: d.Cp, ldc2=64)),                     # !C && (C2 || accumulate)
    "single-accumulate_without_c": (_M1, _set(accumulate=1)),
    "single-c1p_with_c": (_M4, _set(C=lambda d: d.Cp, ldc=64)),                         # C1p && (C || C2)
    "single-c1p_without_cp": (_M4, _set(Cp=None)),                                      # C1p && !Cp
    "single-nplanes_2": (_M1, _set(cp_nplanes=2)),                                      # *_nplanes not in {0, 1, 3}
    "single-a_planes_alone": (_PAIRS, _set(b_planes=0)),                                # a_planes && !b_planes
    "single-pair_operands_in_the_wgrad_layout": (_WPAIRS, _set(a_kcontig=0, b_kcontig=0)),   # ABI 8 operands: the grouped entry only
    "single-pairs_amax_bcast": (_PAIRS, _set(amax_bcast=1)),                            # pairs && (... amax_bcast || a_colsum)
    "single-pairs_a_colsum": (_PAIRS, _set(a_colsum=lambda d: d.C)),
    "single-wpairs_K_not_16": (_WPAIRS, _set(K=40)),                                    # weight pairs: K & 15
    "single-wpairs_lda_odd": (_WPAIRS, _set(lda=lambda d: d.lda + 1)),
    "single-planes_M32": (_WPLANES, _set(M=32)),                                        # planes: M <= 32 || N <= 32
    "single-planes_layout_mixed": (_PLANES, _set(b_kcontig=0)),                         # planes: a_kcontig != b_kcontig
    "single-planes_lda_short": (_PLANES, _set(lda=lambda d: d.lda - 32)),               # both in planes: ld < padded row
    "single-wpairs_ldb_short": (_WPAIRS, _set(ldb=lambda d: d.ldb - 64)),               # weight pairs: ldb < 2 * kpad
    "single-wplanes_K_not_32": (_WPLANES, _set(K=80)),                                  # weight planes: K & 31
    "single-wplanes_ldb_short": (_WPLANES, _set(ldb=lambda d: d.ldb - 32)),
    "single-cp_ld_odd": (_M1, _set(ldcp=lambda d: d.ldcp + 1)),                         # !al8(Cp, ldcp)
    "single-negative_M": (_H3, _set(M=-1)),                                             # M < 0
    "single-K_zero": (_H3, _set(K=0)),                                                  # K == 0
    "single-layout_a_kmajor_b_kcontig": (_H3, _set(a_kcontig=0)),                       # a_kcontig == 0 && b_kcontig == 1
    "single-drop_p_one": (_H3, _set(drop_p=1.0)),                                       # drop_p outside [0, 1)
    "single-precision_7": (_H3, _set(precision=7)),                                     # precision out of range
    "single-f16x3_without_amax": (_H3, _set(a_amax=None)),                              # F32_F16X3 needs a_amax / b_amax
    "single-native_with_resp": (_NATIVE, _set(resp=lambda d: d.res, ldresp=64)),        # the native kernel takes no bf16 tensors
    "single-res_ln_with_aux": (_H3_LN, _set(aux=lambda d: d.res, ldaux=lambda d: d.ldres)),   # res_ln_* with aux
    "single-res_ln_without_gamma": (_H3_LN, _set(res_ln_gamma=None)),                   # res_ln_*: all four arrays
    "single-res_ln_on_native": (_NATIVE, _set(res_ln_mean=lambda d: d.bias, res_ln_rstd=lambda d: d.bias, res_ln_gamma=lambda d: d.bias,
                                              res_ln_beta=lambda d: d.bias)),            # res_ln_*: the split kernels only
    "single-forced_tile_without_kernel": (_H3, _set(plan_cfg=1)),                       # pl.main_tiles <= 0
    "single-wpairs_forced_256x256": (_WPAIRS, _set(plan_cfg=8)),                        # weight pairs: the 256 x 128 tile only
    "single-a_colsum_on_kcontig_A": (_H3, _set(a_colsum=lambda d: d.C)),                # a_colsum && a_kcontig
    "single-plan_tail_4": (_H3, _set(plan_tail=4)),                                     # plan options out of range
    "single-splitk_reduce_3": (_H3, _set(splitk_reduce=3)),
    "single-parts_on_native": (_NATIVE_AMAX, _set(out_amax_parts=lambda d: d.out_amax, out_amax=None)),   # out_amax_parts && !bf16x
    "single-parts_and_out_amax": (_H3_AMAX, _set(out_amax_parts=lambda d: d.out_amax)),
    "single-nseg_on_wgrad": (_H3_WGRAD, _set(a_amax_nseg=2)),                           # a_amax_nseg > 1 && !a_kcontig
    "single-nseg_on_pairs": (_PAIRS, _set(a_amax_nseg=2)),                              # ... && planes && !wpairs_il_ok
    "single-wpairs_nseg_on_loop": (_WPAIRS_LOOP, _set(a_amax_nseg=2)),
    "single-nseg_with_bcast": (_H3, _set(a_amax_nseg=2, amax_bcast=1)),
    # group4_desc_ok
    "group4-null_C": (_G4, _set(1, C=None)),
    "group4-cp": (_G4, _set(1, Cp=lambda d: d.C, ldcp=64)),
    "group4-M32": (_G4, _set(1, M=32)),
    "group4-a_kmajor": (_G4, _set(1, a_kcontig=0)),
    "group4-precision_differs": (_G4, _set(1, precision=2)),
    "group4-native_precision": (_G4, _all(precision=0)),
    "group4-layout_differs": (_G4, _set(1, b_kcontig=0)),
    "group4-format_differs": (_G4, _set(1, b_planes=1)),
    "group4-drop_p_one": (_G4, _set(1, drop_p=1.0)),
    "group4-weight_pairs": (_G4, _all(b_planes=1)),
    "group4-f16x3_without_amax": (_G4, _set(1, b_amax=None)),
    "group4-pairs_lda_short": (_G4_PAIRS, _set(0, lda=lambda d: d.lda - 64)),
    "group4-scalar_loads": (_G4, _set(1, K=lambda d: d.K - 1)),
    "group4-parts_and_out_amax": (_G4, _set(0, out_amax_parts=lambda d: d.out_amax)),
    "group4-nseg_with_bcast": (_G4, _set(1, a_amax_nseg=2, amax_bcast=1)),
    "group4-res_ln_without_rstd": (_G4_4, _set(3, res_ln_rstd=None)),
    # group_desc_ok and grappa_gemm_f32_grouped
    "grouped-a_kcontig": (_GROUPED, _set(a_kcontig=1)),
    "grouped-pair_operand_without_rowmax": (_GROUPED, _set(a_planes=1)),
    "grouped-pair_operand_without_bcast": (_GROUPED_PA, _set(amax_bcast=0)),
    "grouped-out_amax": (_GROUPED, _set(out_amax=lambda d: d.C)),
    "grouped-N32": (_GROUPED, _set(N=32)),
    "grouped-native_precision": (_GROUPED, _set(precision=0)),
    "grouped-precision_differs": (_GROUPED_8, _set(3, precision=2)),
    "grouped-f16x3_without_amax": (_GROUPED, _set(a_amax=None)),
    "grouped-drop_p_negative": (_GROUPED, _set(drop_p=-0.5)),
    "grouped-pairs_with_a_scalar_partner": (_GROUPED_PA, _set(ldb=lambda d: d.ldb + 1)),
}
